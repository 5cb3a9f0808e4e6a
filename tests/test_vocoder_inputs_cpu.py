"""The random inputs of tests/test_gpu_vocoder_kernels.py do what those tests rely on -- checked with the float64 reference alone (no GPU, no
kernel): the gates are driven through their saturated range, the whole-generator inputs make every block's auxiliary term and dilation visible
far above the asserted bound, and the utterance-length lists really put edges inside tiles and utterances below the dilation.  A later edit of the
builders in helpers.py that turns them back into linear-regime inputs fails here."""
import math

import numpy as np
import pytest
import torch

import helpers as H


def _stats(z, half):
    ta, sg = z[:, :half].abs(), z[:, half:]
    return dict(beyond10=float((ta > 10).double().mean()), mid=float(((ta >= 1) & (ta <= 10)).double().mean()), sig_min=float(sg.min()),
                sig_max=float(sg.max()), finite=bool(torch.isfinite(z).all()))


FEATURES_GIVEN = ([("four_launch", r, aux, k) for r in (32, 96) for aux in (20, 100) for k in (3, 5)] + [("small_aux", 64, aux, 3) for aux in (4, 32, 64)]
                  + [("persistent", 64, aux, 3) for aux in (68, 80, 96)] + [("bf16", 64, aux, 3) for aux in (32, 80)])


def _assert_saturated(zs, half, what):
    st = _stats(torch.cat(zs), half)
    print(what, st)
    assert st["finite"] and st["beyond10"] >= 0.05 and st["mid"] >= 0.25 and st["sig_min"] < -20 and st["sig_max"] > 20, (what, st)


@pytest.mark.parametrize("group,r,aux,ksize", FEATURES_GIVEN)
def test_single_block_inputs_saturate_the_gate(group, r, aux, ksize):
    """the weights and activations of every features-given cell of the GPU file (same builders, same seeds), per dilation, pooled over the four
    utterance-length lists (957 samples): at dilation 512 only the centre tap and the auxiliary term are left, and the fractions must still hold"""
    seed = H.PWG_BLOCK_SEEDS[group]
    sd, _ = H.pwg_block_state_dict(seed, r, aux, ksize)
    w = H.pwg_layer_weights_f64(sd, 0)
    for d in H.PWG_BLOCK_DILATIONS:
        zs = []
        for m, lens in sorted(H.PWG_BLOCK_SAMPLE_LENS.items()):
            inp = H.pwg_block_sample_inputs(seed, m, r, aux)
            x, a = torch.from_numpy(inp["x"]).double(), torch.from_numpy(inp["feats"]).double() @ w["aux"].t()
            s0 = 0
            for n in lens:
                out = H.pwg_block_f64(x[s0 : s0 + n], a[s0 : s0 + n], w, d)
                zs.append(out["z"])
                assert bool(torch.isfinite(out["x_out"]).all()) and bool(torch.isfinite(out["skip"]).all())
                s0 += n
        _assert_saturated(zs, r, (group, r, aux, ksize, d))


FRAME_RATE = ([("frame_rate", aux, sc) for aux in (20, 80, 96) for sc in ((2, 4, 4, 4), (4, 4, 4, 4), (4, 4, 4, 6))] + [("capacity", 80, (4, 4, 4, 4))])


@pytest.mark.parametrize("group,aux,scales", FRAME_RATE)
def test_frame_rate_block_inputs_saturate_the_gate(group, aux, scales):
    """the same for the cells whose auxiliary term comes from mels through the upsampling network, frame lists pooled per dilation"""
    seed = H.PWG_BLOCK_SEEDS[group]
    sd, cfg = H.pwg_block_state_dict(seed, 64, aux, 3, scales)
    w = H.pwg_layer_weights_f64(sd, 0)
    hop = int(np.prod(scales))
    cases = []
    for i, lens in enumerate(H.PWG_BLOCK_FRAME_LENS):
        mels, x, _ = H.pwg_block_frame_inputs(seed + i, lens, hop, 64, aux)
        s0 = 0
        for mel in mels:
            n = mel.shape[0] * hop
            cases.append((torch.from_numpy(x[s0 : s0 + n]).double(), H.pwg_features_f64(sd, mel, cfg) @ w["aux"].t()))
            s0 += n
    for d in H.PWG_BLOCK_DILATIONS:
        _assert_saturated([H.pwg_block_f64(x, a, w, d)["z"] for x, a in cases], 64, (group, aux, hop, d))


GENERATORS = {"v1": (None, H.PWG_GENERATOR_LENS), "small": (H.PWG_SMALL_CFG, H.PWG_SMALL_LENS)}


@pytest.fixture(scope="module", params=sorted(GENERATORS))
def gen(request):
    """the whole-generator inputs of the GPU file (same builder, same seed, same lens): float64 reference and its plane-rounded error model"""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cfg, lens = GENERATORS[request.param]
    sd, mels, noise = H.pwg_generator_inputs(H.PWG_GENERATOR_SEEDS[request.param], lens, cfg)
    ref = [H.pwg_generator_f64(sd, m, z, cfg) for m, z in zip(mels, noise)]
    model = [H.pwg_generator_f64(sd, m, z, cfg, rnd=H.plane_round) for m, z in zip(mels, noise)]
    return request.param, sd, H.pwg_cfg(cfg), ref, model


def test_generator_inputs_reach_saturation_and_audible_level(gen):
    name, sd, cfg, ref, _ = gen
    half = cfg["gate_channels"] // 2
    st = _stats(torch.cat([z for r in ref for z in r["zs"]]), half)
    peaks = [float(r["wav"].abs().max()) for r in ref]
    print(name, "waveform peaks", peaks, "tap peak %.2f" % max(float(t.abs().max()) for r in ref for t in r["taps"]), st)
    assert st["finite"] and min(peaks) >= 0.1
    assert st["beyond10"] >= 0.005 and st["mid"] >= 0.5


def test_generator_reference_sees_every_blocks_auxiliary_term_and_dilation(gen):
    """Sensitivity of the whole-generator tests, a property of the reference alone: removing block l's auxiliary term, or halving its dilation
    (1 -> 2), moves block l's tap by more than 100 x the bound test_gpu_vocoder_kernels asserts for that tap,
    4 * max(err_model, 2**-15 * max|tap|), err_model = the float64 generator on plane-rounded GEMM operands against the exact one; taps
    concatenated over the batch's utterances as the GPU test compares them."""
    name, sd, cfg, ref, model = gen
    lps = cfg["layers"] // cfg["stacks"]
    worst = None
    for l in range(cfg["layers"]):
        tap = torch.cat([r["taps"][l] for r in ref])
        bound = 4 * max(float((torch.cat([m["taps"][l] for m in model]) - tap).abs().max()), 2.0 ** -15 * float(tap.abs().max()))
        w = H.pwg_layer_weights_f64(sd, l)
        d = 2 ** (l % lps)
        no_aux = half_d = 0.0
        for r in ref:
            aux, x = r["c_up"] @ w["aux"].t(), r["xin"][l]
            assert float((H.pwg_block_f64(x, aux, w, d)["x_out"] - r["taps"][l]).abs().max()) == 0.0
            no_aux = max(no_aux, float((H.pwg_block_f64(x, None, w, d)["x_out"] - r["taps"][l]).abs().max()))
            half_d = max(half_d, float((H.pwg_block_f64(x, aux, w, d // 2 if d > 1 else 2)["x_out"] - r["taps"][l]).abs().max()))
        ratio = min(no_aux, half_d) / bound
        worst = ratio if worst is None else min(worst, ratio)
        assert no_aux > 100 * bound and half_d > 100 * bound, (name, l, no_aux, half_d, bound)
    print("%s: smallest mutation / bound ratio over %d blocks: %.0f" % (name, cfg["layers"], worst))


def test_utterance_length_lists_give_the_claimed_edges():
    S = H.PWG_BLOCK_SAMPLE_LENS
    assert sorted(S) == [1, 127, 129, 700] and all(sum(v) == k for k, v in S.items())
    for m in (127, 129, 700):
        edges = np.cumsum(S[m])[:-1]
        assert any(e % 128 for e in edges)  # an utterance edge inside a 128-row tile
        assert m % 128  # ragged last tile
    edges = np.cumsum(S[700])[:-1]
    assert sum(1 for e in edges if e < 128) >= 3  # several edges inside ONE tile
    assert 1 in S[700] and 1 in S[127]  # a one-sample utterance
    assert min(S[700]) < 2 and any(n < 64 for n in S[129]) and all(n < 512 for v in S.values() for n in v)  # shorter than the dilation
    assert any(n > 2 * 64 for n in S[700])  # ... and one long enough for both taps of dilation 64 to stay inside
    F = H.PWG_BLOCK_FRAME_LENS
    assert F == [[1], [1, 1, 1], [3, 1, 33, 2]]
    utt = lambda off, m: int(np.searchsorted(off, m, side="right")) - 1 if 0 <= m < off[-1] else None  # utterance that owns sample m (None: outside)
    for hop in (128, 256, 384):
        one = np.array([0, hop])  # [1]: at dilation 512 both taps of every sample fall outside the only utterance
        assert all(utt(one, m - 512) is None and utt(one, m + 512) is None for m in (0, hop - 1))
        off = np.cumsum([0] + [n * hop for n in F[2]])  # [3, 1, 33, 2]
        assert utt(off, off[1] + 512) == 2  # from the one-frame utterance (index 1) the right tap lands in the NEIGHBOURING 33-frame utterance
        assert utt(off, off[2] + hop - 512) in (None, 0, 1)  # from the 33-frame one a left tap lands in an earlier utterance or before the batch
        assert utt(off, off[2] - 512) != 2 and utt(off, off[2] + 512) == 2  # its first sample: the left tap leaves, the right tap stays inside
        mid = (off[2] + off[3]) // 2
        assert utt(off, mid - 512) == 2 and utt(off, mid + 512) == 2  # samples in its middle keep both taps
        assert utt(off, off[3] - 1 + 512) is None or utt(off, off[3] - 1 + 512) == 3  # its last sample: the right tap leaves
    G = H.PWG_GENERATOR_LENS
    assert sum(G) == 70 and 1 in G and max(G) == 33  # frames on every position mod 32 incl. the window switch, a one-frame utterance
    assert math.prod(H.PWG_SMALL_CFG["upsample_scales"]) % 128 != 0 and H.PWG_SMALL_CFG["aux_channels"] <= 64  # -> pwg_layer_kernel<4,3>
    assert (sum(H.PWG_SMALL_LENS) * 6) % 128 != 0
    assert sum(H.PWG_LONG_LENS) * 2 > 2 * 256 and 1 in H.PWG_LONG_LENS  # more than twice as many 128-sample tiles as an MI355X has compute units
