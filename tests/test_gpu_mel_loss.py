"""The msl_* kernels of csrc/stft_loss.hip, the autograd module on them and `evaluate --aligned --aligned-mel` against the float64 statement of
tests/mel_loss_ref.py.  Every buffer a kernel writes sits between guard zones filled with a NaN bit pattern, which must survive; every
kernel test reads the library's launch record and fails if its kernels did not run.  The inputs, their bounds and the conditions both have to meet
are built and checked in mel_loss_ref.py / test_mel_loss_cpu.py."""
import functools
import json

import numpy as np
import pytest
import torch

import mel_loss_ref as M
from test_gpu_features import DEV, Guarded, launched
from test_gpu_stft_loss import Guarded64, _write_wav, grads_of, split

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
S = M.S


@pytest.fixture(scope="module")
def ML():
    assert torch.cuda.is_available()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, mel_loss

    _lib.load()
    return mel_loss


@functools.lru_cache(maxsize=None)
def reference(case, silent=False):
    """computed once per case and shared, read-only"""
    xs, ys = M.signals(case, silent=silent)
    assert M.conditions(case, xs, ys) == 1.0
    ref = M.kernel_reference(case, xs, ys, "utterance")
    for v in list(ref.values()) + ref["grad"] + xs + ys:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return xs, ys, ref


def kernel_names(n_fft):
    return ("msl_sums_kernel<%d>" % n_fft, "msl_utt_sums_kernel", "msl_grad_frames_kernel<%d>" % n_fft, "stl_grad_gather_kernel")


def plan_of(ML, case):
    basis = [M.filterbank(case)] if case[3] == "hand" else None
    return ML.MelLossPlan(DEV, M.MEL["fs"], [case[0]], [case[1]], [case[2]], 80 if basis else case[3], M.MEL["fmin"], M.MEL["fmax"], basis)


def run(ML, case, xs, ys, coef):
    """both entries on guarded buffers -> (maps, frame_sums, utt_sums, gx)"""
    rs = plan_of(ML, case).resolutions[0]
    mp = ML.Maps([len(x) for x in xs], rs.hop, DEV)
    n = sum(len(x) for x in xs)
    x, y = Guarded(n).set(np.concatenate(xs)), Guarded(n).set(np.concatenate(ys))
    fs, us = Guarded(mp.frames), Guarded64(mp.n_utt)
    cf, fr, gx = Guarded(mp.n_utt).set(coef), Guarded(mp.frames, rs.n_fft), Guarded(n)
    with launched(*kernel_names(rs.n_fft)):
        ML.launch_sums(rs, mp, x.t, y.t, fs.t, us.t)
        ML.launch_grad(rs, mp, x.t, y.t, cf.t, fr.t, gx.t)
    assert all(b.intact() for b in (x, y, fs, us, cf, fr, gx))
    return mp, fs, us, gx


@pytest.mark.parametrize("case", M.CASES, ids=str)
def test_sums_and_gradient_vs_float64(ML, case):
    """frame_sums, utt_sums and gx of one packed batch of three utterances within the derived bounds of mel_loss_ref.py: 80, 13 and 256 mels and the
    hand-made matrix (an all-zero row, a bin under four channels that are no run, bands out of order); the coefficients are the float64
    reference's, rounded to float32"""
    xs, ys, ref = reference(case)
    rs = plan_of(ML, case).resolutions[0]
    held = ML.dense_from_transpose(rs.bt_off, rs.bt_ch, rs.bt_w.astype(np.float32).astype(np.float64), rs.n_mels)
    assert np.allclose(held, ref["B"], rtol=2 * U, atol=0.0) and np.array_equal(held != 0, ref["B"] != 0)  # the device's weights: the reference's to one rounding
    mp, fs, us, gx = run(ML, case, xs, ys, ref["coef"])
    assert mp.frames == len(ref["frame_sums"])
    r_f = (np.abs(fs.np() - ref["frame_sums"]) / ref["frame_bounds"]).max()
    r_u = (np.abs(us.np() - ref["utt_sums"]) / ref["utt_bounds"]).max()
    g = split(gx.np(), [len(x) for x in xs])
    r_g = np.array([np.linalg.norm(a - b) / e for a, b, e in zip(g, ref["grad"], ref["grad_bounds"])])
    print("mel loss %r: worst share of the bound: frame sums %.3g, utterance sums %.3g, gradient %s" % (case, r_f, r_u, r_g))
    assert np.isfinite(fs.np()).all() and np.isfinite(us.np()).all() and np.isfinite(gx.np()).all()
    assert r_f <= 1.0 and r_u <= 1.0 and r_g.max() <= 1.0


def test_silent_utterance_has_an_exactly_zero_gradient(ML):
    """x = 0 in the middle of the batch: every bin of it sits at the floor, its gradient is bit-exact 0.0 (its mels do not sit at their floor: dl is
    not zero, the magnitude floor stops it), its sums meet their bounds and the neighbours' results are those of the batch without silence"""
    case = M.SILENT_CASE
    xs, ys, ref = reference(case, True)
    _, _, ref0 = reference(case)
    assert ref["grad_bounds"][1] == 0.0
    mp, fs, us, gx = run(ML, case, xs, ys, ref["coef"])
    lens = [len(x) for x in xs]
    g = split(gx.np(), lens)
    assert g[1].tobytes() == np.zeros(lens[1]).tobytes()
    assert (np.abs(fs.np() - ref["frame_sums"]) <= ref["frame_bounds"]).all() and (np.abs(us.np() - ref["utt_sums"]) <= ref["utt_bounds"]).all()
    _, fs0, us0, gx0 = run(ML, case, *reference(case)[:2], ref0["coef"])
    g0, f, f0 = split(gx0.np(), lens), split(fs.np(), mp.lens), split(fs0.np(), mp.lens)
    for i in (0, 2):
        assert g[i].tobytes() == g0[i].tobytes() and f[i].tobytes() == f0[i].tobytes() and us.np()[i].tobytes() == us0.np()[i].tobytes()


@pytest.mark.parametrize("case", [(512, 50, 240, 80), (1024, 256, 1024, 13), (2048, 240, 1200, 80)], ids=str)
def test_batch_equals_per_utterance_runs_bit_for_bit(ML, case):
    """one packed batch against three runs of one utterance (another slot of the workgroup, another block: the same bits) and against itself"""
    xs, ys, ref = reference(case)
    mp, fs, us, gx = run(ML, case, xs, ys, ref["coef"])
    _, fs2, us2, gx2 = run(ML, case, xs, ys, ref["coef"])
    assert fs.bits() == fs2.bits() and us.bits() == us2.bits() and gx.bits() == gx2.bits()
    f = split(fs.t.cpu().numpy(), mp.lens)
    g = split(gx.t.cpu().numpy(), [len(x) for x in xs])
    for i in range(len(xs)):
        _, fs1, us1, gx1 = run(ML, case, [xs[i]], [ys[i]], ref["coef"][i : i + 1])
        assert fs1.bits() == f[i].tobytes() and us1.bits() == us.np()[i : i + 1].tobytes() and gx1.bits() == g[i].tobytes(), i


def test_accumulate_over_two_resolutions_is_the_sum_of_the_single_runs(ML):
    """the second resolution's launch with accumulate adds its gradient to the first's: the float32 sum of the two single runs, bit for bit, and
    within the combined bound of the float64 sum"""
    c1, c2 = (512, 50, 240, 80), (512, 50, 240, "hand")
    xs, ys, r1 = reference(c1)
    assert M.conditions(c2, xs, ys) == 1.0  # the first case's signals under the second matrix
    r2 = M.kernel_reference(c2, xs, ys, "utterance")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
    x, y = t(np.concatenate(xs)), t(np.concatenate(ys))
    singles = []
    gx = Guarded(x.numel())
    for i, (case, ref) in enumerate(((c1, r1), (c2, r2))):
        rs = plan_of(ML, case).resolutions[0]
        mp = ML.Maps([len(v) for v in xs], rs.hop, DEV)
        fr, own = torch.empty(mp.frames, rs.n_fft, device=DEV), torch.empty_like(x)
        ML.launch_grad(rs, mp, x, y, t(ref["coef"]), fr, own)
        ML.launch_grad(rs, mp, x, y, t(ref["coef"]), fr, gx.t, accumulate=i > 0)
        singles.append(own)
    assert torch.equal(gx.t, singles[0] + singles[1]) and gx.intact()
    lens = [len(v) for v in xs]
    for a, b1, b2, e1, e2 in zip(split(gx.np(), lens), r1["grad"], r2["grad"], r1["grad_bounds"], r2["grad_bounds"]):
        assert np.linalg.norm(a - b1 - b2) <= e1 + e2 + 2 * U * (np.linalg.norm(b1) + np.linalg.norm(b2))


def test_module_batch_reduction_on_equal_length_clips(ML):
    """[B, T] = [2, 2100], reduction="batch", three resolutions: the loss and x.grad after backward() against the float64 statement within the
    bounds combined over the resolutions; [B, 1, T] gives the same bits; the default plan is the single resolution of features.DEFAULTS"""
    xs, ys = M.module_signals()
    ref = M.module_reference(xs, ys, M.THREE_RESOLUTIONS, "batch")
    cfg = list(zip(*[c[:3] for c in M.THREE_RESOLUTIONS]))
    loss = ML.MelSpectrogramLoss(DEV, fft_sizes=cfg[0], hop_sizes=cfg[1], win_lengths=cfg[2])
    assert ML.MelSpectrogramLoss(DEV).plan.configs == [c[:3] for c in M.DEFAULT_RESOLUTIONS]
    x = torch.from_numpy(np.stack(xs)).to(DEV).requires_grad_(True)
    y = torch.from_numpy(np.stack(ys)).to(DEV)
    names = [n for c in M.THREE_RESOLUTIONS for n in kernel_names(c[0])]
    with launched(*names):
        val = loss(x, y)
        val.backward()
    assert val.dtype == torch.float32 and val.dim() == 0 and x.grad.shape == x.shape
    r_g = [np.linalg.norm(a - b) / e for a, b, e in zip(grads_of(x, [M.MODULE_T] * M.MODULE_B), ref["grad"], ref["grad_bounds"])]
    print("module, batch: loss %.7f (|d| %.2e of %.2e), gradient share of the bound %s" % (val.item(), abs(val.item() - ref["loss"]), ref["loss_bound"], r_g))
    assert abs(val.item() - ref["loss"]) <= ref["loss_bound"] and max(r_g) <= 1.0
    x3 = x.detach().clone()[:, None, :].requires_grad_(True)
    val3 = loss(x3, y[:, None, :])
    val3.backward()
    assert torch.equal(val3, val) and torch.equal(x3.grad[:, 0], x.grad)
    keep = loss._maps
    loss(x.detach(), y)
    assert loss._maps is keep  # the maps are kept for the next batch of the same lengths


def test_module_utterance_reduction_on_ragged_input(ML):
    """reduction="utterance" on a ragged packed batch against float64; the padded [B, T] + lens form gives the same values and an exactly zero
    gradient in the padding; distances() gives each utterance's own figure"""
    xs, ys = M.ragged_signals()
    lens = [len(v) for v in xs]
    ref = M.module_reference(xs, ys, M.THREE_RESOLUTIONS, "utterance")
    cfg = list(zip(*[c[:3] for c in M.THREE_RESOLUTIONS]))
    loss = ML.MelSpectrogramLoss(DEV, fft_sizes=cfg[0], hop_sizes=cfg[1], win_lengths=cfg[2])
    x = torch.from_numpy(np.concatenate(xs)).to(DEV).requires_grad_(True)
    y = torch.from_numpy(np.concatenate(ys)).to(DEV)
    val = loss(x, y, lens=lens, reduction="utterance")
    val.backward()
    r_g = [np.linalg.norm(a - b) / e for a, b, e in zip(grads_of(x, lens), ref["grad"], ref["grad_bounds"])]
    print("module, utterance: |d loss| %.2e of %.2e, gradient share of the bound %s" % (abs(val.item() - ref["loss"]), ref["loss_bound"], r_g))
    assert abs(val.item() - ref["loss"]) <= ref["loss_bound"] and max(r_g) <= 1.0
    T = max(lens) + 37
    pad = lambda vs, fill: torch.from_numpy(np.stack([np.concatenate([v, np.full(T - len(v), fill, np.float32)]) for v in vs])).to(DEV)
    xp, yp = pad(xs, 0.25).requires_grad_(True), pad(ys, -0.5)  # the padding holds values that would matter if it were read
    valp = loss(xp, yp, lens=lens, reduction="utterance")
    valp.backward()
    assert torch.equal(valp, val)
    for b, n in enumerate(lens):
        assert torch.equal(xp.grad[b, :n], x.grad[sum(lens[:b]) : sum(lens[:b]) + n]) and not bool(xp.grad[b, n:].any())
    d = loss.distances(x.detach(), lens, y)
    assert d.shape == (3, 3) and abs(d.mean() - val.item()) <= 4 * U * val.item()
    with pytest.raises(ValueError, match="utterance tiny has 1024 samples"):
        loss(torch.zeros(3000, device=DEV), torch.zeros(3000, device=DEV), lens=[1976, 1024], ids=["ok", "tiny"])


def test_module_inside_a_graph_as_the_generator_term(ML):
    """x = 0.9 z made by a torch operation, the loss 45 mel(x, y) as in HiFi-GAN's generator: z.grad against the float64 statement (0.9 times the
    gradient at x, the bound scaled alike plus the rounding of the product); y.requires_grad and an unknown reduction are refused"""
    zs, ys = M.module_signals()
    xs = [(np.float32(0.9) * z).astype(np.float32) for z in zs]  # what the device computes
    assert all(M.conditions(c, xs, ys) == 1.0 for c in M.THREE_RESOLUTIONS)
    ref = M.module_reference(xs, ys, M.THREE_RESOLUTIONS, "batch", 45.0)
    cfg = list(zip(*[c[:3] for c in M.THREE_RESOLUTIONS]))
    loss = ML.MelSpectrogramLoss(DEV, fft_sizes=cfg[0], hop_sizes=cfg[1], win_lengths=cfg[2])
    z = torch.from_numpy(np.stack(zs)).to(DEV).requires_grad_(True)
    y = torch.from_numpy(np.stack(ys)).to(DEV)
    x = 0.9 * z
    assert np.array_equal(x.detach().cpu().numpy(), np.stack(xs))
    val = loss(x, y)
    (45.0 * val).backward()
    want = [np.float64(np.float32(0.9)) * g for g in ref["grad"]]
    r_g = [np.linalg.norm(a - b) / (0.9 * e + 2 * U * np.linalg.norm(b)) for a, b, e in zip(grads_of(z, [M.MODULE_T] * M.MODULE_B), want, ref["grad_bounds"])]
    print("module in a graph: gradient share of the bound %s" % r_g)
    assert abs(val.item() - ref["loss"]) <= ref["loss_bound"] and max(r_g) <= 1.0
    with pytest.raises(ValueError, match="must not require a gradient"):
        loss(x.detach(), y.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="reduction"):
        loss(x.detach(), y, reduction="mean")


def test_evaluate_aligned_mel_driver(ML, tmp_path):
    """python -m fcl_taco2_amd.evaluate --aligned --aligned-mel on three tiny wav pairs: the records carry distances()'s values on the pairs cut to
    the shorter side, the corpus figure is their mean, and without the flag the document is the one --aligned alone gives"""
    from fcl_taco2_amd import evaluate as E

    rd, sd = tmp_path / "ref", tmp_path / "syn"
    rd.mkdir()
    sd.mkdir()
    ids, L, extra = ["ua", "ub", "uc"], [4500, 5200, 4800], [0, 100, -60]
    refs, syns = {}, {}
    for i, (u, n, e) in enumerate(zip(ids, L, extra)):
        y = 0.5 * S.R.signal(60 + i, n + max(e, 0))
        refs[u] = _write_wav(rd / (u + ".wav"), y[:n])
        syns[u] = _write_wav(sd / (u + "_gen.wav"), 0.8 * y[: n + e] + 0.02 * S.R.signal(90 + i, n + e))
    out = tmp_path / "m.json"
    base = ["--ref-wav-dir", str(rd), "--syn-wav-dir", str(sd), "--aligned", "--verbose", "0", "--aligned-batch-samples", "10000"]
    with launched("msl_sums_kernel<1024>", "msl_utt_sums_kernel"):
        doc = E.main(base + ["--aligned-mel", "--out", str(out)])
    assert json.loads(out.read_text()) == doc and doc["settings"]["aligned"]["mel"] == dict(n_mels=80, mel_basis=None)
    n = [min(len(refs[u]), len(syns[u])) for u in ids]
    loss = ML.MelSpectrogramLoss(DEV)
    d = loss.distances([syns[u][:k] for u, k in zip(ids, n)], None, [refs[u][:k] for u, k in zip(ids, n)])
    case = M.DEFAULT_RESOLUTIONS[0]
    for k, r in enumerate(doc["utterances"]):
        assert r["id"] == ids[k] and r["mel_l1"] == float(d[k, 0]) and "stft_sc" in r
        want = M.figure(*M.utt_sums([syns[ids[k]][: n[k]]], [refs[ids[k]][: n[k]]], M.window(case), case[1], M.filterbank(case)), "utterance")
        assert np.isclose(d[k, 0], want, rtol=1e-4)  # against float64, loosely (the kernels' own bounds are the tests' above)
    assert doc["mel_l1"] == float(np.mean([r["mel_l1"] for r in doc["utterances"]]))
    assert E.summary_line(doc).endswith(", mel L1 %.4f" % doc["mel_l1"])
    plain = E.main(base)
    assert "mel_l1" not in plain and "mel" not in plain["settings"]["aligned"] and "mel L1" not in E.summary_line(plain)
    strip = lambda q: {k: v for k, v in q.items() if k != "mel_l1"}
    assert [strip(r) for r in doc["utterances"]] == plain["utterances"] and E.summary_line(doc).startswith(E.summary_line(plain))
