"""Shared test helpers: closed-form state_dicts as torch tensors, tiny hparams used by the goldens; float64 references and seeded random
inputs of the vocoder tests."""
import math

import numpy as np
import torch

import fcl_taco2_amd  # noqa: F401
from fcl_taco2_amd import hparams as HP
from fcl_taco2_amd import synthetic as SYN

TINY_S = HP.student_hparams(idim=12, odim=8, embed_dim=16, eunits=16, econv_chans=16, dunits=24, prenet_units=20,
                            postnet_chans=12, duration_predictor_chans=20, dropout_rate=0.0)
TINY_T = HP.teacher_hparams(idim=12, odim=8, embed_dim=32, eunits=32, econv_chans=32, dunits=40, prenet_units=28,
                            postnet_chans=20, duration_predictor_chans=20, dropout_rate=0.0)
# the train-mode goldens (G7, G9) use the same shapes (hence the same closed-form weights) with the shipped dropout rate
TINY_S7 = HP.student_hparams(idim=12, odim=8, embed_dim=16, eunits=16, econv_chans=16, dunits=24, prenet_units=20,
                             postnet_chans=12, duration_predictor_chans=20, dropout_rate=0.5)
TINY_T7 = HP.teacher_hparams(idim=12, odim=8, embed_dim=32, eunits=32, econv_chans=32, dunits=40, prenet_units=28,
                             postnet_chans=20, duration_predictor_chans=20, dropout_rate=0.5)


def np_state_dict(hp, thp=None, share_proj=True):
    return SYN.closed_form_state_dict(HP.param_spec(hp, thp, share_proj))


def torch_state_dict(hp, thp=None, share_proj=True):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in np_state_dict(hp, thp, share_proj).items()}


def max_abs(a, b):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    b = b.detach().cpu().numpy() if hasattr(b, "detach") else np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)))) if a.size else 0.0

# the `--use-masking False` loss variant (G10): same shapes / weights as TINY_S / TINY_T
TINY_SU = HP.student_hparams(idim=12, odim=8, embed_dim=16, eunits=16, econv_chans=16, dunits=24, prenet_units=20,
                             postnet_chans=12, duration_predictor_chans=20, dropout_rate=0.0, use_masking=False)
TINY_TU = HP.teacher_hparams(idim=12, odim=8, embed_dim=32, eunits=32, econv_chans=32, dunits=40, prenet_units=28,
                             postnet_chans=20, duration_predictor_chans=20, dropout_rate=0.0, use_masking=False)

# the `--use-residual True` variant (G11): same shapes / weights, encoder convs with skip connections
TINY_SR = HP.student_hparams(idim=12, odim=8, embed_dim=16, eunits=16, econv_chans=16, dunits=24, prenet_units=20,
                             postnet_chans=12, duration_predictor_chans=20, dropout_rate=0.0, use_residual=True)
TINY_TR = HP.teacher_hparams(idim=12, odim=8, embed_dim=32, eunits=32, econv_chans=32, dunits=40, prenet_units=28,
                             postnet_chans=20, duration_predictor_chans=20, dropout_rate=0.0, use_residual=True)

# the `--output-activation sigmoid` variant (G12): same shapes / weights, outputs through torch.nn.functional.sigmoid
TINY_SA = HP.student_hparams(idim=12, odim=8, embed_dim=16, eunits=16, econv_chans=16, dunits=24, prenet_units=20,
                             postnet_chans=12, duration_predictor_chans=20, dropout_rate=0.0, output_activation="sigmoid")
TINY_TA = HP.teacher_hparams(idim=12, odim=8, embed_dim=32, eunits=32, econv_chans=32, dunits=40, prenet_units=28,
                             postnet_chans=20, duration_predictor_chans=20, dropout_rate=0.0, output_activation="sigmoid")

# decoder options outside the shipped recipes (G14): zoneout_rate 0 (plain LSTMCell, no `.cell` key level), use_concate False, append_position False;
# the KD pair keeps use_concate (the reference's KD decoder cannot run forward() without it: tests/golden/records.json)
_OPT = dict(idim=12, odim=8, duration_predictor_chans=20, dropout_rate=0.0, zoneout_rate=0.0, append_position=False)
TINY_TO = HP.teacher_hparams(embed_dim=32, eunits=32, econv_chans=32, dunits=40, prenet_units=28, postnet_chans=20, use_concate=False, **_OPT)
TINY_SO = HP.student_hparams(embed_dim=16, eunits=16, econv_chans=16, dunits=24, prenet_units=20, postnet_chans=12, use_concate=False, **_OPT)
TINY_TOK = HP.teacher_hparams(embed_dim=32, eunits=32, econv_chans=32, dunits=40, prenet_units=28, postnet_chans=20, **_OPT)
TINY_SOK = HP.student_hparams(embed_dim=16, eunits=16, econv_chans=16, dunits=24, prenet_units=20, postnet_chans=12, **_OPT)

# `--use-batch-norm false` (G15): encoder / postnet blocks without a normalisation layer
_NOBN = dict(idim=12, odim=8, duration_predictor_chans=20, dropout_rate=0.0, use_batch_norm=False)
TINY_TN = HP.teacher_hparams(embed_dim=32, eunits=32, econv_chans=32, dunits=40, prenet_units=28, postnet_chans=20, **_NOBN)
TINY_SN = HP.student_hparams(embed_dim=16, eunits=16, econv_chans=16, dunits=24, prenet_units=20, postnet_chans=12, **_NOBN)

# encoder widths that all differ (G16; every shipped recipe sets embed_dim == econv_chans == eunits)
_WID = dict(idim=12, odim=8, duration_predictor_chans=20, dropout_rate=0.0)
TINY_TW = HP.teacher_hparams(embed_dim=24, econv_chans=32, eunits=40, dunits=40, prenet_units=28, postnet_chans=20, **_WID)
TINY_SW = HP.student_hparams(embed_dim=12, econv_chans=16, eunits=24, dunits=24, prenet_units=20, postnet_chans=12, **_WID)

# layer counts outside the shipped recipes that the reference's teacher class runs (G17): two encoder blocks, three postnet blocks
TINY_TL = HP.teacher_hparams(idim=12, odim=8, embed_dim=32, eunits=32, econv_chans=32, dunits=40, prenet_units=28, postnet_chans=20,
                             duration_predictor_chans=20, dropout_rate=0.0, econv_layers=2, postnet_layers=3)

# speaker embeddings (G13): F.normalize(spemb) appended to the encoder states; predictors / embeddings / decoder on eunits + 8 channels
TINY_TK = HP.teacher_hparams(idim=12, odim=8, embed_dim=32, eunits=32, econv_chans=32, dunits=40, prenet_units=28,
                             postnet_chans=20, duration_predictor_chans=20, dropout_rate=0.0, spk_embed_dim=8)

# structure options of the reference's teacher class beyond the shipped recipes (G18 - G20, round 5): decoder cell count, prenet block count,
# stacked encoder BiLSTM
_OPT = dict(idim=12, odim=8, embed_dim=32, eunits=32, econv_chans=32, dunits=40, prenet_units=28, postnet_chans=20, duration_predictor_chans=20, dropout_rate=0.0)
TINY_VARIANTS = {
    "g18_teacher_dlayers1": HP.teacher_hparams(dlayers=1, **_OPT),
    "g18_teacher_dlayers3": HP.teacher_hparams(dlayers=3, **_OPT),
    "g19_teacher_prenet1": HP.teacher_hparams(prenet_layers=1, **_OPT),
    "g19_teacher_prenet3": HP.teacher_hparams(prenet_layers=3, **_OPT),
    "g20_teacher_elayers2": HP.teacher_hparams(elayers=2, **_OPT),
}

# reduction_factor 2 on the teacher class (G21)
TINY_R2 = HP.teacher_hparams(reduction_factor=2, **_OPT)

# the KD classes with the structure options their tap lists allow (G22): teacher with three prenet blocks, student with one; two BiLSTM layers each
_KDS = dict(idim=12, odim=8, duration_predictor_chans=20, dropout_rate=0.0, elayers=2)
TINY_TQ = HP.teacher_hparams(embed_dim=32, eunits=32, econv_chans=32, dunits=40, prenet_units=28, postnet_chans=20, prenet_layers=3, **_KDS)
TINY_SQ = HP.student_hparams(embed_dim=16, eunits=16, econv_chans=16, dunits=24, prenet_units=20, postnet_chans=12, prenet_layers=1, **_KDS)


# ---- Parallel WaveGAN vocoder: float64 references and seeded random inputs (tests/test_gpu_vocoder_kernels.py, tests/test_vocoder_inputs_cpu.py) ----
# Plain numpy / torch from the published algebra (header of csrc/pwg.hip, include/fcl_hip.h); nothing here calls a kernel of the library.
# Layout as on the device: rows are samples (or frames), channels are columns; every function sees ONE utterance, so its edges are real zero padding.
def bf16_rn(x):
    """numpy restatement of the device's float -> bf16 conversion (round to nearest even), as the uint16 bit pattern."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_to_f32(h):
    return (h.astype(np.uint32) << 16).view(np.float32)


def split_planes_np(x):
    """[R, K] float32 -> P32 planes uint16 [R, ceil(K/32), 2, 32] (include/fcl_hip.h: hi = bf16_rn(x), lo = bf16_rn(x - hi), zeros past K)."""
    r, k = x.shape
    kp = (k + 31) // 32 * 32
    xp = np.zeros((r, kp), np.float32)
    xp[:, :k] = x
    hi = bf16_rn(xp)
    lo = bf16_rn(xp - bf16_to_f32(hi))
    return np.stack([hi.reshape(r, kp // 32, 32), lo.reshape(r, kp // 32, 32)], axis=2)


def plane_round(t):
    """float64 tensor -> the value its P32 planes carry (hi + lo of the float32 rounding), as float64."""
    x = t.to(torch.float32)
    hi = x.to(torch.bfloat16).to(torch.float32)
    lo = (x - hi).to(torch.bfloat16).to(torch.float32)
    return hi.to(torch.float64) + lo.to(torch.float64)


def bf16_round(t):
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def pwg_shift(x, sh):
    """rows t -> x[t + sh], zero where t + sh leaves the utterance"""
    out = torch.zeros_like(x)
    n = x.shape[0]
    if sh >= 0:
        if sh < n:
            out[: n - sh] = x[sh:]
    elif -sh < n:
        out[-sh:] = x[: n + sh]
    return out


def pwg_block_f64(x, aux_term, w, d, rnd=None, rnd_g=None, x_op=None):
    """One residual block on ONE utterance in float64.  x [T, R]; aux_term [T, 2R] (conv1x1_aux of the upsampled features, or None);
    w: dict conv [2R, R, k], b_conv, out [R, R], b_out, skip [S, R], b_skip (float64 tensors).  rnd / rnd_g: optional rounding of the first GEMM's
    operands / of the gate output and W_os (the operand-format error model); x_op: the convolution's operand when it is not rnd(x).  Returns z (pre-activations), g, x_out, skip."""
    rnd = rnd or (lambda t: t)
    rnd_g = rnd_g or rnd
    k = w["conv"].shape[2]
    xr = rnd(x) if x_op is None else x_op
    z = w["b_conv"].clone().expand(x.shape[0], -1).clone()
    for j in range(k):
        z = z + pwg_shift(xr, (j - (k - 1) // 2) * d) @ rnd(w["conv"][:, :, j]).t()
    if aux_term is not None:
        z = z + aux_term
    half = z.shape[1] // 2
    g = torch.tanh(z[:, :half]) * torch.sigmoid(z[:, half:])
    gr = rnd_g(g)
    x_out = (gr @ rnd_g(w["out"]).t() + w["b_out"] + x) * math.sqrt(0.5)
    skip = gr @ rnd_g(w["skip"]).t() + w["b_skip"]
    return dict(z=z, g=g, x_out=x_out, skip=skip)


def pwg_conv_in_f64(mel, w_in, ctx):
    """replicate padding by ctx frames + conv_in (no bias, 'valid'): mel [T', A] -> [T', A]"""
    n = mel.shape[0]
    pad = mel[torch.clamp(torch.arange(-ctx, n + ctx), 0, n - 1)]
    return sum(pad[j : j + n] @ w_in[:, :, j].t() for j in range(w_in.shape[2]))


def pwg_stage_f64(c, s, w):
    """one upsampling stage on one utterance: nearest stretch by s + the zero-padded 1 x (2s+1) smoothing convolution w (cross-correlation)"""
    st = torch.repeat_interleave(c, s, dim=0)
    return sum(float(w[j + s]) * pwg_shift(st, j) for j in range(-s, s + 1))


def pwg_upsample_f64(c_in, scales, up_w):
    for s, w in zip(scales, up_w):
        c_in = pwg_stage_f64(c_in, s, w)
    return c_in


def pwg_cfg(cfg=None):
    from oracle import pwg_oracle as O

    return dict(O.CONFIG, **(cfg or {}))


def pwg_layer_weights_f64(sd, l):
    p = "conv_layers.%d." % l
    t = lambda k: torch.from_numpy(np.asarray(sd[k])).to(torch.float64)
    return dict(conv=t(p + "conv.weight"), b_conv=t(p + "conv.bias"), aux=t(p + "conv1x1_aux.weight")[:, :, 0], out=t(p + "conv1x1_out.weight")[:, :, 0],
                b_out=t(p + "conv1x1_out.bias"), skip=t(p + "conv1x1_skip.weight")[:, :, 0], b_skip=t(p + "conv1x1_skip.bias"))


def pwg_features_f64(sd, mel, cfg=None):
    """upsample_net on one utterance: mel [T', A] -> upsampled features [T' * hop, A] (float64)"""
    cfg = pwg_cfg(cfg)
    t = lambda k: torch.from_numpy(np.asarray(sd[k])).to(torch.float64)
    c_in = pwg_conv_in_f64(torch.as_tensor(mel).to(torch.float64), t("upsample_net.conv_in.weight"), cfg["aux_context_window"])
    ups = [t("upsample_net.upsample.up_layers.%d.weight" % (2 * i + 1)).reshape(-1) for i in range(len(cfg["upsample_scales"]))]
    return pwg_upsample_f64(c_in, cfg["upsample_scales"], ups)


def pwg_generator_f64(sd, mel, z, cfg=None, rnd=None):
    """The whole generator on ONE utterance in float64: mel [T', A], noise z [T' * hop].  rnd: rounding applied to every GEMM operand (x, features,
    gate output, ReLU(skips), weights) -- the plane-format error model; None = exact.  Returns taps (x after every block), xin (x before every block),
    zs (pre-activations), c_up, skips (the unscaled sum) and wav."""
    cfg = pwg_cfg(cfg)
    r = rnd or (lambda v: v)
    t = lambda k: torch.from_numpy(np.asarray(sd[k])).to(torch.float64)
    c_up = pwg_features_f64(sd, mel, cfg)
    x = torch.as_tensor(z).to(torch.float64).reshape(-1, 1) * t("first_conv.weight").reshape(1, -1) + t("first_conv.bias")
    lps = cfg["layers"] // cfg["stacks"]
    taps, xin, zs, skips = [], [], [], 0
    c_r = r(c_up)
    for l in range(cfg["layers"]):
        w = pwg_layer_weights_f64(sd, l)
        out = pwg_block_f64(x, c_r @ r(w["aux"]).t(), w, 2 ** (l % lps), rnd)
        xin.append(x)
        x = out["x_out"]
        skips = skips + out["skip"]
        taps.append(x)
        zs.append(out["z"])
    y = torch.relu(skips * math.sqrt(1.0 / cfg["layers"]))
    h = torch.relu(r(y) @ r(t("last_conv_layers.1.weight")[:, :, 0]).t() + t("last_conv_layers.1.bias"))
    wav = h @ t("last_conv_layers.3.weight").reshape(-1) + t("last_conv_layers.3.bias").reshape(())
    return dict(taps=taps, xin=xin, zs=zs, c_up=c_up, skips=skips, wav=wav)


def pwg_random_state_dict(rng, cfg=None, gain=4.0):
    """Seeded random generator weights at a gain that drives the gates into saturation (tests/test_vocoder_inputs_cpu.py asserts that it does): dilated
    convolutions and conv1x1_aux gain * N(0,1) / sqrt(fan_in), every other convolution N(0,1) / sqrt(fan_in), biases 0.5 N(0,1), smoothing
    weights (1 + 0.5 N(0,1)) / (2s+1)."""
    from oracle import pwg_oracle as O

    sd = {}
    for k, shp in O.param_spec(cfg).items():
        if k.endswith("bias"):
            v = 0.5 * rng.standard_normal(shp)
        elif "up_layers" in k:
            v = (1.0 + 0.5 * rng.standard_normal(shp)) / shp[-1]
        else:
            fan_in = int(np.prod(shp[1:]))
            g = gain if (k.endswith("conv.weight") or "conv1x1_aux" in k) and k.startswith("conv_layers") else 1.0
            v = g * rng.standard_normal(shp) / math.sqrt(fan_in)
        sd[k] = np.ascontiguousarray(v, dtype=np.float32)
    return sd


def pwg_generator_inputs(seed, lens, cfg=None, gain=4.0):
    """(state dict, mels, noise) of the whole-generator tests: random weights (pwg_random_state_dict), mel and noise N(0,1)."""
    cfg_full = pwg_cfg(cfg)
    rng = np.random.RandomState(seed)
    sd = pwg_random_state_dict(rng, cfg, gain)
    hop = int(np.prod(cfg_full["upsample_scales"]))
    mels = [rng.standard_normal((n, cfg_full["aux_channels"])).astype(np.float32) for n in lens]
    noise = [rng.standard_normal(n * hop).astype(np.float32) for n in lens]
    return sd, mels, noise


PWG_BLOCK_GAIN = 2.0  # gain of the dilated-conv / conv1x1_aux weights of the single-block tests (pwg_random_state_dict)


def pwg_block_cfg(r, aux, ksize=3, scales=(2,)):
    return dict(layers=1, stacks=1, residual_channels=r, gate_channels=2 * r, skip_channels=r, aux_channels=aux, kernel_size=ksize, upsample_scales=tuple(scales))


def pwg_block_inputs(rng, m, r, aux):
    """Seeded random activations of ONE teacher-forced residual block at a scale that saturates the gate: x = 3 N(0,1), features 2.5 N(0,1),
    skips-so-far 2 N(0,1); with the weights of pwg_random_state_dict(gain = PWG_BLOCK_GAIN) the pre-activation std is ~8, and ~6 where a dilation
    leaves only the centre tap inside the utterance.  float32 numpy arrays."""
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    return dict(x=np.float32(3.0) * f(m, r), feats=np.float32(2.5) * f(m, aux), skips=np.float32(2.0) * f(m, r))


# Seeds and builders of the single-block cases: test_gpu_vocoder_kernels.py runs them on the device, test_vocoder_inputs_cpu.py checks the very same
# arrays with the reference alone.
PWG_BLOCK_SEEDS = dict(four_launch=100, small_aux=200, persistent=300, frame_rate=400, capacity=500, bf16=600, bf16_frame_rate=700)


def pwg_block_state_dict(seed, r, aux, ksize=3, scales=(2,)):
    """(state dict, cfg) of a one-block generator: the block's weights and, for the frame-rate cases, the upsampling network's"""
    cfg = pwg_block_cfg(r, aux, ksize, scales)
    return pwg_random_state_dict(np.random.RandomState(seed + r + aux + ksize), cfg, PWG_BLOCK_GAIN), cfg


def pwg_block_sample_inputs(seed, m, r, aux):
    """x / feats / skips of the features-given case with m samples"""
    return pwg_block_inputs(np.random.RandomState(seed + m), m, r, aux)


def pwg_block_frame_inputs(seed, lens, hop, r, aux):
    """(mels per utterance = 2.5 N(0,1), x = 3 N(0,1), skips-so-far = 2 N(0,1)) of a case whose auxiliary term comes from mels; lens in frames"""
    rng = np.random.RandomState(seed)
    mels = [(2.5 * rng.standard_normal((n, aux))).astype(np.float32) for n in lens]
    m = sum(lens) * hop
    return mels, (3.0 * rng.standard_normal((m, r))).astype(np.float32), (2.0 * rng.standard_normal((m, r))).astype(np.float32)


# utterance-length lists of the single-block tests (features given: samples; frame-rate term: frames).  What each one provides is asserted in
# tests/test_vocoder_inputs_cpu.py.
PWG_BLOCK_SAMPLE_LENS = {1: [1], 127: [60, 1, 66], 129: [100, 29], 700: [3, 1, 50, 17, 129, 300, 200]}
PWG_BLOCK_FRAME_LENS = [[1], [1, 1, 1], [3, 1, 33, 2]]
PWG_BLOCK_DILATIONS = (1, 2, 64, 512)
PWG_GENERATOR_LENS = [29, 3, 1, 33, 2, 2]
PWG_SMALL_CFG = dict(layers=30, stacks=3, residual_channels=64, gate_channels=128, skip_channels=64, aux_channels=32, upsample_scales=(2, 3))
PWG_SMALL_LENS = [200, 1, 90]
PWG_GENERATOR_SEEDS = dict(v1=21, small=22, long=23)
PWG_LONG_LENS = [150, 1, 140]  # 291 frames = 582 tiles at hop 256: more tiles than the device has compute units, so a workgroup of the persistent block walks several


def seg_bounds(lens):
    """per-row [lo, hi) of its utterance, int32"""
    lens = np.asarray(lens, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens)])
    return np.repeat(off[:-1], lens).astype(np.int32), np.repeat(off[1:], lens).astype(np.int32)


def decoder_case(ops, hp, n_rows, seed, forced, masked, dur=None, dev="cuda:0"):
    """One fcl_decoder_loop_fwd pass (closed-form weights, want_taps) and O.decoder_loop on the same inputs: ((before, taps), (ref_before, ref_taps)),
    frame-major on the CPU.  dur: per-row durations, sorted descending (default: seeded Poisson draws); forced: teacher forcing on random frames;
    masked: DROP_MASK with the closed-form keep masks (else DROP_NONE)."""
    from fcl_taco2_amd.plan import SynthesisPlan
    from oracle import fcl_oracle as O

    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev).contiguous()  # noqa: E731
    rng = np.random.RandomState(seed)
    sd = torch_state_dict(hp)
    plan = SynthesisPlan(np_state_dict(hp), hp, dev)
    if dur is None:
        dur = np.sort(np.clip(rng.poisson(6, n_rows), 1, 30))[::-1].astype(np.int32).copy()
    lmax = int(dur[0])
    att = rng.standard_normal((n_rows, hp.eunits)).astype(np.float32)
    foff = np.concatenate([[0], np.cumsum(dur)[:-1]]).astype(np.int32)
    F_ = int(dur.sum())
    live = np.ascontiguousarray((dur[None, :] > np.arange(lmax)[:, None]).sum(1).astype(np.int32))
    ys = rng.standard_normal((n_rows, lmax, hp.odim)).astype(np.float32) if forced else None
    keep = SYN.closed_form_keep_mask((lmax, 2, n_rows, hp.prenet_units), seed) if masked else None
    before, taps = ops.decoder_loop(plan.decoder, d(att), d(dur), live, d(foff), F_,
                                    teacher_ys=d(ys) if ys is not None else None,
                                    dropout_mode=ops.DROP_MASK if masked else ops.DROP_NONE,
                                    prenet_keep=d(keep) if masked else None, want_taps=True)
    pos = O.position_table(torch.from_numpy(dur))
    with torch.no_grad():
        outs, pres, l0, l1 = O.decoder_loop(sd, hp, torch.from_numpy(att), pos, lmax,
                                            torch.from_numpy(ys) if ys is not None else None,
                                            torch.from_numpy(keep) if masked else None)
    mask = torch.from_numpy(dur[:, None] > np.arange(lmax)[None, :])
    return (before.cpu(), [t.cpu() for t in taps]), (outs.transpose(1, 2)[mask], [pres[mask], l0[mask], l1[mask]])
