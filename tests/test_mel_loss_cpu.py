"""The float64 statement of the mel-spectrogram loss (tests/mel_loss_ref.py) without a GPU: the inputs of tests/test_gpu_mel_loss.py meet
the conditions their bounds assume, the statement agrees with torch.stft + matmul + log10 + autograd, a float32 evaluation stays inside every bound
and every mutant leaves its bound; then the filterbank's bin-major transpose, the C ABI's argument checks and the evaluation driver's flag."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mel_loss_ref as M

S = M.S
CASES = M.CASES
REDUCTIONS = ("utterance", "batch")
WIDE = [c for c in CASES if c[2] == 240]  # the cases whose short window tells the symmetric Hann from the periodic one


@functools.lru_cache(maxsize=None)
def reference(case, reduction):
    xs, ys = M.signals(case)
    return xs, ys, M.kernel_reference(case, xs, ys, reduction)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b))


@pytest.mark.parametrize("case", CASES, ids=str)
def test_inputs_meet_the_conditions_of_the_bounds(case):
    """asserted before anything else is: neither floor and no sign of l_x - l_y can flip within its error, p >= 4e-10 on every bin that carries
    weight -- in 100 % of the bins and cells, in float64 alone"""
    xs, ys = M.signals(case)
    assert [len(x) for x in xs] == M.lengths(case)
    assert M.conditions(case, xs, ys) == 1.0
    if case == M.SILENT_CASE:
        w = M.window(case)
        zs, _ = M.signals(case, silent=True)
        assert not np.any(zs[1]) and M.all_floored(zs[1], w, case[1]) and all(np.array_equal(zs[i], xs[i]) for i in (0, 2))
        qs, _ = M.floored_signals(case)
        assert np.all(qs[1] != 0) and M.all_floored(qs[1], w, case[1])
    _, _, ref = reference(case, "utterance")
    print("mel loss %r: gradient bound / gradient norm per utterance %s" % (case, np.round(ref["grad_bounds"] / [np.linalg.norm(g) for g in ref["grad"]], 5)))


def test_module_inputs_meet_the_conditions():
    for xs, ys in (M.module_signals(), M.ragged_signals()):
        assert all(M.conditions(c, xs, ys) == 1.0 for c in M.THREE_RESOLUTIONS)
    zs, ys = M.module_signals()
    assert all(M.conditions(c, [(np.float32(0.9) * z).astype(np.float32) for z in zs], ys) == 1.0 for c in M.THREE_RESOLUTIONS)
    assert M.DEFAULT_RESOLUTIONS[0] == M.THREE_RESOLUTIONS[0]


def test_hand_made_basis_has_the_features_the_transpose_is_tested_on():
    B = M.hand_basis()
    nz = B != 0
    assert not nz[2].any() and (nz.sum(0) >= 3).any()
    k = int(np.argmax(nz.sum(0) >= 3))
    assert np.flatnonzero(nz[:, k]).tolist() == [0, 3, 5]  # no contiguous run of channels
    first = [int(np.argmax(r)) for r in nz if r.any()]
    assert first != sorted(first)


@pytest.mark.parametrize("reduction", REDUCTIONS)
@pytest.mark.parametrize("case", CASES + ["silent"], ids=str)
def test_numpy_statement_equals_torch_in_float64(case, reduction):
    """(a) loss and gradient to 1e-10 relative on ragged lengths, an upstream gradient other than 1; the silent utterance's gradient is exactly zero
    in both"""
    silent = case == "silent"
    case = M.SILENT_CASE if silent else case
    xs, ys = M.signals(case, silent=silent)
    val, grad = M.torch_statement(xs, ys, [case], reduction, 45.0)
    nval, ngrad = M.loss(xs, ys, [case], reduction), M.gradient(xs, ys, case, 45.0, reduction)
    worst = max(rel(a, b) for u, (a, b) in enumerate(zip(ngrad, grad)) if not (silent and u == 1))
    print("numpy against torch, %r %s: loss %.3g, gradient %.3g relative" % (case, reduction, abs(val - nval) / val, worst))
    assert abs(val - nval) <= 1e-10 * val and worst <= 1e-10
    if silent:
        assert not np.any(ngrad[1]) and not np.any(grad[1])


def test_numpy_statement_equals_torch_on_three_resolutions():
    for (xs, ys), reduction in ((M.module_signals(), "batch"), (M.ragged_signals(), "utterance")):
        val, grad = M.torch_statement(xs, ys, M.THREE_RESOLUTIONS, reduction)
        assert abs(val - M.loss(xs, ys, M.THREE_RESOLUTIONS, reduction)) <= 1e-10 * val
        per = [M.gradient(xs, ys, c, 1.0 / 3, reduction) for c in M.THREE_RESOLUTIONS]
        assert all(rel(sum(p[u] for p in per), grad[u]) <= 1e-10 for u in range(len(xs)))
        ref = M.module_reference(xs, ys, M.THREE_RESOLUTIONS, reduction)  # on the float32-rounded weights: 1e-7 away
        assert abs(ref["loss"] - val) <= 1e-6 * val and all(rel(a, b) <= 1e-5 for a, b in zip(ref["grad"], grad))


@pytest.mark.parametrize("reduction", REDUCTIONS)
@pytest.mark.parametrize("case", CASES, ids=str)
def test_float32_evaluation_stays_inside_every_bound(case, reduction):
    """(b) torch.stft + matmul + log10 + autograd in float32 on the CPU: frame sums, utterance sums and gradient within the derived bounds"""
    xs, ys, ref = reference(case, reduction)
    _, grad, frames = M.torch_statement(xs, ys, [case], reduction, dtype=torch.float32, bases=[ref["B"]], detail=True)
    use_f = (np.abs(frames[0] - ref["frame_sums"]) / ref["frame_bounds"]).max()
    offs = np.concatenate([[0], np.cumsum([S.F.frames_of(len(x), case[1]) for x in xs])])
    utt = np.array([frames[0][a:b].astype(np.float64).sum() for a, b in zip(offs[:-1], offs[1:])])
    use_u = (np.abs(utt - ref["utt_sums"]) / ref["utt_bounds"]).max()
    use_g = max(np.linalg.norm(a - b) / e for a, b, e in zip(grad, ref["grad"], ref["grad_bounds"]))
    msg = "float32 on the CPU, %r %s: worst share of the bound: frame sums %.3g, utterance sums %.3g, gradient %.3g" % (case, reduction, use_f, use_u, use_g)
    print(msg)
    assert use_f <= 1.0 and use_u <= 1.0 and use_g <= 1.0, msg


@pytest.mark.parametrize("reduction", REDUCTIONS)
@pytest.mark.parametrize("case", CASES, ids=str)
def test_every_mutant_leaves_its_bound(case, reduction):
    """(c) the bounds are not vacuous: each wrong rule's gradient lies outside the gradient bound of EVERY utterance, and the natural logarithm,
    which changes the forward pass, outside every utterance's sum bound too.  The symmetric Hann's distance from the periodic one falls with
    1 / win_length and a sum of log ratios hardly sees the window (x and y carry the same one): it is held against the gradient bound at
    win_length 240; its share of the sum bounds is printed."""
    xs, ys, ref = reference(case, reduction)
    w, hop, B = M.window(case), case[1], ref["B"]
    n_mels = len(B)
    excess = lambda grads: np.array([np.linalg.norm(a - b) / e for a, b, e in zip(grads, ref["grad"], ref["grad_bounds"])])
    g = lambda **kw: M.gradient(xs, ys, case, 1.0, reduction, B=B, **kw)
    muts = dict(natural_log=g(coef=ref["coef"], natural_log=True), n_as_frames=g(coef=M.coefficients(ref["n"], 1.0, reduction, n_as_frames=n_mels)),
                first_channel_only=g(coef=ref["coef"], first_channel_only=True), interior_bins_twice=g(coef=ref["coef"], double_interior=True),
                reflection_adjoint_dropped=g(coef=ref["coef"], no_reflection=True), window_omitted_in_backward=g(coef=ref["coef"], no_window=True))
    for name, got in muts.items():
        ex = excess(got)
        print("mutant %s, %r %s: %s gradient bounds" % (name, case, reduction, np.round(ex, 1)))
        if name == "n_as_frames" and n_mels == 1:
            continue
        assert ex.min() > 1.5, (name, ex)
    d_ln, _ = M.utt_sums(xs, ys, w, hop, B, log=np.log)
    ex = np.abs(d_ln - ref["utt_sums"]) / ref["utt_bounds"]
    print("mutant natural_log forward, %r: %s sum bounds" % (case, np.round(ex, 1)))
    assert ex.min() > 1.5
    if case in WIDE:
        wm = M.symmetric_window(case)
        d_s, _ = M.utt_sums(xs, ys, wm, hop, B)
        gs = [M.utt_gradient(x, y, wm, hop, B, c) for x, y, c in zip(xs, ys, ref["coef"])]
        ex_s, ex_g = np.abs(d_s - ref["utt_sums"]) / ref["utt_bounds"], excess(gs)
        print("mutant symmetric_hann, %r %s: %s sum bounds, %s gradient bounds" % (case, reduction, np.round(ex_s, 1), np.round(ex_g, 1)))
        assert ex_g.min() > 1.5, ex_g


def test_magnitude_floor_of_the_stft_loss_is_a_mutant_on_a_quiet_utterance():
    """m = sqrt(max(p, 1e-7)) in place of 1e-10: on a pair scaled down until most bins lie between the two floors, the utterance's sum leaves its
    bound (which needs no condition on the signs)"""
    case = M.SILENT_CASE
    xs, ys = M.quiet_signals(case)
    w, hop = M.window(case), case[1]
    ref = M.kernel_reference(case, xs, ys, "utterance")
    for v in (xs[1], ys[1]):
        X = S.spectrum(v, w, hop)
        p = X.real ** 2 + X.imag ** 2
        assert ((p > M.FLOOR) & (p < 1e-7)).mean() > 0.5
    d7, _ = M.utt_sums(xs, ys, w, hop, ref["B"], floor=1e-7)
    ex = np.abs(d7 - ref["utt_sums"]) / ref["utt_bounds"]
    print("mutant floor 1e-7 on the quiet utterance: %s sum bounds" % np.round(ex, 1))
    assert ex[1] > 1.5 and ex[0] < 1.0 and ex[2] < 1.0


def test_gradient_through_the_floor_is_a_mutant():
    """an utterance whose bins all lie below the floor without being zero: exactly zero is demanded, the bound is zero, and a gradient let through
    the magnitude floor is not zero; torch.clamp passes none either"""
    case = M.SILENT_CASE
    xs, ys = M.floored_signals(case)
    ref = M.kernel_reference(case, xs, ys, "utterance")
    assert ref["grad_bounds"][1] == 0.0 and not np.any(ref["grad"][1]) and (ref["grad_bounds"][[0, 2]] > 0).all()
    mut = M.gradient(xs, ys, case, 1.0, "utterance", B=ref["B"], coef=ref["coef"], through_floor=True)
    assert np.linalg.norm(mut[1]) > 0.0 and all(np.array_equal(mut[i], ref["grad"][i]) for i in (0, 2))
    _, grad = M.torch_statement(xs, ys, [case], "utterance", bases=[ref["B"]])
    assert not np.any(grad[1])
    zs, _ = M.signals(case, silent=True)
    zref = M.kernel_reference(case, zs, ys, "utterance")
    assert zref["grad_bounds"][1] == 0.0 and not np.any(zref["grad"][1])


# ---- (d) the filterbank's bin-major transpose -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["slaney_1024_80", "slaney_512_256", "hand"])
def test_banded_filterbank_transposes_and_comes_back(which):
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import features, griffinlim, mel_loss

    B = M.hand_basis() if which == "hand" else griffinlim.mel_filterbank(22050, int(which.split("_")[1]), int(which.split("_")[2]), 80.0, 7600.0)
    bins = B.shape[1]
    lo, off, w = features.banded_filterbank(B)
    bt_off, bt_ch, bt_w = mel_loss.bin_major_transpose(lo, off, w, bins)
    assert len(bt_off) == bins + 1 and bt_off[0] == 0 and bt_off[-1] == len(w) == len(bt_ch) == len(bt_w) == int((B != 0).sum())
    assert all(np.all(np.diff(bt_ch[a:b]) > 0) for a, b in zip(bt_off[:-1], bt_off[1:]))  # channels ascending within a bin
    assert np.array_equal(mel_loss.dense_from_transpose(bt_off, bt_ch, bt_w, len(B)), B)
    assert np.array_equal(features.dense_filterbank(lo, off, w, bins), B)
    if which == "hand":
        k = 45
        assert bt_ch[bt_off[k] : bt_off[k + 1]].tolist() == [0, 3, 4, 5] and not (bt_ch == 2).any()
        np.testing.assert_array_equal(np.asarray(M.filterbank((512, 50, 240, "hand"))), B)
    else:
        assert np.allclose(B, M.filterbank((int(which.split("_")[1]), 0, 0, int(which.split("_")[2]))), rtol=1e-9, atol=1e-15)  # the reference's own Slaney matrix


# ---- (e) the C ABI -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from fcl_taco2_amd import _lib

    return _lib.load()


def test_entry_points_validate_arguments_without_a_gpu(lib):
    from fcl_taco2_amd import _lib

    for fn in (lib.fcl_msl_sums_fwd, lib.fcl_msl_grad_bwd):
        assert fn(None, None) == -1 and b"null argument" in lib.fcl_last_error()
        a = _lib.MelLoss()
        a.frames, a.samples, a.n_fft, a.hop, a.n_utt, a.n_mels, a.nnz = 10, 1000, 768, 100, 2, 0, 0
        assert fn(C.byref(a), None) == -2 and b"n_fft must be 512, 1024 or 2048" in lib.fcl_last_error()
        a.n_fft, a.hop = 1024, 513
        assert fn(C.byref(a), None) == -2 and b"hop" in lib.fcl_last_error()
        a.hop = 0
        assert fn(C.byref(a), None) == -2 and b"hop" in lib.fcl_last_error()
        a.hop = 120
        assert fn(C.byref(a), None) == -2 and b"1 <= n_mels <= 256" in lib.fcl_last_error()
        a.n_mels = 257
        assert fn(C.byref(a), None) == -2 and b"1 <= n_mels <= 256" in lib.fcl_last_error()
        a.n_mels = 80
        assert fn(C.byref(a), None) == -2 and b"nnz" in lib.fcl_last_error()
        a.nnz, a.n_utt = 500, 11
        assert fn(C.byref(a), None) == -2 and b"frames >= n_utt" in lib.fcl_last_error()
        a.n_utt = 0
        assert fn(C.byref(a), None) == -2 and b"frames >= n_utt" in lib.fcl_last_error()
        a.n_utt, a.frames = 2, 1 << 21
        assert fn(C.byref(a), None) == -2 and b"2^31" in lib.fcl_last_error()
        a.frames, a.samples = 10, 1 << 31
        assert fn(C.byref(a), None) == -2 and b"samples" in lib.fcl_last_error()
        a.samples = 1000
        assert fn(C.byref(a), None) == -1 and b"null x" in lib.fcl_last_error()
        a.x = a.y = a.smp_off = a.frame_utt = a.utt_off = 256
        assert fn(C.byref(a), None) == -1 and b"null window" in lib.fcl_last_error()
        a.window, a.twiddle = 260, 256
        assert fn(C.byref(a), None) == -1 and b"null fb_lo" in lib.fcl_last_error()
        a.fb_lo = a.fb_off = a.fb_w = 256
        assert fn(C.byref(a), None) == -3 and b"8-byte aligned" in lib.fcl_last_error()
        a.window, a.twiddle = 256, 260
        assert fn(C.byref(a), None) == -3 and b"8-byte aligned" in lib.fcl_last_error()
        a.twiddle = 256
        assert fn(C.byref(a), None) == -1  # the entry's own buffers are missing
    assert b"null bt_off" in lib.fcl_last_error()
    a.bt_off = a.bt_ch = a.bt_w = 256
    assert lib.fcl_msl_grad_bwd(C.byref(a), None) == -1 and b"null coef" in lib.fcl_last_error()
    assert lib.fcl_msl_sums_fwd(C.byref(a), None) == -1 and b"null frame_sums" in lib.fcl_last_error()
    a.frame_sums, a.utt_sums = 256, 260
    assert lib.fcl_msl_sums_fwd(C.byref(a), None) == -3 and b"utt_sums" in lib.fcl_last_error()
    a.coef, a.gx, a.fr = 256, 256, 260
    assert lib.fcl_msl_grad_bwd(C.byref(a), None) == -3 and b"fr must be" in lib.fcl_last_error()


def test_plan_checks_its_configuration_before_any_device_call():
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, features, mel_loss

    with pytest.raises(_lib.FclError, match="GPU"):
        mel_loss.MelLossPlan("cpu")
    cfg = mel_loss.check_configuration(22050, [1024], [256], [None], 80, 80.0, 7600.0)
    assert (features.DEFAULTS["n_fft"], features.DEFAULTS["hop"], features.DEFAULTS["win_length"], features.DEFAULTS["n_mels"]) == (1024, 256, None, 80)
    assert [c[:3] for c in cfg] == [(1024, 256, 1024)] == [c[:3] for c in M.DEFAULT_RESOLUTIONS]  # win_length None: n_fft
    assert np.allclose(cfg[0][3], M.filterbank(M.DEFAULT_RESOLUTIONS[0]), rtol=1e-9, atol=1e-15)
    with pytest.raises(NotImplementedError, match="n_fft 768"):
        mel_loss.MelLossPlan("cuda:0", fft_sizes=[768], hop_sizes=[100], win_lengths=[600])
    with pytest.raises(NotImplementedError, match="hop 600"):
        mel_loss.MelLossPlan("cuda:0", fft_sizes=[1024], hop_sizes=[600], win_lengths=[600])
    with pytest.raises(NotImplementedError, match="win_length 2000"):
        mel_loss.MelLossPlan("cuda:0", fft_sizes=[1024], hop_sizes=[100], win_lengths=[2000])
    with pytest.raises(NotImplementedError, match="n_mels 257"):
        mel_loss.MelLossPlan("cuda:0", n_mels=257)
    with pytest.raises(ValueError, match="one length"):
        mel_loss.MelLossPlan("cuda:0", fft_sizes=[1024, 512], hop_sizes=[100], win_lengths=[600, 240])
    with pytest.raises(ValueError, match="resolutions"):
        mel_loss.MelLossPlan("cuda:0", fft_sizes=[512] * 9, hop_sizes=[50] * 9, win_lengths=[240] * 9)
    gap = M.hand_basis(513)
    gap[0, 20] = 0.0
    with pytest.raises(ValueError, match="row 0 is not a contiguous band"):
        mel_loss.MelLossPlan("cuda:0", mel_bases=[gap])
    with pytest.raises(ValueError, match="mel_basis 0 must be"):
        mel_loss.MelLossPlan("cuda:0", mel_bases=[M.hand_basis(257)])
    with pytest.raises(ValueError, match="mel bases for"):
        mel_loss.MelLossPlan("cuda:0", mel_bases=[None, None])


# ---- (f) the evaluation driver's flag --------------------------------------------------------------------------------------------------------------------
def test_evaluate_aligned_mel_flag(tmp_path):
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import evaluate as E

    d = str(tmp_path)
    base = ["--ref-wav-dir", d, "--syn-wav-dir", d]
    assert E.parse_args(base + ["--aligned", "--aligned-mel"]).aligned_mel
    assert not E.parse_args(base + ["--aligned"]).aligned_mel and not E.parse_args(base).aligned_mel
    with pytest.raises(SystemExit) as e:
        E.parse_args(base + ["--aligned-mel"])
    assert e.value.code == 2
    # without the flag the document and the line are what they were, byte for byte
    recs = [dict(id="a", ref_frames=3, syn_frames=4, path_len=5, mcd_db=1.5)]
    E.add_aligned(recs, np.array([[0.5, 0.3]]), np.array([[1.0, 3.0]]), [4000], [(512, 50, 240), (1024, 120, 600)])
    doc = E.summarise([dict(r) for r in recs], dict(order=13))
    assert sorted(doc) == ["mcd_db", "n_utt", "settings", "stft_log_mag", "stft_sc", "utterances"] and "mel_l1" not in doc["utterances"][0]
    line = E.summary_line(doc)
    assert line == "evaluate: 1 utterances, MCD 1.500 dB, STFT spectral convergence 0.4000, log-magnitude 2.0000"
    E.add_aligned_mel(recs, np.array([[0.25]]))
    doc = E.summarise(recs, dict(order=13))
    assert recs[0]["mel_l1"] == 0.25 and doc["mel_l1"] == 0.25 and E.summary_line(doc) == line + ", mel L1 0.2500"
