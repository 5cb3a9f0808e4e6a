"""The float64 statement of the multi-resolution STFT loss (tests/stft_loss_ref.py) without a GPU: it agrees with torch.stft + autograd,
the inputs of tests/test_gpu_stft_loss.py meet the conditions their bounds assume, a float32 evaluation stays inside every bound and every mutant
leaves its bound; then the C ABI's argument checks and the evaluation driver's flags."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import stft_loss_ref as S

CASES = list(S.CASES)
REDUCTIONS = ("utterance", "batch")


@functools.lru_cache(maxsize=None)
def reference(case, reduction):
    xs, ys = S.signals(case)
    return xs, ys, S.kernel_reference(case, xs, ys, reduction)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b))


@pytest.mark.parametrize("case", CASES, ids=str)
def test_inputs_meet_the_conditions_of_the_bounds(case):
    """every bin of x and y: p >= 4e-7, neither the clamp nor the sign of log m_y - log m_x can flip within the frame's magnitude bound -- for 100 % of
    the bins, in float64 alone; the silent utterance is digital silence and its neighbours are the case's own"""
    xs, ys = S.signals(case)
    assert [len(x) for x in xs] == S.CASES[case] and all(np.abs(x).max() > 0.1 for x in xs)
    assert S.conditions(case, xs, ys) == 1.0
    if case == S.SILENT_CASE:
        zs, _ = S.signals(case, silent=True)
        assert not np.any(zs[1]) and S.all_clamped(zs[1], S.window(case), case[1]) and all(np.array_equal(zs[i], xs[i]) for i in (0, 2))
        qs, _ = S.quiet_signals(case)
        assert np.all(qs[1] != 0) and S.all_clamped(qs[1], S.window(case), case[1])
    _, _, ref = reference(case, "utterance")
    print("stft loss %r: gradient bound / gradient norm per utterance %s" % (case, np.round(ref["grad_bounds"] / [np.linalg.norm(g) for g in ref["grad"]], 4)))


def test_default_resolution_inputs_meet_the_conditions():
    for xs, ys in (S.module_signals(), S.ragged_signals()):
        assert all(S.conditions(c, xs, ys) == 1.0 for c in S.DEFAULT_RESOLUTIONS)
    xs, _ = S.module_signals()
    assert [len(x) for x in xs] == [S.MODULE_T] * S.MODULE_B


@pytest.mark.parametrize("reduction", REDUCTIONS)
@pytest.mark.parametrize("case", CASES + ["silent"], ids=str)
def test_numpy_statement_equals_torch_stft_autograd_in_float64(case, reduction):
    """(a) loss and gradient to 1e-10 relative, upstream gradients other than 1; the silent utterance's gradient is exactly zero in both"""
    silent = case == "silent"
    case = S.SILENT_CASE if silent else case
    xs, ys = S.signals(case, silent=silent)
    sc, mag, grad = S.torch_statement(xs, ys, [case], reduction, 2.0, 0.5)
    nsc, nmag = S.loss(xs, ys, [case], reduction)
    ngrad = S.gradient(xs, ys, case, 2.0, 0.5, reduction)
    assert abs(sc - nsc) <= 1e-10 * sc and abs(mag - nmag) <= 1e-10 * mag
    for u, (a, b) in enumerate(zip(ngrad, grad)):
        if silent and u == 1:
            assert not np.any(a) and not np.any(b)
        else:
            assert rel(a, b) <= 1e-10, (u, rel(a, b))


def test_numpy_statement_equals_torch_on_the_default_resolutions():
    for (xs, ys), reduction in ((S.module_signals(), "batch"), (S.ragged_signals(), "utterance")):
        sc, mag, grad = S.torch_statement(xs, ys, S.DEFAULT_RESOLUTIONS, reduction)
        ref = S.module_reference(xs, ys, S.DEFAULT_RESOLUTIONS, reduction)
        assert abs(sc - ref["sc"]) <= 1e-10 * sc and abs(mag - ref["mag"]) <= 1e-10 * mag
        assert all(rel(a, b) <= 1e-10 for a, b in zip(ref["grad"], grad))
        total = S.total_gradient(xs, ys, S.DEFAULT_RESOLUTIONS, 1.0, 1.0, reduction)
        assert all(rel(a, b) <= 1e-12 for a, b in zip(total, ref["grad"]))


@pytest.mark.parametrize("reduction", REDUCTIONS)
@pytest.mark.parametrize("case", CASES, ids=str)
def test_float32_evaluation_stays_inside_every_bound(case, reduction):
    """(b) torch.stft + autograd in float32 on the CPU: frame sums, utterance sums and gradient within the derived bounds -- they are reachable"""
    xs, ys, ref = reference(case, reduction)
    _, _, grad, frames = S.torch_statement(xs, ys, [case], reduction, *S.UPSTREAM, dtype=torch.float32, detail=True)
    use_f = (np.abs(frames[0] - ref["frame_sums"]) / ref["frame_bounds"]).max()
    offs = np.concatenate([[0], np.cumsum([S.F.frames_of(len(x), case[1]) for x in xs])])
    utt = np.stack([frames[0][a:b].astype(np.float64).sum(0) for a, b in zip(offs[:-1], offs[1:])])
    use_u = (np.abs(utt - ref["utt_sums"]) / ref["utt_bounds"]).max()
    use_g = max(np.linalg.norm(a - b) / e for a, b, e in zip(grad, ref["grad"], ref["grad_bounds"]))
    msg = "float32 on the CPU, %r %s: worst share of the bound: frame sums %.3g, utterance sums %.3g, gradient %.3g" % (case, reduction, use_f, use_u, use_g)
    print(msg)
    assert use_f <= 1.0 and use_u <= 1.0 and use_g <= 1.0, msg


def mutant_gradients(case, xs, ys, reduction):
    """name -> per-utterance gradient of each wrong rule (the window mutants: the wrong window forward and backward)"""
    w, hop = S.window(case), case[1]
    s, n = S.utt_sums(xs, ys, w, hop)
    g = lambda **kw: S.gradient(xs, ys, case, *S.UPSTREAM, reduction, **kw)
    out = dict(interior_bins_twice=g(double_interior=True), reflection_adjoint_dropped=g(no_reflection=True), window_omitted_in_backward=g(no_window=True),
               n_as_frames=g(coef=S.coefficients(s, n, *S.UPSTREAM, reduction, n_as_frames=case[0] // 2 + 1)))
    if reduction == "batch":
        out["utterance_ab_under_batch"] = g(coef=S.coefficients(s, n, *S.UPSTREAM, reduction, utt_ab=True))
    for name, wm in (("window_left_aligned", S.left_aligned_window(case)), ("symmetric_hann", S.symmetric_window(case))):
        sm = np.stack([S.frame_sums(x, y, wm, hop).sum(0) for x, y in zip(xs, ys)])
        out[name] = ([S.utt_gradient(x, y, wm, hop, c[0], c[1]) for x, y, c in zip(xs, ys, S.coefficients(sm, n, *S.UPSTREAM, reduction))], sm)
    return out


@pytest.mark.parametrize("reduction", REDUCTIONS)
@pytest.mark.parametrize("case", CASES, ids=str)
def test_every_mutant_leaves_its_bound(case, reduction):
    """(c) the bounds are not vacuous.  Gradient mutants against the gradient bound of EVERY utterance; the per-utterance A, B under "batch" against
    at least one (an utterance whose own A B lies next to the batch's moves little); the two window mutants change the forward pass, so they are
    held against the utterance sums' bounds in every case (left-aligned: where win_length < n_fft, elsewhere it is the same window), and the
    symmetric Hann, whose distance from the periodic one falls with 1 / win_length, against the gradient bound at win_length 240."""
    xs, ys, ref = reference(case, reduction)
    excess = lambda grads: np.array([np.linalg.norm(a - b) / e for a, b, e in zip(grads, ref["grad"], ref["grad_bounds"])])
    for name, got in mutant_gradients(case, xs, ys, reduction).items():
        if isinstance(got, tuple):
            if name == "window_left_aligned" and case[2] == case[0]:
                assert np.array_equal(S.left_aligned_window(case), S.window(case))
                continue
            grads, sums = got
            ex_s = (np.abs(sums - ref["utt_sums"]) / ref["utt_bounds"]).max(1)  # the most affected of A, B, C, per utterance (C, a sum of log ratios, hardly sees the window)
            print("mutant %s, %r %s: utterance sums %s, gradient %s bounds" % (name, case, reduction, np.round(ex_s, 1), np.round(excess(grads), 2)))
            assert (ex_s > 2.0).all(), (name, ex_s)
            if name == "window_left_aligned" or case[2] == 240:
                assert (excess(grads) > 2.0).all(), (name, excess(grads))
            continue
        ex = excess(got)
        print("mutant %s, %r %s: %s gradient bounds" % (name, case, reduction, np.round(ex, 2)))
        assert (ex.max() if name == "utterance_ab_under_batch" else ex.min()) > 1.5, (name, ex)


def test_gradient_through_the_clamp_is_a_mutant():
    """an utterance whose bins all lie below the clamp without being zero: the gradient is exactly zero and its bound is zero; passing a gradient
    through the clamp gives one that is not"""
    case = S.SILENT_CASE
    xs, ys = S.quiet_signals(case)
    ref = S.kernel_reference(case, xs, ys, "utterance")
    assert ref["grad_bounds"][1] == 0.0 and not np.any(ref["grad"][1]) and (ref["grad_bounds"][[0, 2]] > 0).all()
    mut = S.gradient(xs, ys, case, *S.UPSTREAM, "utterance", coef=ref["coef"], through_clamp=True)
    assert np.linalg.norm(mut[1]) > 0.0 and all(np.array_equal(mut[i], ref["grad"][i]) for i in (0, 2))
    _, _, grad = S.torch_statement(xs, ys, [case], "utterance", *S.UPSTREAM)
    assert not np.any(grad[1])  # torch.clamp passes none either


# ---- (d) the C ABI -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from fcl_taco2_amd import _lib

    return _lib.load()


def test_entry_points_validate_arguments_without_a_gpu(lib):
    from fcl_taco2_amd import _lib

    for fn in (lib.fcl_stl_sums_fwd, lib.fcl_stl_grad_bwd):
        assert fn(None, None) == -1 and b"null argument" in lib.fcl_last_error()
        a = _lib.StftLoss()
        a.frames, a.samples, a.n_fft, a.hop, a.n_utt = 10, 1000, 768, 100, 2
        assert fn(C.byref(a), None) == -2 and b"n_fft must be 512, 1024 or 2048" in lib.fcl_last_error()
        a.n_fft, a.hop = 1024, 513
        assert fn(C.byref(a), None) == -2 and b"hop" in lib.fcl_last_error()
        a.hop, a.n_utt = 120, 11
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
        assert fn(C.byref(a), None) == -3 and b"8-byte aligned" in lib.fcl_last_error()
        a.window = 256
        assert fn(C.byref(a), None) == -1  # the entry's own buffers are missing
    assert b"frame_sums" in lib.fcl_last_error() or b"coef" in lib.fcl_last_error()
    a.frame_sums, a.utt_sums = 256, 260
    assert lib.fcl_stl_sums_fwd(C.byref(a), None) == -3 and b"utt_sums" in lib.fcl_last_error()
    a.coef, a.gx, a.fr = 256, 256, 260
    assert lib.fcl_stl_grad_bwd(C.byref(a), None) == -3 and b"fr must be" in lib.fcl_last_error()


def test_plan_checks_its_configuration_before_any_device_call():
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, stft_loss

    assert (stft_loss.FFT_SIZES, stft_loss.HOP_SIZES, stft_loss.WIN_LENGTHS) == tuple(zip(*S.DEFAULT_RESOLUTIONS))
    with pytest.raises(_lib.FclError, match="GPU"):
        stft_loss.STFTLossPlan("cpu")
    with pytest.raises(NotImplementedError, match="n_fft 768"):
        stft_loss.STFTLossPlan("cuda:0", [768], [100], [600])
    with pytest.raises(NotImplementedError, match="hop 600"):
        stft_loss.STFTLossPlan("cuda:0", [1024], [600], [600])
    with pytest.raises(NotImplementedError, match="win_length 2000"):
        stft_loss.STFTLossPlan("cuda:0", [1024], [100], [2000])
    with pytest.raises(ValueError, match="one length"):
        stft_loss.STFTLossPlan("cuda:0", [1024, 512], [100], [600, 240])
    with pytest.raises(ValueError, match="resolutions"):
        stft_loss.STFTLossPlan("cuda:0", [512] * 9, [50] * 9, [240] * 9)


# ---- (e) the evaluation driver's flags -----------------------------------------------------------------------------------------------------------------
def test_evaluate_aligned_flags(tmp_path):
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import evaluate as E

    d = str(tmp_path)
    args = E.parse_args(["--ref-wav-dir", d, "--syn-wav-dir", d, "--aligned"])
    assert args.aligned and args.aligned_max_diff == 2 * args.hop
    assert list(zip(args.stft_fft_sizes, args.stft_hops, args.stft_win_lengths)) == S.DEFAULT_RESOLUTIONS
    args = E.parse_args(["--ref-wav-dir", d, "--syn-wav-dir", d, "--aligned", "--stft-fft-sizes", "512,1024", "--stft-hops", "50,120", "--stft-win-lengths",
                         "240,600", "--aligned-max-diff", "7"])
    assert (args.stft_fft_sizes, args.stft_hops, args.stft_win_lengths, args.aligned_max_diff) == ([512, 1024], [50, 120], [240, 600], 7)
    assert not E.parse_args(["--ref-wav-dir", d, "--syn-wav-dir", d]).aligned
    for bad in (["--ref-mel-dir", d, "--syn-wav-dir", d, "--aligned"], ["--ref-wav-dir", d, "--syn-mel-dir", d, "--aligned"],
                ["--ref-wav-dir", d, "--syn-wav-dir", d, "--aligned", "--stft-hops", "120,240"],
                ["--ref-wav-dir", d, "--syn-wav-dir", d, "--aligned", "--stft-fft-sizes", "1000,2048,512"],
                ["--ref-wav-dir", d, "--syn-wav-dir", d, "--aligned", "--aligned-max-diff", "-1"]):
        with pytest.raises(SystemExit) as e:
            E.parse_args(bad)
        assert e.value.code == 2, bad


def test_evaluate_aligned_refusals_name_the_utterance():
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import evaluate as E

    assert E.check_aligned(["a", "b"], [5000, 4100], [5100, 4000], 512, 2048) == [5000, 4000]
    with pytest.raises(ValueError, match="utterance b has 4100 reference and 4700 synthesised samples"):
        E.check_aligned(["a", "b"], [5000, 4100], [5100, 4700], 512, 2048)
    with pytest.raises(ValueError, match="utterance b has 1000 samples"):
        E.check_aligned(["a", "b"], [5000, 1000], [5100, 1100], 512, 2048)
    assert E.sample_batches([10, 20, 30, 100, 5], 60) == [[0, 1, 2], [3], [4]]
    # the document and the line without --aligned carry none of the new keys
    recs = [dict(id="a", ref_frames=3, syn_frames=4, path_len=5, mcd_db=1.5)]
    doc = E.summarise([dict(r) for r in recs], dict(order=13))
    assert sorted(doc) == ["mcd_db", "n_utt", "settings", "utterances"] and "STFT" not in E.summary_line(doc)
    E.add_aligned(recs, np.array([[0.5, 0.3]]), np.array([[1.0, 3.0]]), [4000], [(512, 50, 240), (1024, 120, 600)])
    doc = E.summarise(recs, dict(order=13))
    assert doc["stft_sc"] == pytest.approx(0.4) and doc["stft_log_mag"] == pytest.approx(2.0) and recs[0]["aligned_samples"] == 4000
    assert recs[0]["stft"][1] == dict(n_fft=1024, hop=120, win_length=600, sc=pytest.approx(0.3), log_mag=pytest.approx(3.0))
    assert "STFT spectral convergence 0.4000, log-magnitude 2.0000" in E.summary_line(doc)
