"""tests/evaluate_ref.py, the float64 statement of the evaluation contract, against facts that need no device: the DCT rows are
orthonormal, the folded de-normalisation, the vectorised recurrence against the plain loops, the cases whose arithmetic is exact in float32 (which
is why test_gpu_evaluate.py may demand bit-exact paths on them) and the error model of the float32 recurrence.  Then the C entries' error codes, the
ctypes mirror of fcl_ev_t, and the host side of the package and the driver."""
import ctypes as C
import json
import math
import subprocess

import numpy as np
import pytest

import evaluate_ref as E


# ---- the statement ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D", [(80, 13), (80, 40), (20, 1), (20, 19)])
def test_dct_rows_are_orthonormal(N, D):
    W = E.dct_rows(N, D)
    assert W.shape == (D, N) and np.abs(W @ W.T - np.eye(D)).max() <= 1e-12
    full = np.vstack([np.full((1, N), math.sqrt(1.0 / N)), E.dct_rows(N, N - 1)])  # with the c_0 row: the whole orthonormal basis
    assert np.abs(full @ full.T - np.eye(N)).max() <= 1e-12


def test_folded_statistics_equal_denormalising_first():
    rng = np.random.RandomState(0)
    N, D = 80, 13
    stats = np.stack([rng.uniform(-6.0, -1.0, N), rng.uniform(0.3, 2.0, N)])
    x = rng.randn(50, N)
    raw_t, raw_b = E.table_bias(N, D)
    t, b = E.table_bias(N, D, stats)
    assert not raw_b.any() and np.allclose(raw_t, math.log(10.0) * E.dct_rows(N, D), rtol=0, atol=0)
    want, _ = E.cepstra(x * (stats[1] + 1e-8) + stats[0], raw_t, raw_b)
    got, absum = E.cepstra(x, t, b)
    assert np.abs(got - want).max() <= 1e-12 and (absum > 0).all()


@pytest.mark.parametrize("size", [(1, 1), (1, 7), (7, 1), (2, 3), (23, 17), (40, 61)], ids=str)
def test_vectorised_recurrence_equals_the_double_loop(size):
    rng = np.random.RandomState(sum(size))
    for a, b in ((rng.randn(size[0], 5), rng.randn(size[1], 5)), (rng.randint(0, 3, (size[0], 1)), rng.randint(0, 3, (size[1], 1)))):
        for dt in (np.float64, np.float32):
            d = E.distances(a, b, dt)
            C1, bp1 = E.dp_loops(d)
            C2, bp2 = E.dp(d)
            assert C1.dtype == C2.dtype == dt and np.array_equal(C1, C2) and np.array_equal(bp1, bp2)
            path = E.backtrack(bp2)
            assert E.is_warping_path(path, *size) and E.path_cost(d, path) == C2[-1, -1]
    assert not E.is_warping_path(np.array([(0, 0), (1, 2)]), 2, 3) and not E.is_warping_path(np.array([(0, 0), (0, 0), (1, 1)]), 2, 2)


def test_exact_cases_are_exact_in_float32():
    """integer cepstra, D = 1: float32 and float64 give identical distances, costs and paths, all integers below 2^24; the all-ties paths by hand"""
    names = []
    for name, a, b in E.exact_cases():
        names.append(name)
        assert a.shape[1] == b.shape[1] == 1 and max(len(a), len(b)) <= 40 and max(np.abs(a).max(), np.abs(b).max()) <= 64
        d32, d64 = E.distances(a, b, np.float32), E.distances(a, b, np.float64)
        assert d32.dtype == np.float32 and np.array_equal(d32.astype(np.float64), d64) and np.array_equal(d64, np.rint(d64))
        C32, bp32 = E.dp(d32)
        C64, bp64 = E.dp(d64)
        assert np.array_equal(C32.astype(np.float64), C64) and np.array_equal(bp32, bp64) and C64.max() < 2 ** 24 and np.array_equal(C64, np.rint(C64))
        c32, p32 = E.dtw(a, b, np.float32)
        c64, p64 = E.dtw(a, b)
        assert float(c32) == c64 and np.array_equal(p32, p64) and E.is_warping_path(p64, len(a), len(b))
        if name.startswith(("same", "apart")):
            assert [tuple(v) for v in p64] == E.TIES[(len(a), len(b))], name
            assert c64 == (0.0 if name.startswith("same") else 3.0 * len(p64))
    assert sum(n.startswith(("same", "apart")) for n in names) == 6 and len(names) >= 12


@pytest.mark.parametrize("D", E.ORDERS)
@pytest.mark.parametrize("kind", E.KINDS)
def test_error_model_on_the_float32_reference(D, kind):
    """for the Gaussian inputs of the GPU test: the float32 recurrence's cost within gamma C64 of the float64 optimum, its own path valid, and that
    path's float64 cost within 2.1 gamma C64 above the optimum (the float32 DP is the minimum over paths of their float32 chain sums)"""
    worst = 0.0
    for size in E.SIZES:
        ref = E.reference(size, D, kind)
        g = E.gamma(size[0], size[1], D)
        c32, p32 = E.dtw(ref["a"], ref["b"], np.float32)
        assert E.is_warping_path(p32, *size) and E.is_warping_path(ref["path"], *size)
        assert ref["cost"] == E.path_cost(ref["d"], ref["path"])
        rel = abs(float(c32) - ref["cost"]) / ref["cost"] if ref["cost"] else 0.0
        worst = max(worst, rel / g)
        assert rel <= g, (size, rel, g)
        over = E.path_cost(ref["d"], p32) - ref["cost"]
        assert 0.0 <= over <= 2.1 * g * ref["cost"], (size, over)
    print("D %d, %s: worst share of gamma on the float32 reference %.3f" % (D, kind, worst))
    assert E.gamma(300, 511, 13) == pytest.approx(4.97e-5, rel=1e-2)


def test_figures_and_pitch_statement():
    assert E.mcd_db(3.0, 2) == pytest.approx(10.0 * math.sqrt(2.0) / math.log(10.0) * 1.5, rel=1e-15)
    assert E.cents([0.0, 1.0, 2.0, 440.0]) == pytest.approx([0.0, 0.0, 1200.0, 1200.0 * math.log2(440.0)], rel=1e-15)
    path = np.array([(0, 0), (1, 0), (2, 1), (2, 2)])
    vv, vuv, S = E.pitch_figures(path, [100.0, 0.0, 7.0], [90.0, 0.0, 4.0])
    assert (vv, vuv, S) == (2, 2, 100.0 + 9.0) and E.f0_rmse(S, vv) == pytest.approx(math.sqrt(54.5)) and math.isnan(E.f0_rmse(0.0, 0))


# ---- the package's host side --------------------------------------------------------------------------------------------------------------------
def test_the_package_builds_the_same_tables_and_refuses_what_the_kernels_do_not_cover():
    from fcl_taco2_amd import _lib, metrics as M

    assert (M.ORDER, M.ORDER_MAX, M.FRAMES_MAX) == (E.ORDER, E.ORDER_MAX, E.FRAMES_MAX) and M.MCD_SCALE == E.MCD_SCALE
    rng = np.random.RandomState(1)
    stats = np.stack([rng.uniform(-6.0, -1.0, 80), rng.uniform(0.3, 2.0, 80)])
    for N, D, st in ((80, 13, None), (80, 40, stats), (20, 1, None)):
        t, b = M.cepstra_table(N, D, st)
        t0, b0 = E.table_bias(N, D, st)
        assert np.abs(t - t0).max() <= 1e-14 and np.abs(b - b0).max() <= 1e-12
    for N, D in ((80, 0), (80, 41), (20, 20)):
        with pytest.raises(ValueError, match="--order"):
            M.check_order(N, D)
    with pytest.raises(NotImplementedError, match="--n-mels"):
        M.check_order(257, 13)
    with pytest.raises(ValueError, match=r"mel_stats must be \[2, 80\]"):
        M.cepstra_table(80, 13, np.zeros((2, 40)))
    with pytest.raises(_lib.FclError, match="GPU"):
        M.CepstraPlan("cpu", 80)
    with pytest.raises(_lib.FclError, match="GPU"):
        M.Evaluator("cpu")
    with pytest.raises(ValueError, match="utterance long1 has 4097 reference and 10 synthesised frames"):
        M.check_pairs([5, 4097], [7, 10], ["ok", "long1"])
    with pytest.raises(ValueError, match="utterance #0 has 3 reference and 0 synthesised"):
        M.check_pairs([3], [0])
    M.check_pairs([4096, 1], [1, 4096])
    with pytest.raises(ValueError, match="utterance ub: the synthesised F0 track has 4 frames, its mel has 5"):
        M._track([np.zeros(3), np.zeros(4)], [3, 5], "cpu", ["ua", "ub"], "synthesised")
    assert M.pair_batches([10, 10, 10, 50, 1], [10, 10, 10, 50, 1], 250) == [[0, 1], [2], [3], [4]]
    f = M.figures([3.0, 0.0], [2, 4], [[2, 1], [0, 0]], [109.0, 0.0])
    assert f["mcd_db"][0] == E.mcd_db(3.0, 2) and f["f0_rmse_cents"][0] == pytest.approx(math.sqrt(54.5)) and math.isnan(f["f0_rmse_cents"][1])
    assert list(f["vuv_error"]) == [0.5, 0.0] and list(f["n_vv"]) == [2, 0]


def test_ctypes_mirror_of_the_argument_struct_matches_the_header(tmp_path):
    from conftest import ROOT
    from fcl_taco2_amd import _lib

    names = [n for n, _ in _lib.Evaluate._fields_]
    body = ['#include <stdio.h>', '#include <stddef.h>', '#include "fcl_hip.h"', "int main(void) {", '  printf("%zu", sizeof(fcl_ev_t));']
    body += ['  printf(" %%zu", offsetof(fcl_ev_t, %s));' % n for n in names] + ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(body))
    subprocess.run(["gcc", "-I", "%s/include" % ROOT, str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(_lib.Evaluate)] + [getattr(_lib.Evaluate, n).offset for n in names] and len(names) == 23


def test_entry_points_validate_arguments_without_a_gpu():
    """every fcl_ev_* entry returns before any HIP call: -1 for a null pointer, -2 for D, a length or a count out of range, -5 for a workspace that is
    too small, 0 for an empty batch"""
    from fcl_taco2_amd import _lib

    lib = _lib.load()
    assert lib.fcl_ev_dtw_workspace_bytes(0, 0) == 0 and lib.fcl_ev_dtw_workspace_bytes(-3, 1) == 0
    assert lib.fcl_ev_dtw_workspace_bytes(1000, 3) >= 1000 and lib.fcl_ev_dtw_workspace_bytes(1 << 33, 600) >= 1 << 33
    # cepstra
    assert lib.fcl_ev_cepstra_fwd(None, None, None, None, 10, 80, 13, None) == -1 and b"null" in lib.fcl_last_error()
    for frames, N, D in ((10, 80, 0), (10, 80, 41), (10, 20, 20), (10, 257, 13), (10, 1, 1), (-1, 80, 13), (1 << 31, 80, 13)):
        assert lib.fcl_ev_cepstra_fwd(256, 256, 256, 256, frames, N, D, None) == -2, (frames, N, D)
    assert lib.fcl_ev_cepstra_fwd(None, None, None, None, 0, 80, 13, None) == 0
    # dtw and pitch
    for fn in (lib.fcl_ev_dtw_fwd, lib.fcl_ev_path_pitch_fwd):
        assert fn(None, None) == -1
        a = _lib.Evaluate()
        a.frames_a, a.frames_b, a.cells, a.path_rows, a.n_pairs, a.d, a.max_ta, a.max_tb = 10, 12, 120, 21, 1, 13, 10, 12
        assert fn(C.byref(a), None) == -1 and b"null" in lib.fcl_last_error()
        for f, _ in _lib.Evaluate._fields_[8:]:
            if f != "workspace_bytes":
                setattr(a, f, 256)
        a.workspace_bytes = lib.fcl_ev_dtw_workspace_bytes(120, 1)
        for field, bad in (("d", 0), ("d", 41), ("n_pairs", -1), ("n_pairs", 65536), ("max_ta", 0), ("max_ta", 4097), ("max_tb", 4097), ("max_tb", 0),
                           ("frames_a", 0), ("frames_b", -1), ("frames_a", 1 << 31), ("cells", 0), ("path_rows", 0)):
            good = getattr(a, field)
            setattr(a, field, bad)
            assert fn(C.byref(a), None) == -2, field
            setattr(a, field, good)
        for f in (("a", "cost", "workspace", "a_off", "path_len") if fn is lib.fcl_ev_dtw_fwd else ("pitch_a", "counts", "sums", "path", "path_off")):
            setattr(a, f, None)
            assert fn(C.byref(a), None) == -1, f
            setattr(a, f, 256)
        if fn is lib.fcl_ev_dtw_fwd:
            a.workspace_bytes = 119
            assert fn(C.byref(a), None) == -5 and b"workspace" in lib.fcl_last_error()
            a.workspace_bytes = lib.fcl_ev_dtw_workspace_bytes(120, 1)
        a.n_pairs = 0
        for f, _ in _lib.Evaluate._fields_[8:]:
            if f != "workspace_bytes":
                setattr(a, f, None)
        assert fn(C.byref(a), None) == 0


# ---- the driver's host side ---------------------------------------------------------------------------------------------------------------------
def _tree(tmp_path):
    ref, syn = tmp_path / "ref", tmp_path / "syn"
    ref.mkdir()
    syn.mkdir()
    for u, t in (("ua", 5), ("ub", 9)):
        np.save(ref / (u + ".npy"), np.zeros((t, 80), np.float32))
        np.save(syn / (u + ".npy"), np.zeros((t + 2, 80), np.float32))
    return ref, syn


def test_driver_pairs_by_id_and_refuses_before_any_device_call(tmp_path):
    from fcl_taco2_amd import evaluate as V

    ref, syn = _tree(tmp_path)
    a, b = V.read_source(mel_dir=str(ref)), V.read_source(mel_dir=str(syn))
    assert V.pair_ids(a, b) == ["ua", "ub"] and V.frame_counts(b, ["ua", "ub"], 22050, 256, 80, False) == ([7, 11], None)
    np.save(syn / "uc.npy", np.zeros((4, 80), np.float32))
    with pytest.raises(ValueError, match=r"0 only in .*ref \(first: -\), 1 only in .*syn \(first: uc\)"):
        V.pair_ids(a, V.read_source(mel_dir=str(syn)))
    with pytest.raises(ValueError, match="first: uc"):  # the driver itself, on a device that does not exist: refused before it is touched
        V.main(["--ref-mel-dir", str(ref), "--syn-mel-dir", str(syn), "--device", "cuda:99"])
    (syn / "uc.npy").unlink()
    np.save(syn / "ub.npy", np.zeros((4097, 80), np.float32))
    with pytest.raises(ValueError, match="utterance ub has 9 reference and 4097 synthesised frames"):
        V.main(["--ref-mel-dir", str(ref), "--syn-mel-dir", str(syn), "--device", "cuda:99"])
    np.save(syn / "ub.npy", np.zeros((11, 40), np.float32))
    with pytest.raises(ValueError, match="utterance ub: .*mismatched n_mels"):
        V.main(["--ref-mel-dir", str(ref), "--syn-mel-dir", str(syn), "--device", "cuda:99"])
    # wav names: <utt>.wav and <utt>_gen.wav give the same id; an scp's shapes come from the headers
    import wave

    from fcl_taco2_amd import kaldi_io

    wd = tmp_path / "w"
    wd.mkdir()
    for n, rate in (("ua.wav", 22050), ("ub_gen.wav", 16000)):
        with wave.open(str(wd / n), "wb") as f:
            f.setnchannels(1), f.setsampwidth(2), f.setframerate(rate), f.writeframes(np.zeros(3200, "<i2").tobytes())
    w = V.read_source(wav_dir=str(wd))
    assert sorted(w.items) == ["ua", "ub"] and w.kind == "wav"
    with pytest.raises(ValueError, match="ub_gen.wav: sampling rate 16000, --fs is 22050"):
        V.frame_counts(w, ["ua", "ub"], 22050, 256, 80, False)
    assert V.frame_counts(w, ["ua", "ub"], 22050, 256, 80, True) == ([3200 // 256 + 1, (3200 * 441 // 320) // 256 + 1], [22050, 16000])
    with kaldi_io.ArkScpWriter(str(tmp_path / "f")) as wr:
        wr["ua"] = np.ones((6, 80), np.float32)
        wr["ub"] = np.ones((3, 80), np.float32)
    s = V.read_source(feats_scp=str(tmp_path / "f.scp"))
    assert [s.mel_shape(u) for u in ("ua", "ub")] == [(6, 80), (3, 80)] and s.mel("ub").shape == (3, 80)


def test_driver_flag_errors(tmp_path, capsys):
    from fcl_taco2_amd import evaluate as V

    ref, syn = _tree(tmp_path)
    np.save(tmp_path / "st.npy", np.ones((2, 80)))
    base = ["--ref-mel-dir", str(ref), "--syn-mel-dir", str(syn)]
    for extra, msg in ((["--mel-stats", str(tmp_path / "st.npy")], "which side"), (["--syn-normalised"], "needs --mel-stats"), (["--order", "41"], "--order"),
                       (["--batch-cells", "0"], "--batch-cells"), (["--ref-feats-scp", "x"], "not allowed with")):
        with pytest.raises(SystemExit):
            V.parse_args(base + extra)
        assert msg in capsys.readouterr().err
    args = V.parse_args(base + ["--mel-stats", str(tmp_path / "st.npy"), "--syn-normalised"])
    assert args.syn_normalised and not args.ref_normalised and args.order == 13 and args.batch_cells == 16 << 20


def test_json_layout_from_hand_made_records():
    from fcl_taco2_amd import evaluate as V

    res = dict(path_len=np.array([10, 20, 8]), mcd_db=np.array([4.0, 6.0, 8.0]), f0_rmse_cents=np.array([30.0, float("nan"), 50.0]),
               vuv_error=np.array([0.1, 0.5, 0.3]), n_vv=np.array([7, 0, 5]))
    recs = V.records_of(["a", "b", "c"], [9, 15, 8], [10, 20, 6], res)
    doc = V.summarise(recs, dict(order=13))
    assert list(doc) == ["n_utt", "mcd_db", "vuv_error", "f0_rmse_cents", "n_utt_voiced", "settings", "utterances"]
    assert doc["n_utt"] == 3 and doc["mcd_db"] == 6.0 and doc["vuv_error"] == pytest.approx(0.3) and doc["f0_rmse_cents"] == 40.0 and doc["n_utt_voiced"] == 2
    assert doc["utterances"][1] == dict(id="b", ref_frames=15, syn_frames=20, path_len=20, mcd_db=6.0, f0_rmse_cents=None, vuv_error=0.5, n_vv=0)
    assert json.loads(json.dumps(doc)) == doc and "F0 RMSE 40.0 cents over 2 utterances" in V.summary_line(doc)
    mel_only = V.summarise(V.records_of(["a"], [9], [10], dict(path_len=np.array([10]), mcd_db=np.array([4.0]))), {})
    assert list(mel_only) == ["n_utt", "mcd_db", "settings", "utterances"] and list(mel_only["utterances"][0]) == ["id", "ref_frames", "syn_frames", "path_len", "mcd_db"]
    assert V.summary_line(mel_only) == "evaluate: 1 utterances, MCD 4.000 dB"
