"""The three kernels of csrc/align.hip, alignment.Aligner and the align driver against the float64 numpy statement of tests/align_ref.py (DESIGN.md
6i).  Every buffer a kernel writes, the workspace included, sits between guard zones filled with a NaN bit pattern, which must survive; every test
reads the library's launch record and fails if its kernel did not run.  The statement itself and the exactness of the exact cases are checked in
test_align_cpu.py."""
import contextlib
import functools
import json
import wave

import numpy as np
import pytest
import torch

import align_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAT32 = 0x7FC12345  # an fp32 NaN (and the halves of an fp64 NaN): whatever is read from an unwritten word poisons the result
U = 2.0 ** -24
LOGLIK, VITERBI, STATS = "al_loglik_kernel", "al_viterbi_kernel", "al_stats_kernel"
MCOL = 1024  # the columns of every ll matrix of the Viterbi cases: one batch takes them all; the columns past a case's states hold NaN


@pytest.fixture(scope="module")
def A():
    assert torch.cuda.is_available()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, alignment

    _lib.load()
    return alignment


@contextlib.contextmanager
def launched(*names, absent=()):
    """the launches inside run the named kernels and none of `absent` (the library's own launch record)"""
    from fcl_taco2_amd import _lib

    _lib.prof_enable(True)
    try:
        yield
        torch.cuda.synchronize()
        seen = set(_lib.prof_collect())
    finally:
        _lib.prof_enable(False)
    for n in names:
        assert n in seen, (n, sorted(seen))
    for n in absent:
        assert n not in seen, (n, sorted(seen))


class Guarded(object):
    """a device buffer of n elements between two guard zones; everything starts as the NaN pattern"""

    PAD = 8192

    def __init__(self, n, dtype=torch.float32):
        self.n, self.dtype = int(n), dtype
        self.words = self.n * torch.empty(0, dtype=dtype).element_size() // 4
        self.buf = torch.empty(self.words + 2 * self.PAD, dtype=torch.int32, device=DEV)
        self.buf.fill_(PAT32)

    @property
    def t(self):
        return self.buf[self.PAD : self.PAD + self.words].view(self.dtype)

    def set(self, a):
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(a)).reshape(-1).to(self.dtype))
        return self

    def np(self):
        return self.t.cpu().numpy()

    def intact(self):
        return bool((self.buf[: self.PAD] == PAT32).all()) and bool((self.buf[self.PAD + self.words :] == PAT32).all())


# ---- log-likelihood -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 13, 28, 40])
def test_loglik_vs_float64(A, D):
    """M = 1, 24, 210, 1024 (below a tile of 64 states, tiles with a partial last one, 16 tiles) x 1, 2, 63, 64, 65, 300 frames (below, at and above
    a workgroup's 16, a partial last workgroup): every value within align_ref.loglik_bound of float64 on the float32-rounded parameters"""
    rng = np.random.RandomState(D)
    worst = 0.0
    for M in (1, 24, 210, 1024):
        mean32, ivar32, g32 = R.params32(rng.randn(M, D) * 2.0, rng.uniform(0.2, 3.0, (M, D)))
        params = tuple(Guarded(a.size).set(a) for a in (mean32, ivar32, g32))
        views = (params[0].t.view(M, D), params[1].t.view(M, D), params[2].t)
        for frames in (1, 2, 63, 64, 65, 300):
            x = (rng.randn(frames, D) * 2.5).astype(np.float32)
            xg, lg = Guarded(frames * D).set(x), Guarded(frames * M)
            with launched(LOGLIK):
                A.launch_loglik(views, xg.t, lg.t, frames)
            assert xg.intact() and lg.intact() and all(p.intact() for p in params)
            got = lg.np().astype(np.float64).reshape(frames, M)
            want, q = R.loglik(x, mean32, ivar32, g32)
            share = np.abs(got - want) / R.loglik_bound(q, want, D)
            assert np.isfinite(got).all() and share.max() <= 1.0, (M, frames, float(share.max()))
            worst = max(worst, float(share.max()))
    print("loglik D %d: worst share of the bound %.3f" % (D, worst))


# ---- Viterbi --------------------------------------------------------------------------------------------------------------------------------------------
def padded(ll):
    out = np.full((ll.shape[0], MCOL), np.nan, dtype=np.float32)
    out[:, : ll.shape[1]] = ll
    return out


def guarded_launch(mp, cases, n_states, workspace_bytes, launch, tables=()):
    """the tail run_viterbi and test_gpu_align_lattice.run_lattice share: ll, the workspace and the outputs of ONE launch over the maps mp on guarded
    buffers, launch(ll, ws, frame_row, row_begin, row_frames, score, ok) on their views, every guard zone (and those of `tables`) intact -> per case
    dict(ok, score as float32, frame_row, row_begin, row_frames, frame0) with row_begin relative to the batch"""
    ll = Guarded(mp.frames * n_states).set(np.concatenate([c[0] for c in cases]))
    nws = mp.workspace_bytes() if workspace_bytes is None else workspace_bytes
    assert nws % 4 == 0 and (workspace_bytes is not None or nws >= mp.cells)
    ws = Guarded(nws, torch.uint8)
    frame_row, row_begin, row_frames = Guarded(mp.frames, torch.int32), Guarded(mp.rows, torch.int32), Guarded(mp.rows, torch.int32)
    score, ok = Guarded(mp.n_utt), Guarded(mp.n_utt, torch.int32)
    launch(ll.t, ws.t, frame_row.t, row_begin.t, row_frames.t, score.t, ok.t)
    assert all(g.intact() for g in (ll, ws, frame_row, row_begin, row_frames, score, ok) + tuple(tables))
    fr, rb, rf, sc, okh = frame_row.np(), row_begin.np(), row_frames.np(), score.np(), ok.np()
    out = []
    for k in range(mp.n_utt):
        f, r = slice(mp.frame_offs[k], mp.frame_offs[k + 1]), slice(mp.row_offs[k], mp.row_offs[k + 1])
        out.append(dict(ok=int(okh[k]), score=sc[k], frame_row=fr[f].astype(np.int64), row_begin=rb[r].astype(np.int64), row_frames=rf[r].astype(np.int64),
                        frame0=int(mp.frame_offs[k])))
    return out


def run_viterbi(A, cases, workspace_bytes=None, n_states=MCOL, tamper=None):
    """ONE al_viterbi_kernel launch over cases [(ll float32 [T][n_states], row_state, row_skip)] on guarded buffers -> guarded_launch's dicts;
    tamper(mp) may replace device tables first"""
    mp = A.AlignMaps([len(c[0]) for c in cases], [(c[1], c[2]) for c in cases], n_states, DEV)
    if tamper is not None:
        tamper(mp)

    def launch(*bufs):
        with launched(VITERBI):
            A.launch_viterbi(mp, *bufs)

    return guarded_launch(mp, cases, n_states, workspace_bytes, launch)


def case(size, kind):
    row_state, row_skip = R.case_graph(size[0])
    return padded(R.case_ll(size[0], size[1], kind)), row_state, row_skip


@functools.lru_cache(maxsize=None)
def device_viterbi(size, kind):
    """one single-utterance launch per case, shared by the tests that compare them"""
    from fcl_taco2_amd import alignment

    return run_viterbi(alignment, [case(size, kind)])[0]


def check_failed(got, S, T):
    assert got["ok"] == 0 and got["score"] == -np.inf and (got["frame_row"] == -1).all() and len(got["frame_row"]) == T
    assert not got["row_frames"].any() and (got["row_begin"] == got["frame0"]).all() and len(got["row_frames"]) == S


def check_path(got, ll, row_state, row_skip):
    """the path is valid and row_begin / row_frames say what frame_row says"""
    S, T = len(row_state), len(ll)
    assert got["ok"] == 1 and R.path_valid(got["frame_row"], row_skip)
    begin, count = R.runs(got["frame_row"], S)
    assert np.array_equal(got["row_frames"], count) and np.array_equal(got["row_begin"], begin + got["frame0"]) and count.sum() == T


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: "%dx%d" % s)
def test_viterbi_vs_float64(A, size, kind):
    """With gamma = 1.01 (T + 2) 2^-24 and A the sum of |ll| along the path: the path is valid; the score is within gamma A of the float64 sum s64(G)
    along the GPU's own path G; 0 <= V64 - s64(G) <= 2.1 gamma A against the float64 optimum (the lower end less the rounding of the two float64
    sums, T 2^-52 A).  The float32 recurrence in numpy gives the kernel's path and score bit for bit (one rounded add per cell on either side)."""
    S, T = size
    ll, row_state, row_skip = case(size, kind)
    got = device_viterbi(size, kind)
    want = R.viterbi(ll, row_state, row_skip)
    if size == (3, 2):
        assert want["ok"] == 0
        check_failed(got, S, T)
        return
    assert want["ok"] == 1
    check_path(got, ll, row_state, row_skip)
    s64, absum = R.path_score(ll, row_state, got["frame_row"])
    gamma = 1.01 * (T + 2) * U
    assert abs(float(got["score"]) - s64) <= gamma * absum, (float(got["score"]), s64, gamma * absum)
    gap = float(want["score"]) - s64
    assert -T * 2.0 ** -52 * absum <= gap <= 2.1 * gamma * absum, (gap, gamma * absum)
    f32 = R.viterbi(ll, row_state, row_skip, dtype=np.float32)
    assert np.array_equal(f32["frame_row"], got["frame_row"]) and f32["score"].tobytes() == got["score"].tobytes()
    if S == 9 and T < 9:
        assert not got["row_frames"][3:6].any()  # fewer frames than rows: the optional phoneme is skipped
    if kind == "planted" and T >= S:
        flat = R.uniform_alignment(T, row_skip)
        assert (np.repeat(np.arange(S), flat) == got["frame_row"]).mean() >= 0.9  # + 8 on the planted cells against sigma 2


def test_viterbi_exact_cases_bit_for_bit(A):
    """integer-valued ll: the float32 sums are exact, so path and score are those of float64, bit for bit; all of them in one launch"""
    cases = []
    for K in (1, 2, 3):
        for seed in range(12):
            S, T = K * (3 + seed % 5), 9 + 2 * seed + (seed % 3)
            cases.append(R.exact_case(S, T, K, 100 * K + seed))
    M = max(c[0].shape[1] for c in cases)
    got = run_viterbi(A, [(np.pad(ll, ((0, 0), (0, M - ll.shape[1]))), rs, sk) for ll, rs, sk in cases], n_states=M)
    n = 0
    for g, (ll, row_state, row_skip) in zip(got, cases):
        want = R.viterbi(ll, row_state, row_skip)
        if not want["ok"]:
            check_failed(g, len(row_state), len(ll))
            continue
        check_path(g, ll, row_state, row_skip)
        assert np.array_equal(g["frame_row"], want["frame_row"]) and float(g["score"]) == float(want["score"])
        n += 1
    assert n >= 30


def test_viterbi_batch_is_bit_for_bit_its_single_launches(A):
    """every size and kind through ONE launch, interleaved (large beside small, the infeasible one in the middle)"""
    order = [(s, k) for s in R.SIZES[::2] + R.SIZES[1::2] for k in R.KINDS]
    got = run_viterbi(A, [case(s, k) for s, k in order])
    for g, (s, k) in zip(got, order):
        one = device_viterbi(s, k)
        assert g["ok"] == one["ok"] and g["score"].tobytes() == one["score"].tobytes() and np.array_equal(g["frame_row"], one["frame_row"]), (s, k)
        assert np.array_equal(g["row_frames"], one["row_frames"]) and np.array_equal(g["row_begin"] - g["frame0"], one["row_begin"] - one["frame0"]), (s, k)


@pytest.mark.parametrize("size", [(9, 9), (257, 511)], ids=lambda s: "%dx%d" % s)
def test_viterbi_survives_non_finite_inputs(A, size):
    """NaN and +-inf sprinkled over ll, a whole frame of NaN, a whole frame of -inf: ok 0 with the failed outputs, or a valid path; the guard zones
    are checked in run_viterbi either way, and the finite neighbour in the same launch is untouched"""
    S, T = size
    ll, row_state, row_skip = case(size, "noise")
    rng = np.random.RandomState(S)
    variants = []
    for what in ("sprinkled", "nan frame", "-inf frame", "+inf frame"):
        bad = ll.copy()
        if what == "sprinkled":
            idx = rng.rand(T, S) < 0.05
            bad[:, :S][idx] = rng.choice([np.nan, np.inf, -np.inf], int(idx.sum())).astype(np.float32)
        else:
            bad[T // 2, :S] = dict(n=np.nan, m=-np.inf, p=np.inf)[{"nan frame": "n", "-inf frame": "m", "+inf frame": "p"}[what]]
        variants.append(bad)
    got = run_viterbi(A, [(v, row_state, row_skip) for v in variants[:2]] + [(ll, row_state, row_skip)] + [(v, row_state, row_skip) for v in variants[2:]])
    clean = got.pop(2)
    one = device_viterbi(size, "noise")
    assert clean["ok"] == 1 and np.array_equal(clean["frame_row"], one["frame_row"]) and clean["score"].tobytes() == one["score"].tobytes()
    for g in got:
        if g["ok"]:
            check_path(g, ll, row_state, row_skip)
        else:
            check_failed(g, S, T)


def test_viterbi_fails_an_utterance_whose_slices_do_not_fit(A):
    """device tables the host cannot check: a cell slice one cell short, a frame slice longer than max_t says, offsets far outside the buffers --
    that utterance gets the failed outputs inside its clamped slices, the guard zones survive (run_viterbi), the other utterance is bit for bit
    its single launch"""
    sizes = [(9, 9), (257, 511)]
    cases = [case(s, "noise") for s in sizes]
    one = device_viterbi(sizes[1], "noise")

    def short_cells(mp):
        off = mp.cell_offs.copy()
        off[1] -= 1  # utterance 0 owns 80 cells for 9 x 9; utterance 1 one more than it needs
        mp.cell_off = torch.from_numpy(off).to(DEV)

    def wild_offsets(mp):
        mp.frame_off = torch.tensor([-5, 9, 1 << 30], dtype=torch.int32, device=DEV)  # utterance 0: frames 0 .. 9; utterance 1: 9 .. 520 after the clamp
        mp.cell_off = torch.tensor([-(1 << 40), 81, 1 << 40], dtype=torch.int64, device=DEV)

    for tamper in (short_cells, wild_offsets):
        got = run_viterbi(A, cases, tamper=tamper)
        if tamper is short_cells:
            check_failed(got[0], 9, 9)
        else:
            check_path(got[0], cases[0][0], cases[0][1], cases[0][2])
        assert got[1]["ok"] == 1 and np.array_equal(got[1]["frame_row"], one["frame_row"]) and got[1]["score"].tobytes() == one["score"].tobytes()

    def long_frames(mp):
        mp.max_t = 300  # utterance 1 has 511 frames

    got = run_viterbi(A, cases, tamper=long_frames)
    check_path(got[0], cases[0][0], cases[0][1], cases[0][2])
    check_failed(got[1], 257, 511)


def test_viterbi_refusals_launch_nothing(A):
    from fcl_taco2_amd import _lib

    z = lambda n, dt=torch.float32: torch.zeros(n, device=DEV, dtype=dt)
    graph = lambda S: (np.zeros(S, np.int32), np.zeros(S, np.int32))
    with launched(absent=(VITERBI,)):
        for T, S, ws_bytes, code in ((4097, 3, None, "-2"), (10, 1025, None, "-2"), (10, 3, 0, "-5")):
            mp = A.AlignMaps([T], [graph(S)], 4, DEV)
            ws = z(mp.workspace_bytes() if ws_bytes is None else 16, torch.uint8)
            with pytest.raises(_lib.FclError, match="error %s" % code):
                A.launch_viterbi(mp, z(T * 4), ws, z(T, torch.int32), z(S, torch.int32), z(S, torch.int32), z(1), z(1, torch.int32))
        mp = A.AlignMaps([], [], 4, DEV)  # an empty batch is no error and no launch
        A.launch_viterbi(mp, z(1), z(1, torch.uint8), z(1, torch.int32), z(1, torch.int32), z(1, torch.int32), z(1), z(1, torch.int32))


# ---- statistics -------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def first_model(seed):
    """the float64 reference's model after the flat start and one round on the synthetic corpus"""
    c = R.corpus(seed)
    return R.fit(c["feats"], c["graphs"], c["M"], 1)[:2]


def test_stats_of_the_gpu_alignments_chain_bit_for_bit(A):
    """two batches of the synthetic corpus, aligned on the device with the reference's first model and accumulated one after the other into the
    same buffers: acc_n exact, acc_s and acc_q bit for bit the float64 chain of align_ref.stats_chain on the same alignments"""
    c = R.corpus(0)
    M, D = c["M"], c["D"]
    mean, var = first_model(0)
    params = tuple(torch.from_numpy(a).to(DEV) for a in R.params32(mean, var))
    acc_n, acc_s, acc_q = Guarded(M, torch.int64).set(np.zeros(M, np.int64)), Guarded(M * D, torch.float64).set(np.zeros(M * D)), Guarded(M * D, torch.float64).set(np.zeros(M * D))
    want_n, want_s, want_q = np.zeros(M, np.int64), np.zeros((M, D)), np.zeros((M, D))
    aligned = 0
    for lo, hi in ((0, 37), (37, 60)):
        feats, graphs = c["feats"][lo:hi], c["graphs"][lo:hi]
        mp = A.AlignMaps([len(x) for x in feats], graphs, M, DEV)
        x = np.concatenate(feats)
        xg, ll = Guarded(x.size).set(x), torch.empty(mp.frames, M, device=DEV)
        ws = torch.empty(mp.workspace_bytes(), device=DEV, dtype=torch.uint8)
        frame_row, row_begin, row_frames = Guarded(mp.frames, torch.int32), Guarded(mp.rows, torch.int32), Guarded(mp.rows, torch.int32)
        score, ok = Guarded(mp.n_utt), Guarded(mp.n_utt, torch.int32)
        with launched(LOGLIK, VITERBI, STATS):
            A.launch_loglik(params, xg.t, ll, mp.frames)
            A.launch_viterbi(mp, ll, ws, frame_row.t, row_begin.t, row_frames.t, score.t, ok.t)
            A.launch_stats(mp, xg.t, row_begin.t, row_frames.t, acc_n.t, acc_s.t.view(M, D), acc_q.t.view(M, D))
        assert all(g.intact() for g in (xg, frame_row, row_begin, row_frames, score, ok, acc_n, acc_s, acc_q))
        assert ok.np().all() and row_frames.np().sum() == mp.frames
        aligned += mp.frames
        state_off, state_rows = R.state_lists(mp.row_states, M)
        assert np.array_equal(state_off, mp.state_offs) and np.array_equal(state_rows, mp.state_rows_h)
        R.stats_chain(x, row_begin.np(), row_frames.np(), state_off, state_rows, want_n, want_s, want_q)
    assert np.array_equal(acc_n.np(), want_n) and want_n.sum() == aligned
    assert acc_s.np().tobytes() == want_s.tobytes() and acc_q.np().tobytes() == want_q.tobytes()
    assert np.abs(want_s).max() > 100.0 and (want_n > 0).sum() >= M - 3


# ---- fit ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_fit_reaches_the_float64_trainers_accuracy(A):
    """Aligner.fit on the synthetic corpus, 4 rounds after the flat start, in two batches: the frame accuracy is at least the float64 trainer's less
    0.002 (a float32 tie may move a boundary), and the durations returned say what the rows say"""
    c = R.corpus(1)
    K = c["K"]
    phones = ["p%d" % i for i in range(R.N_PHONES)] + ["sp"]
    transcripts = [[phones[m // K] for m in g[0][::K]] for g in c["graphs"]]
    cells = sum(len(x) * len(g[0]) for x, g in zip(c["feats"], c["graphs"]))
    al = A.Aligner(DEV, phones, K, optional=("sp",), batch_cells=cells // 2 + 1)
    with launched(LOGLIK, VITERBI, STATS):
        hist = al.fit([torch.from_numpy(x) for x in c["feats"]], transcripts, iterations=4)
        res = al.align([torch.from_numpy(x) for x in c["feats"]], transcripts)
    assert len(hist["score"]) == 4 and hist["failed"] == [[]] * 4 and hist["score"][-1] > hist["score"][0]
    acc = R.frame_accuracy([r["row_frames"] for r in res], c["row_phone"], c["truth"])
    mean, var, _ = R.fit(c["feats"], c["graphs"], c["M"], 4)
    ref = R.frame_accuracy(R.align(c["feats"], c["graphs"], mean, var)[0], c["row_phone"], c["truth"])
    print("fit: frame accuracy %.4f on the device, %.4f in float64" % (acc, ref))
    assert ref >= 0.99 and acc >= ref - 0.002
    for r, tr, x in zip(res, transcripts, c["feats"]):
        per = r["row_frames"].reshape(-1, K).sum(axis=1)
        assert r["ok"] and sum(r["durations"]) == len(x) and r["durations"] == [int(n) for n in per if n > 0]
        assert r["phones"] == [p for p, n in zip(tr, per) if n > 0] and all(p == "sp" for p, n in zip(tr, per) if n == 0)


# ---- driver -------------------------------------------------------------------------------------------------------------------------------------------------
FS, HOP = 22050, 256
TONES = dict(aa=300.0, iy=800.0, uw=1800.0, sh=3500.0)


def _write_wav(path, x, rate=FS):
    pcm = np.clip(np.rint(np.asarray(x, dtype=np.float64) * 32767.0), -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(rate)
        f.writeframes(pcm.tobytes())


@pytest.fixture(scope="module")
def speech(tmp_path_factory):
    """8 wavs of about half a second: one sinusoid per "phoneme", low-level noise for the pause, which the transcript has between two phonemes and
    every other recording leaves out; and `crowded`, whose transcript has more rows than it has frames"""
    root = tmp_path_factory.mktemp("align")
    (root / "wavs").mkdir()
    rng = np.random.RandomState(11)
    names = sorted(TONES)
    lines, truth = [], {}
    for u in range(8):
        labels = [names[i] for i in rng.permutation(4)] + [names[int(rng.randint(4))]]
        labels.insert(2, "sp")
        frames = [0 if p == "sp" and u % 2 else int(rng.randint(5, 10)) for p in labels]
        x = np.concatenate([(0.3 * np.sin(2 * np.pi * TONES[p] * np.arange(n * HOP) / FS) if p != "sp" else np.zeros(n * HOP)) for p, n in zip(labels, frames)])
        x = x[: len(x) - int(rng.randint(1, HOP))]  # T = len(x) // HOP + 1 = sum(frames)
        x = x + 1e-3 * rng.randn(len(x))
        uid = "utt%d" % u
        _write_wav(root / "wavs" / (uid + ".wav"), x)
        lines.append(uid + " " + " ".join(labels))
        truth[uid] = (labels, frames, len(x))
    _write_wav(root / "wavs" / "crowded.wav", 0.3 * np.sin(2 * np.pi * 300.0 * np.arange(20 * HOP) / FS))
    lines.insert(3, "crowded " + " ".join(["aa", "iy"] * 4))  # 24 rows, 21 frames
    (root / "phones.txt").write_text("\n".join(lines) + "\n")
    return dict(root=root, truth=truth, ids=[ln.split()[0] for ln in lines], transcripts={ln.split()[0]: ln.split()[1:] for ln in lines})


def boundary_hits(durations, labels, frames):
    """(hits, boundaries): the true inner boundaries (between the phonemes really there) found within +-2 frames"""
    true_edges = np.cumsum([n for n in frames if n > 0])[:-1]
    got_edges = np.cumsum(durations)[:-1]
    if len(got_edges) != len(true_edges):
        return 0, len(true_edges)
    return int((np.abs(got_edges - true_edges) <= 2).sum()), len(true_edges)


def test_driver_trains_aligns_and_writes_textgrids(A, speech):
    """python -m fcl_taco2_amd.align on the synthetic recordings: the TextGrids read back through read_textgrid + alignment to the durations
    Aligner.align returns on the same features, the last one less by 1; durations sum to T; every mandatory phoneme has >= K frames; the report lists
    the utterance that cannot be aligned; --model reproduces the alignment without training; and at +-2 frames the device loses at most one
    boundary in twenty to the float64 trainer run on the same device features"""
    from fcl_taco2_amd import align as drv, extract_features as X, features, textgrid as TG

    root, ids = speech["root"], speech["ids"]
    common = ["--wav-dir", str(root / "wavs"), "--transcripts", str(root / "phones.txt"), "--optional", "sp", "--verbose", "0"]
    with launched("fx_logmel_kernel<1024>", "ev_cepstra_kernel", LOGLIK, VITERBI, STATS):
        doc = drv.main(common + ["--textgrid-out", str(root / "tg"), "--durations-out", str(root / "dur"), "--model-out", str(root / "m.npz"), "--iterations", "6",
                                 "--report", str(root / "rep.json")])
    assert json.load(open(root / "rep.json")) == doc and doc["n_utt"] == 9 and doc["n_aligned"] == 8 and doc["not_aligned"] == ["crowded"]
    assert len(doc["iterations"]) == 6 and all(it["not_aligned"] == ["crowded"] for it in doc["iterations"]) and doc["settings"]["trained"] is True
    assert doc["settings"]["phones"] == sorted(list(TONES) + ["sp"]) and doc["settings"]["features"]["dim"] == 28 and doc["settings"]["states"] == 3
    assert sorted(p.name for p in (root / "tg").iterdir()) == sorted(u + ".TextGrid" for u in ids if u != "crowded")
    # the same features, the saved model
    model = A.AlignModel.load(str(root / "m.npz"))
    af = A.AlignFeatures(features.FeatureExtractor(features.FeaturePlan(DEV)))
    assert model.settings == af.settings and model.dim == 28 and model.K == 3
    feats = af.from_waves([X.read_wav(str(root / "wavs" / (u + ".wav")), FS) for u in ids], ids=ids)
    trs = [speech["transcripts"][u] for u in ids]
    res = A.Aligner(DEV, model=model, optional=("sp",)).align(feats, trs, ids=ids)
    hits = total = 0
    for u, r, x in zip(ids, res, feats):
        if u == "crowded":
            assert not r["ok"] and r["durations"] is None
            continue
        labels, frames, n_samples = speech["truth"][u]
        T = n_samples // HOP + 1
        assert r["ok"] and x.shape == (T, 28) and sum(r["durations"]) == T and min(r["durations"]) >= 3
        assert [p for p in labels if p != "sp"] == [p for p in r["phones"] if p != "sp"]
        tiers = TG.read_textgrid(str(root / "tg" / (u + ".TextGrid")))
        got_phones, got = TG.alignment(tiers["phones"], FS, HOP)
        assert got_phones == r["phones"] and got == r["durations"][:-1] + [r["durations"][-1] - 1]
        assert tiers["phones"][-1][1] == pytest.approx(n_samples / FS, abs=1e-9)
        assert list(np.load(root / "dur" / (u + ".npy"))) == r["durations"]
        h, n = boundary_hits(r["durations"], labels, frames)
        hits, total = hits + h, total + n
    # --model aligns without training and writes the same files
    with launched(LOGLIK, VITERBI, absent=(STATS,)):
        doc2 = drv.main(common + ["--textgrid-out", str(root / "tg2"), "--model", str(root / "m.npz")])
    assert doc2["not_aligned"] == ["crowded"] and doc2["iterations"] == [] and doc2["settings"]["trained"] is False
    assert doc2["score_per_frame"] == doc["score_per_frame"]
    for u in ids:
        if u != "crowded":
            assert (root / "tg2" / (u + ".TextGrid")).read_bytes() == (root / "tg" / (u + ".TextGrid")).read_bytes()
    # the float64 trainer on the same device features
    keep = [k for k, u in enumerate(ids) if u != "crowded"]
    index = {p: i for i, p in enumerate(model.phones)}
    graphs = [A.build_graph(trs[k], index, {"sp"}, 3, ids[k])[:2] for k in keep]
    f64 = [feats[k].cpu().numpy().astype(np.float64) for k in keep]
    mean, var, _ = R.fit(f64, graphs, model.n_states, 6)
    counts, _ = R.align(f64, graphs, mean, var)
    ref_hits = 0
    for k, c in zip(keep, counts):
        labels, frames, _ = speech["truth"][ids[k]]
        per = c.reshape(-1, 3).sum(axis=1)
        ref_hits += boundary_hits([int(n) for n in per if n > 0], labels, frames)[0]
    print("driver: %d of %d boundaries within 2 frames on the device, %d in float64" % (hits, total, ref_hits))
    assert total >= 32 and hits >= ref_hits - total / 20.0


def test_driver_refuses_before_the_first_device_call(A, speech, tmp_path):
    from fcl_taco2_amd import align as drv

    root = speech["root"]
    base = ["--wav-dir", str(root / "wavs"), "--textgrid-out", str(tmp_path / "tg"), "--verbose", "0", "--transcripts"]
    cases = (("utt0 aa sp\n", "utterance utt0: the optional phoneme 'sp' is the last label"), ("utt0 sp aa iy\n", "is the first label"),
             ("utt0 aa sp sp iy\n", "next to each other"), ("nowav aa iy\n", "nowav.*has no wav"), ("utt0\n", "has no labels"))
    with launched(absent=(LOGLIK, VITERBI, STATS, "fx_logmel_kernel<1024>")):
        for text, msg in cases:
            (tmp_path / "t.txt").write_text(text)
            with pytest.raises(ValueError, match=msg):
                drv.main(base + [str(tmp_path / "t.txt"), "--optional", "sp"])
        A.AlignModel(["aa", "iy"], 3, np.zeros((6, 28)), np.ones((6, 28))).save(str(tmp_path / "m.npz"))
        (tmp_path / "t.txt").write_text("utt0 aa zz iy\n")
        with pytest.raises(ValueError, match="utterance utt0: label 'zz' is not in the inventory"):
            drv.main(base + [str(tmp_path / "t.txt"), "--model", str(tmp_path / "m.npz")])
        (tmp_path / "t.txt").write_text("utt0 aa iy\n")
        with pytest.raises(ValueError, match="was trained on other features"):
            drv.main(base + [str(tmp_path / "t.txt"), "--model", str(tmp_path / "m.npz")])
        _write_wav(tmp_path / "long.wav", np.zeros(4096 * HOP + 10))
        (tmp_path / "t.txt").write_text("long aa iy\n")
        with pytest.raises(ValueError, match="utterance long has 4097 frames"):
            drv.main(["--wav-dir", str(tmp_path), "--textgrid-out", str(tmp_path / "tg"), "--verbose", "0", "--transcripts", str(tmp_path / "t.txt")])
