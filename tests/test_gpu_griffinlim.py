"""Every kernel of csrc/griffinlim.hip against the float64 numpy statement of tests/griffinlim_ref.py.  Every buffer a kernel writes
sits between guard zones filled with a NaN bit pattern, which must survive; every test reads the library's launch record and fails if its kernel did
not run.  The inputs and their conditions are built and checked in griffinlim_ref.py / test_griffinlim_cpu.py."""
import contextlib
import json
import wave

import numpy as np
import pytest
import torch

import griffinlim_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAT32 = 0x7FC12345  # an fp32 NaN: whatever is read from an unwritten word poisons the result
U = 2.0 ** -24


@pytest.fixture(scope="module")
def GL():
    assert torch.cuda.is_available()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, griffinlim

    _lib.load()
    return griffinlim


@contextlib.contextmanager
def launched(*names):
    """the launches inside run the named kernels (the library's own launch record)"""
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


class Guarded(object):
    """a float32 device buffer of n words between two guard zones; everything starts as the NaN pattern"""

    PAD = 8192

    def __init__(self, *shape, **kw):
        self.shape, self.cplx = shape, kw.get("cplx", False)
        self.n = int(np.prod(shape)) * (2 if self.cplx else 1)
        self.buf = torch.empty(self.n + 2 * self.PAD, dtype=torch.float32, device=DEV)
        self.buf.view(torch.int32).fill_(PAT32)
        assert self.t.data_ptr() % 8 == 0

    @property
    def t(self):
        return self.buf[self.PAD : self.PAD + self.n]

    def set(self, a):
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(a)).view(torch.float32).reshape(-1) if not self.cplx else
                     torch.view_as_real(torch.from_numpy(np.ascontiguousarray(a, dtype=np.complex64))).reshape(-1))
        return self

    def np(self):
        a = self.t.cpu().numpy().astype(np.float64)
        return (a[0::2] + 1j * a[1::2]).reshape(self.shape) if self.cplx else a.reshape(self.shape)

    def intact(self):
        b = self.buf.view(torch.int32)
        return bool((b[: self.PAD] == PAT32).all()) and bool((b[self.PAD + self.n :] == PAT32).all())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def plan_of(GL, case, **kw):
    n_fft, hop, wl = case
    return GL.GriffinLimPlan(DEV, n_fft=n_fft, hop=hop, win_length=wl, **kw)


def f32(a):
    return np.asarray(a).astype(np.complex64 if np.iscomplexobj(a) else np.float32)


def rel2(got, want, axis=None):
    return np.linalg.norm(got - want, axis=axis) / np.linalg.norm(want, axis=axis)


def zero_padded_stft(x, window, hop):
    """the mutant: zero padding in place of the reflection"""
    n_fft, h = len(window), len(window) // 2
    xp = np.concatenate([np.zeros(h), x, np.zeros(h)])
    return np.fft.rfft(np.stack([xp[t * hop : t * hop + n_fft] for t in range(len(x) // hop + 1)]) * window, axis=1)


@pytest.mark.parametrize("case", R.CASES, ids=str)
def test_analysis_vs_float64(GL, case):
    """gl_analysis_kernel alone (momentum 0, no C_prev): every frame's spectrum against float64 in the norm form of Higham's FFT bound,
    ||C_gpu - C||_2 <= 7 (log2(n_fft) + 2) 2^-24 ||C||_2; the utterance list holds the shortest allowed T, about 40 frames and T + 1, so every frame of
    the short ones reflects.  A zero-padding analysis misses the same bound by orders of magnitude (computed here in numpy on the same input)."""
    n_fft, hop, _ = case
    pl = plan_of(GL, case)
    xs = [f32(x) for x in R.case_signals(case)]
    lens = R.utt_lens(n_fft, hop)
    mp = GL.Maps(lens, DEV)
    y = Guarded(sum(len(x) for x in xs)).set(np.concatenate(xs))
    P, Cg = Guarded(mp.frames, pl.bins, cplx=True), Guarded(mp.frames, pl.bins, cplx=True)
    with launched("gl_analysis_kernel<%d>" % n_fft):
        GL.launch_analysis(pl, mp, y.t, P.t, None, Cg.t, 0.0)
    assert P.intact() and Cg.intact() and y.intact()
    w32 = pl.window.astype(np.float32).astype(np.float64)
    want = np.concatenate([R.stft(x.astype(np.float64), w32, hop) for x in xs])
    got, bound = Cg.np(), R.fft_bound(n_fft)
    err = rel2(got, want, axis=1)
    print("analysis %r: worst frame ||dC|| / ||C|| = %.3g, bound %.3g (%.2f of it)" % (case, err.max(), bound, err.max() / bound))
    assert np.isfinite(got).all() and err.max() <= bound
    mutant = np.concatenate([zero_padded_stft(x.astype(np.float64), w32, hop) for x in xs])
    edge = [int(mp.frame_off[i]) for i in range(3)] + [int(mp.frame_off[i + 1]) - 1 for i in range(3)]  # first and last frame of every utterance
    assert rel2(mutant, want, axis=1)[edge].min() > 1e3 * bound
    # the phase the epilogue writes is the written spectrum's own
    big = np.abs(want) >= 1e-3 * np.abs(want).max()
    assert np.abs(P.np() - got / (np.abs(got) + 1e-16))[big].max() < 8 * U


@pytest.mark.parametrize("case", R.CASES + [R.SHORT_WINDOW_CASE], ids=str)
def test_synthesis_and_overlap_add_vs_float64(GL, case):
    """gl_synth_kernel + gl_ola_kernel from given S and P: the windowed frames and every utterance's waveform against the float64 istft in the same norm
    form.  The case with win_length < hop reaches the undivided (window-sum-square <= FLT_MIN) branch (test_griffinlim_cpu.py checks that it does)."""
    n_fft, hop, _ = case
    pl = plan_of(GL, case)
    sp = [(f32(S), f32(P)) for S, P in R.case_spectra(case)]
    lens = R.utt_lens(n_fft, hop)
    mp = GL.Maps(lens, DEV)
    S, P = dev(np.concatenate([s for s, _ in sp])), dev(np.concatenate([p for _, p in sp]))
    fr, y = Guarded(mp.frames, n_fft), Guarded(hop * (mp.frames - 3))
    with launched("gl_synth_kernel<%d>" % n_fft, "gl_ola_kernel"):
        GL.launch_synth(pl, mp, S, P, fr.t)
        GL.launch_ola(pl, mp, fr.t, y.t)
    assert fr.intact() and y.intact()
    w32 = pl.window.astype(np.float32).astype(np.float64)
    bound = R.fft_bound(n_fft)
    frames = np.concatenate([R.synth_frames(s.astype(np.float64) * p.astype(np.complex128), w32) for s, p in sp])
    e_fr = rel2(fr.np(), frames, axis=1).max()
    got, off, worst = y.np(), 0, 0.0
    for i, (s, p) in enumerate(sp):
        want = R.istft(s.astype(np.float64) * p.astype(np.complex128), w32, hop)
        assert want.shape == (hop * (lens[i] - 1),)
        worst = max(worst, rel2(got[off : off + len(want)], want))
        off += len(want)
    print("synthesis %r: worst ||d frame|| / ||frame|| = %.3g, worst ||dy|| / ||y|| = %.3g, bound %.3g" % (case, e_fr, worst, bound))
    assert off == len(got) and np.isfinite(got).all() and e_fr <= bound and worst <= bound


def test_mel_to_linear_vs_float64(GL):
    """gl_mel2lin_kernel against float64 on the float32 inputs.  Per element  |dS| <= sum_c |m_c| |pinv_ck| ((n_mels + 4) 2^-24 + d_c): the first term is
    the fp32 FMA chain over n_mels terms, d_c the relative error of m_c = exp10f(lm_c): 2 ulp = 2^-22 for exp10f itself (HIP's math API table lists 1 ulp,
    CUDA's lists 2; the larger figure is used) plus ln(10) times the rounding of its argument lm = fma(mel, fl(std + 1e-8), mean), at most
    2^-24 (2 |mel| |std| + |lm|).  The floor is 1-Lipschitz, so the bound holds behind it (plus 2^-24 1e-10 for the floor constant in float32); row 5 drives bins negative and must come out as the floor."""
    pl = plan_of(GL, (1024, 256, 1024), mel_stats=R.mel_case()[1])
    mel, stats = (f32(a) for a in R.mel_case())
    S = Guarded(mel.shape[0], pl.bins)
    with launched("gl_mel2lin_kernel"):
        GL.launch_mel2lin(pl, dev(mel), S.t)
    assert S.intact()
    pt = pl.pinv.T.astype(np.float32).astype(np.float64)
    m64, s64 = mel.astype(np.float64), stats.astype(np.float64)
    assert np.array_equal(pl.stats_d.cpu().numpy(), stats) and np.array_equal(pl.pinv_t_d.cpu().numpy().astype(np.float64), pt)
    lm = m64 * (s64[1] + 1e-8) + s64[0]
    m = 10.0 ** lm
    d = 2.0 ** -22 + np.log(10.0) * U * (2 * np.abs(m64 * s64[1]) + np.abs(lm))
    bound = (np.abs(m) * ((pl.A + 4) * U + d)) @ np.abs(pt) + U * 1e-10  # (+ the floor itself, stored as float32(1e-10): bins above fmax have no other term)
    want, got = R.mel_to_linear(mel, stats, pt), S.np()
    ratio = np.abs(got - want) / bound
    print("mel to linear: worst |dS| / bound = %.3f; floored bins in row 5: %d" % (ratio.max(), int((got[5] == np.float32(1e-10)).sum())))
    assert np.isfinite(got).all() and ratio.max() <= 1.0
    assert (got[5] == np.float32(1e-10)).sum() > 10 and got.min() >= np.float32(1e-10)
    # without stats the de-normalisation is the identity
    pl0 = plan_of(GL, (1024, 256, 1024))
    S0 = Guarded(mel.shape[0], pl.bins)
    small = f32(0.3 * mel)
    GL.launch_mel2lin(pl0, dev(small), S0.t)
    want0 = R.mel_to_linear(small, None, pt)
    m0 = 10.0 ** small.astype(np.float64)
    assert S0.intact() and (np.abs(S0.np() - want0) <= (m0 * ((pl.A + 4) * U + 2.0 ** -22)) @ np.abs(pt) + U * 1e-10).all()


def _iter_inputs():
    case = R.ITER_CASE
    sp = [(f32(S), f32(P)) for S, P in R.case_spectra(case)]
    return case, sp, R.utt_lens(case[0], case[1])


@pytest.mark.parametrize("n_iter", [1, 2])
def test_one_and_two_iterations_vs_float64(GL, n_iter):
    """n_iter full iterations from an explicit phase0 at momentum 0.99, launch by launch on guarded buffers.
    P is judged where |A| >= 1e-3 max|A| (test_griffinlim_cpu.py: that leaves out <= 1 % of the bins):  |dP_k| |A_k| <= 2 x 3 n_iter x fft_bound x
    (||C||_2 + alpha ||C_prev||_2) of its frame -- P = A / |A| moves by at most 2 |dA| / |A|, and dA collects three norm-form stages (synthesis,
    overlap-add, analysis) per iteration.  The waveform follows the project's rule err <= 4 max(model, 2^-15 peak), model = the float64 iteration with
    every stored intermediate (frames, y, C, P) rounded to float32."""
    case, sp, lens = _iter_inputs()
    n_fft, hop, _ = case
    pl = plan_of(GL, case, momentum=0.99)
    mp = GL.Maps(lens, DEV)
    S = dev(np.concatenate([s for s, _ in sp]))
    P = Guarded(mp.frames, pl.bins, cplx=True).set(np.concatenate([p for _, p in sp]))
    Cp = Guarded(mp.frames, pl.bins, cplx=True).set(np.zeros((mp.frames, pl.bins), dtype=np.complex64))
    fr, y = Guarded(mp.frames, n_fft), Guarded(hop * (mp.frames - 3))
    with launched("gl_synth_kernel<%d>" % n_fft, "gl_ola_kernel", "gl_analysis_kernel<%d>" % n_fft):
        for _ in range(n_iter):
            GL.launch_synth(pl, mp, S, P.t, fr.t)
            GL.launch_ola(pl, mp, fr.t, y.t)
            GL.launch_analysis(pl, mp, y.t, P.t, Cp.t, None, 0.99)
        p_got = P.np()
        GL.launch_synth(pl, mp, S, P.t, fr.t)
        GL.launch_ola(pl, mp, fr.t, y.t)
    assert P.intact() and Cp.intact() and fr.intact() and y.intact()
    w32 = pl.window.astype(np.float32).astype(np.float64)
    got, alpha, bound = y.np(), 0.99 / 1.99, R.fft_bound(n_fft)
    f0 = s0 = 0
    skipped = total = 0
    worst_p = worst_y = 0.0
    for (s, p), T in zip(sp, lens):
        s64, p64, tr = s.astype(np.float64), p.astype(np.complex128), {}
        y64 = R.griffin_lim(s64, p64, w32, hop, n_iter, 0.99, trace=tr)
        ymod = R.griffin_lim(s64, p64, w32, hop, n_iter, 0.99, round32=True)
        a = np.abs(tr["A"])
        keep = a >= 1e-3 * a.max()
        skipped, total = skipped + int((~keep).sum()), total + keep.size
        cprev = (tr["C"] - tr["A"]) / alpha  # alpha C_prev = C - A
        lim = 2 * 3 * n_iter * bound * (np.linalg.norm(tr["C"], axis=1) + alpha * np.linalg.norm(cprev, axis=1))[:, None]
        worst_p = max(worst_p, float((np.abs(p_got[f0 : f0 + T] - tr["P"]) * a / lim)[keep].max()))
        n = hop * (T - 1)
        e, e_mod, peak = np.abs(got[s0 : s0 + n] - y64).max(), np.abs(ymod - y64).max(), np.abs(y64).max()
        worst_y = max(worst_y, e / (4 * max(e_mod, 2.0 ** -15 * peak)))
        f0, s0 = f0 + T, s0 + n
    print("%d iteration(s): worst |dP| |A| / bound = %.3g (%.2f %% of the bins left out), worst waveform err / bound = %.3g" %
          (n_iter, worst_p, 100.0 * skipped / total, worst_y))
    assert np.isfinite(got).all() and skipped <= 0.01 * total and worst_p <= 1.0 and worst_y <= 1.0


def test_whole_run_converges_like_float64(GL):
    """32 iterations on about 40 frames plus two shortest utterances: the spectral convergence ||  |stft64(y)| - S ||_F / ||S||_F of the device's
    waveform against the float64 run from the same phase0.  The margin comes from the reference alone: the ratio of the worst to the best convergence
    of the float64 run over 8 initial-phase seeds on that input -- float32 rounding is one more perturbation of the trajectory."""
    case = R.ITER_CASE
    n_fft, hop, _ = case
    t = R.min_frames(n_fft, hop)
    lens = [41, t, t]
    w = R.case_window(case)
    w32 = w.astype(np.float32).astype(np.float64)
    specs = [f32(np.abs(R.stft(R.signal(50 + j, hop * (T - 1)), w, hop))) for j, T in enumerate(lens)]
    phases = [[f32(np.exp(2j * np.pi * np.random.RandomState(100 * k + j).uniform(size=s.shape))) for j, s in enumerate(specs)] for k in range(8)]
    pl = plan_of(GL, case, momentum=0.99, n_iter=32)
    gen = GL.GriffinLim(pl)
    mp = GL.Maps(lens, DEV)
    P = dev(np.concatenate(phases[0]))
    with launched("gl_synth_kernel<%d>" % n_fft, "gl_ola_kernel", "gl_analysis_kernel<%d>" % n_fft):
        flat = gen.iterate(mp, dev(np.concatenate(specs)), P)
    got = flat.cpu().numpy().astype(np.float64)
    assert got.shape == (hop * (sum(lens) - 3),) and np.isfinite(got).all()
    off = 0
    for j, (s, T) in enumerate(zip(specs, lens)):
        s64 = s.astype(np.float64)
        sc = [R.spectral_convergence(R.griffin_lim(s64, phases[k][j].astype(np.complex128), w32, hop, 32, 0.99), s64, w32, hop) for k in range(8)]
        n = hop * (T - 1)
        sc_gpu = R.spectral_convergence(got[off : off + n], s64, w32, hop)
        margin = max(sc) / min(sc)
        print("whole run, utterance of %d frames: convergence device %.4g, float64 same phase0 %.4g, over 8 seeds %.4g .. %.4g (margin %.3f)" %
              (T, sc_gpu, sc[0], min(sc), max(sc), margin))
        assert sc_gpu <= sc[0] * margin
        off += n


def test_seeded_draw_equals_the_numpy_twin(GL):
    case = (512, 100, 512)
    pl = plan_of(GL, case)
    lens = [5, 41, 6]
    mp = GL.Maps(lens, DEV)
    seeds = np.array([7, 2 ** 32 - 1, 123456789], dtype=np.uint32)
    P, u = Guarded(mp.frames, pl.bins, cplx=True), Guarded(mp.frames, pl.bins)
    with launched("gl_phase_init_kernel"):
        GL.launch_phase_init(pl, mp, dev(seeds.view(np.int32)), P.t, u.t)
    assert P.intact() and u.intact()
    want = np.concatenate([R.phase_uniforms(int(s), T, pl.bins) for s, T in zip(seeds, lens)])
    assert u.t.cpu().numpy().tobytes() == want.tobytes()  # bit for bit
    assert np.abs(P.np() - np.exp(2j * np.pi * want.astype(np.float64))).max() < 8 * U


def test_batch_equals_per_utterance_runs_and_the_three_entries_agree(GL):
    pl = plan_of(GL, (1024, 256, 1024), n_iter=3, mel_stats=R.mel_case()[1])
    gen = GL.GriffinLim(pl)
    lens = [4, 23, 5]
    rng = np.random.RandomState(9)
    mels = [f32(rng.randn(n, 80) * 0.8) for n in lens]
    with launched("gl_mel2lin_kernel", "gl_phase_init_kernel", "gl_synth_kernel<1024>", "gl_ola_kernel", "gl_analysis_kernel<1024>"):
        batch = gen.synthesize(mels, seed=40)
    packed, flat = gen.synthesize_packed(dev(np.concatenate(mels)), lens, seed=40, return_flat=True)
    assert [tuple(b.shape) for b in batch] == [(256 * (n - 1),) for n in lens] == [(gen.samples_of(n),) for n in lens]
    assert flat.numel() == sum(gen.samples_of(n) for n in lens) and torch.equal(torch.cat(packed), flat)
    for i, m in enumerate(mels):
        alone = gen.synthesize([m], seed=40 + i)[0]  # utterance i of a batch draws from seed + i
        assert torch.isfinite(alone).all() and float(alone.abs().max()) > 0
        assert torch.equal(alone, batch[i]) and torch.equal(alone, packed[i])  # bit for bit
    assert torch.equal(gen.inference(mels[1]), gen.synthesize([mels[1]], seed=0)[0].reshape(-1, 1))
    assert not torch.equal(gen.synthesize([mels[1]], seed=1)[0], gen.synthesize([mels[1]], seed=2)[0])
    with pytest.raises(ValueError, match="utterance #1 has 3 frames"):
        gen.synthesize([mels[0], mels[0][:3]])


def _read_wav(path):
    with wave.open(str(path)) as f:
        return (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()), np.frombuffer(f.readframes(f.getnframes()), dtype="<i2")


def test_vocoder_decode_with_griffin_lim(GL, tmp_path):
    from fcl_taco2_amd import vocoder, vocoder_decode as V
    from fcl_taco2_amd.kaldi_io import ArkScpWriter

    rng = np.random.RandomState(4)
    feats = {"utt%d" % i: f32(rng.randn(n, 80) * 0.8) for i, n in enumerate([30, 4, 17])}
    with ArkScpWriter(str(tmp_path / "feats")) as w:
        for k, m in feats.items():
            w[k] = m
    np.save(tmp_path / "stats.npy", R.mel_case()[1])
    argv = ["--griffin-lim", "--feats-scp", str(tmp_path / "feats.scp"), "--outdir", str(tmp_path / "wav"), "--mel-stats", str(tmp_path / "stats.npy"),
            "--gl-iters", "4", "--batch-frames", "40", "--verbose", "0", "--seed", "3"]
    with launched("gl_mel2lin_kernel", "gl_synth_kernel<1024>", "gl_ola_kernel", "gl_analysis_kernel<1024>"):
        samples, _ = V.main(argv)
    assert samples == 256 * sum(m.shape[0] - 1 for m in feats.values())
    gen = GL.GriffinLim(GL.GriffinLimPlan(DEV, n_iter=4, mel_stats=np.load(tmp_path / "stats.npy")))
    # batches of <= 40 frames, longest first: [utt0], [utt2, utt1]; batch b draws from seed + b, utterance i of it from seed + b + i
    for uid, seed in (("utt0", 3), ("utt2", 4), ("utt1", 5)):
        hdr, pcm = _read_wav(tmp_path / "wav" / (uid + "_gen.wav"))
        want = vocoder.pcm16(gen.synthesize([feats[uid]], seed=seed)[0])
        assert hdr == (1, 2, 22050, 256 * (feats[uid].shape[0] - 1)) and np.array_equal(pcm, want) and np.abs(pcm).max() > 0, uid
    with ArkScpWriter(str(tmp_path / "short")) as w:
        w["ok"], w["tiny"] = feats["utt1"], feats["utt1"][:3]
    with pytest.raises(ValueError, match="utterance tiny has 3 frames"):
        V.main(["--griffin-lim", "--feats-scp", str(tmp_path / "short.scp"), "--outdir", str(tmp_path / "wav2")])


def test_tts_driver_with_griffin_lim(GL, tmp_path):
    """text -> waveform without a vocoder checkpoint: every batch takes the two-step route and is counted as eager, and the audio is what
    vocoder_decode --griffin-lim makes of the mels --feats-out wrote (same batches, same seeds)"""
    from fcl_taco2_amd import hparams as HP, synthetic as SYN, tts as TTS, vocoder_decode as V
    from fcl_taco2_amd.kaldi_io import ArkScpWriter, read_scp

    hp = HP.student_hparams(dropout_rate=0.0)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in SYN.closed_form_state_dict(HP.param_spec(hp, HP.teacher_hparams(), True)).items()}
    sd["duration_predictor.linear.weight"] = torch.zeros_like(sd["duration_predictor.linear.weight"])
    sd["duration_predictor.linear.bias"] = torch.full((1,), float(np.log(4.0)))  # every phoneme predicts 3 frames
    torch.save({"model": sd, "optimizer": {}}, tmp_path / "snapshot.ep.1")
    args = dict(model_module="nets.knowledge_distillation.e2e_tts_tacotron2_sa_kd_student:Tacotron2_sa", embed_dim=256, eunits=256,
                econv_chans=256, dunits=256, postnet_chans=128, use_residual=False, use_masking=True, dropout_rate=0.0, share_proj=True)
    (tmp_path / "model.json").write_text(json.dumps([80, 80, args]))
    (tmp_path / "teacher.json").write_text(json.dumps([80, 80, dict(use_residual=False)]))
    rng = np.random.RandomState(3)
    utts = {"u%02d" % i: {"output": [{"tokenid": " ".join(map(str, rng.randint(1, 80, size=rng.randint(5, 40))))}]} for i in range(7)}
    (tmp_path / "data.json").write_text(json.dumps({"utts": utts}))
    lens = {k: len(v["output"][0]["tokenid"].split()) for k, v in utts.items()}
    np.save(tmp_path / "stats.npy", np.stack([np.full(80, -2.0), np.full(80, 0.05)]))  # keeps 10^lm of the synthetic model's mels in range
    gl = ["--griffin-lim", "--mel-stats", str(tmp_path / "stats.npy"), "--gl-iters", "3", "--verbose", "0"]
    with launched("gl_mel2lin_kernel", "gl_phase_init_kernel", "gl_synth_kernel<1024>", "gl_ola_kernel", "gl_analysis_kernel<1024>"):
        res = TTS.main(["--model", str(tmp_path / "snapshot.ep.1"), "--model-conf", str(tmp_path / "model.json"), "--teacher-config", str(tmp_path / "teacher.json"),
                        "--json", str(tmp_path / "data.json"), "--batch-size", "3", "--seed", "11", "--outdir", str(tmp_path / "wav"),
                        "--feats-out", str(tmp_path / "feats")] + gl)
    assert res["eager_batches"] == 3 == len(res["batches"]) and res["graph_batches"] == 0 and res["redone_batches"] == 0
    assert res["samples"] == 256 * sum(3 * n - 1 for n in lens.values())
    mels = read_scp(str(tmp_path / "feats.scp"))
    for b, (route, ids, seed) in enumerate(res["batches"]):
        assert route == "two-step"
        with ArkScpWriter(str(tmp_path / ("b%d" % b))) as w:
            for k in ids:
                w[k] = mels[k]
        V.main(["--feats-scp", str(tmp_path / ("b%d.scp" % b)), "--outdir", str(tmp_path / ("dec%d" % b)), "--seed", str(seed), "--batch-frames", "100000"] + gl)
        for k in ids:
            hdr, pcm = _read_wav(tmp_path / "wav" / (k + "_gen.wav"))
            hdr2, pcm2 = _read_wav(tmp_path / ("dec%d" % b) / (k + "_gen.wav"))
            assert hdr == hdr2 == (1, 2, 22050, 256 * (3 * lens[k] - 1)) and np.array_equal(pcm, pcm2) and np.abs(pcm).max() > 0, (b, k)
