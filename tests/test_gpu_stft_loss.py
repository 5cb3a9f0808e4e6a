"""The kernels of csrc/stft_loss.hip, the autograd module on them and `evaluate --aligned` against the float64 statement of tests/stft_loss_ref.py
(DESIGN.md 6j).  Every buffer a kernel writes sits between guard zones filled with a NaN bit pattern, which must survive; every kernel test reads the
library's launch record and fails if its kernels did not run.  The inputs, their bounds and the conditions both have to meet are built and checked
in stft_loss_ref.py / test_stft_loss_cpu.py."""
import functools
import json
import wave

import numpy as np
import pytest
import torch

import stft_loss_ref as S
from test_gpu_features import DEV, Guarded, launched

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
PAT64 = 0x7FF8123456789ABC  # a float64 NaN


@pytest.fixture(scope="module")
def SL():
    assert torch.cuda.is_available()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, stft_loss

    _lib.load()
    return stft_loss


class Guarded64(object):
    """a float64 device buffer of n words between two guard zones"""

    PAD = 1024

    def __init__(self, *shape):
        self.shape, self.n = shape, int(np.prod(shape))
        self.buf = torch.empty(self.n + 2 * self.PAD, dtype=torch.float64, device=DEV)
        self.buf.view(torch.int64).fill_(PAT64)

    @property
    def t(self):
        return self.buf[self.PAD : self.PAD + self.n]

    def np(self):
        return self.t.cpu().numpy().reshape(self.shape)

    def bits(self):
        return self.t.cpu().numpy().tobytes()

    def intact(self):
        b = self.buf.view(torch.int64)
        return bool((b[: self.PAD] == PAT64).all()) and bool((b[self.PAD + self.n :] == PAT64).all())


@functools.lru_cache(maxsize=None)
def reference(case, silent=False):
    """computed once per case and shared, read-only"""
    xs, ys = S.signals(case, silent=silent)
    ref = S.kernel_reference(case, xs, ys, "utterance")
    for v in list(ref.values()) + ref["grad"] + xs + ys:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return xs, ys, ref


def kernel_names(n_fft):
    return ("stl_sums_kernel<%d>" % n_fft, "stl_utt_sums_kernel", "stl_grad_frames_kernel<%d>" % n_fft, "stl_grad_gather_kernel")


def run(SL, case, xs, ys, coef):
    """both entries on guarded buffers -> (maps, frame_sums, utt_sums, gx)"""
    pl = SL.STFTLossPlan(DEV, [case[0]], [case[1]], [case[2]])
    rs = pl.resolutions[0]
    mp = SL.Maps([len(x) for x in xs], rs.hop, DEV)
    n = sum(len(x) for x in xs)
    x, y = Guarded(n).set(np.concatenate(xs)), Guarded(n).set(np.concatenate(ys))
    fs, us = Guarded(mp.frames, 3), Guarded64(mp.n_utt, 3)
    cf, fr, gx = Guarded(mp.n_utt, 2).set(coef), Guarded(mp.frames, rs.n_fft), Guarded(n)
    with launched(*kernel_names(rs.n_fft)):
        SL.launch_sums(rs, mp, x.t, y.t, fs.t, us.t)
        SL.launch_grad(rs, mp, x.t, y.t, cf.t, fr.t, gx.t)
    assert all(b.intact() for b in (x, y, fs, us, cf, fr, gx))
    return mp, fs, us, gx


def split(flat, lens):
    o = np.concatenate([[0], np.cumsum(lens)])
    return [flat[a:b] for a, b in zip(o[:-1], o[1:])]


@pytest.mark.parametrize("case", list(S.CASES), ids=str)
def test_sums_and_gradient_vs_float64(SL, case):
    """frame_sums, utt_sums and gx of one packed batch of three utterances within the derived bounds of stft_loss_ref.py; the coefficients are the
    float64 reference's, rounded to float32 (what the module would pass: the bound's coefficient term covers their error)"""
    xs, ys, ref = reference(case)
    mp, fs, us, gx = run(SL, case, xs, ys, ref["coef"])
    assert mp.frames == len(ref["frame_sums"])
    r_f = (np.abs(fs.np() - ref["frame_sums"]) / ref["frame_bounds"]).max(0)
    r_u = (np.abs(us.np() - ref["utt_sums"]) / ref["utt_bounds"]).max(0)
    g = split(gx.np(), [len(x) for x in xs])
    r_g = np.array([np.linalg.norm(a - b) / e for a, b, e in zip(g, ref["grad"], ref["grad_bounds"])])
    print("stft loss %r: worst share of the bound: frame sums %s, utterance sums %s, gradient %s" % (case, r_f, r_u, r_g))
    assert np.isfinite(fs.np()).all() and np.isfinite(us.np()).all() and np.isfinite(gx.np()).all()
    assert r_f.max() <= 1.0 and r_u.max() <= 1.0 and r_g.max() <= 1.0


def test_silent_utterance_has_an_exactly_zero_gradient(SL):
    """x = 0 in the middle of the batch: every bin of it sits at the clamp, its gradient is bit-exact 0.0, its sums meet their bounds and the
    neighbours' results are those of the batch without silence"""
    case = S.SILENT_CASE
    xs, ys, ref = reference(case, True)
    _, _, ref0 = reference(case)
    assert ref["grad_bounds"][1] == 0.0
    mp, fs, us, gx = run(SL, case, xs, ys, ref["coef"])
    lens = [len(x) for x in xs]
    g = split(gx.np(), lens)
    assert g[1].tobytes() == np.zeros(lens[1]).tobytes()
    assert (np.abs(fs.np() - ref["frame_sums"]) <= ref["frame_bounds"]).all() and (np.abs(us.np() - ref["utt_sums"]) <= ref["utt_bounds"]).all()
    _, fs0, us0, gx0 = run(SL, case, *reference(case)[:2], ref0["coef"])
    g0, f, f0 = split(gx0.np(), lens), split(fs.np(), mp.lens), split(fs0.np(), mp.lens)
    for i in (0, 2):  # utterance coefficients: the neighbours' are their own
        assert g[i].tobytes() == g0[i].tobytes() and f[i].tobytes() == f0[i].tobytes() and us.np()[i].tobytes() == us0.np()[i].tobytes()


@pytest.mark.parametrize("case", [(512, 50, 240), (1024, 120, 600), (2048, 240, 1200)], ids=str)
def test_batch_equals_per_utterance_runs_bit_for_bit(SL, case):
    """one packed batch against three runs of one utterance (another slot of the workgroup, another block, another chunking of nothing: the same
    bits) and against itself"""
    xs, ys, ref = reference(case)
    mp, fs, us, gx = run(SL, case, xs, ys, ref["coef"])
    _, fs2, us2, gx2 = run(SL, case, xs, ys, ref["coef"])
    assert fs.bits() == fs2.bits() and us.bits() == us2.bits() and gx.bits() == gx2.bits()
    f = split(fs.t.reshape(mp.frames, 3).cpu().numpy(), mp.lens)
    g = split(gx.t.cpu().numpy(), [len(x) for x in xs])
    for i in range(len(xs)):
        _, fs1, us1, gx1 = run(SL, case, [xs[i]], [ys[i]], ref["coef"][i : i + 1])
        assert fs1.bits() == f[i].tobytes() and us1.bits() == us.np()[i].tobytes() and gx1.bits() == g[i].tobytes(), i


def test_gather_accumulates_on_request(SL):
    """accumulate adds the resolution's gradient to what gx holds (how the module sums the resolutions); the same launch without it overwrites"""
    case = (512, 50, 240)
    xs, ys, ref = reference(case)
    pl = SL.STFTLossPlan(DEV, [case[0]], [case[1]], [case[2]])
    rs, mp = pl.resolutions[0], SL.Maps([len(x) for x in xs], case[1], DEV)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
    x, y, cf = t(np.concatenate(xs)), t(np.concatenate(ys)), t(ref["coef"])
    fr, gx = torch.empty(mp.frames, rs.n_fft, device=DEV), Guarded(mp.samples)
    SL.launch_grad(rs, mp, x, y, cf, fr, gx.t)
    once = gx.t.clone()
    SL.launch_grad(rs, mp, x, y, cf, fr, gx.t, accumulate=True)
    assert torch.equal(gx.t, once + once) and gx.intact()


def grads_of(x, lens):
    return split(x.grad.detach().cpu().numpy().astype(np.float64).reshape(-1), lens)


def test_module_batch_reduction_on_equal_length_clips(SL):
    """[B, T] = [2, 2100], reduction="batch", the default three resolutions: (sc, mag) and x.grad after (sc + mag).backward() against the float64
    statement within the bounds combined over the resolutions; [B, 1, T] gives the same bits"""
    xs, ys = S.module_signals()
    ref = S.module_reference(xs, ys, S.DEFAULT_RESOLUTIONS, "batch")
    loss = SL.MultiResolutionSTFTLoss(DEV)
    assert [(r.n_fft, r.hop, r.win_length) for r in loss.plan.resolutions] == S.DEFAULT_RESOLUTIONS
    x = torch.from_numpy(np.stack(xs)).to(DEV).requires_grad_(True)
    y = torch.from_numpy(np.stack(ys)).to(DEV)
    names = [n for c in S.DEFAULT_RESOLUTIONS for n in kernel_names(c[0])]
    with launched(*names):
        sc, mag = loss(x, y)
        (sc + mag).backward()
    assert sc.dtype == mag.dtype == torch.float32 and sc.dim() == 0 and x.grad.shape == x.shape
    r_g = [np.linalg.norm(a - b) / e for a, b, e in zip(grads_of(x, [S.MODULE_T] * S.MODULE_B), ref["grad"], ref["grad_bounds"])]
    print("module, batch: sc %.7f (|d| %.2e of %.2e), mag %.7f (|d| %.2e of %.2e), gradient share of the bound %s"
          % (sc.item(), abs(sc.item() - ref["sc"]), ref["sc_bound"], mag.item(), abs(mag.item() - ref["mag"]), ref["mag_bound"], r_g))
    assert abs(sc.item() - ref["sc"]) <= ref["sc_bound"] and abs(mag.item() - ref["mag"]) <= ref["mag_bound"] and max(r_g) <= 1.0
    x3 = x.detach().clone()[:, None, :].requires_grad_(True)
    sc3, mag3 = loss(x3, y[:, None, :])
    (sc3 + mag3).backward()
    assert torch.equal(sc3, sc) and torch.equal(mag3, mag) and torch.equal(x3.grad[:, 0], x.grad)


def test_module_utterance_reduction_on_ragged_input(SL):
    """reduction="utterance" on a ragged packed batch against float64; a padded [B, T] with lens gives the same values and zero gradient in the padding"""
    xs, ys = S.ragged_signals()
    lens = [len(v) for v in xs]
    ref = S.module_reference(xs, ys, S.DEFAULT_RESOLUTIONS, "utterance")
    loss = SL.MultiResolutionSTFTLoss(DEV)
    x = torch.from_numpy(np.concatenate(xs)).to(DEV).requires_grad_(True)
    y = torch.from_numpy(np.concatenate(ys)).to(DEV)
    sc, mag = loss(x, y, lens=lens, reduction="utterance")
    (sc + mag).backward()
    r_g = [np.linalg.norm(a - b) / e for a, b, e in zip(grads_of(x, lens), ref["grad"], ref["grad_bounds"])]
    print("module, utterance: |d sc| %.2e of %.2e, |d mag| %.2e of %.2e, gradient share of the bound %s"
          % (abs(sc.item() - ref["sc"]), ref["sc_bound"], abs(mag.item() - ref["mag"]), ref["mag_bound"], r_g))
    assert abs(sc.item() - ref["sc"]) <= ref["sc_bound"] and abs(mag.item() - ref["mag"]) <= ref["mag_bound"] and max(r_g) <= 1.0
    T = max(lens) + 37
    pad = lambda vs, fill: torch.from_numpy(np.stack([np.concatenate([v, np.full(T - len(v), fill, np.float32)]) for v in vs])).to(DEV)
    xp, yp = pad(xs, 0.25).requires_grad_(True), pad(ys, -0.5)  # the padding holds values that would matter if it were read
    scp, magp = loss(xp, yp, lens=lens, reduction="utterance")
    (scp + magp).backward()
    assert torch.equal(scp, sc) and torch.equal(magp, mag)
    for b, n in enumerate(lens):
        assert torch.equal(xp.grad[b, :n], x.grad[sum(lens[:b]) : sum(lens[:b]) + n]) and not bool(xp.grad[b, n:].any())
    d_sc, d_mag = loss.distances(x.detach(), lens, y)
    assert d_sc.shape == d_mag.shape == (3, 3) and abs(d_sc.mean() - sc.item()) <= 4 * U * sc.item() and abs(d_mag.mean() - mag.item()) <= 4 * U * mag.item()
    with pytest.raises(ValueError, match="utterance tiny has 1024 samples"):
        loss(torch.zeros(3000, device=DEV), torch.zeros(3000, device=DEV), lens=[1976, 1024], ids=["ok", "tiny"])


def test_module_inside_a_graph_with_other_upstream_gradients(SL):
    """x = 0.9 z made by a torch operation, the loss 2 sc + 0.5 mag: z.grad against the float64 statement (0.9 times the gradient at x, the bound
    scaled alike plus the rounding of the product); y.requires_grad and an unknown reduction are refused"""
    zs, ys = S.module_signals()
    xs = [(np.float32(0.9) * z).astype(np.float32) for z in zs]  # what the device computes
    assert all(S.conditions(c, xs, ys) == 1.0 for c in S.DEFAULT_RESOLUTIONS)
    ref = S.module_reference(xs, ys, S.DEFAULT_RESOLUTIONS, "batch", 2.0, 0.5)
    loss = SL.MultiResolutionSTFTLoss(DEV)
    z = torch.from_numpy(np.stack(zs)).to(DEV).requires_grad_(True)
    y = torch.from_numpy(np.stack(ys)).to(DEV)
    x = 0.9 * z
    assert np.array_equal(x.detach().cpu().numpy(), np.stack(xs))
    sc, mag = loss(x, y)
    (2.0 * sc + 0.5 * mag).backward()
    want = [np.float64(np.float32(0.9)) * g for g in ref["grad"]]
    r_g = [np.linalg.norm(a - b) / (0.9 * e + 2 * U * np.linalg.norm(b)) for a, b, e in zip(grads_of(z, [S.MODULE_T] * S.MODULE_B), want, ref["grad_bounds"])]
    print("module in a graph: gradient share of the bound %s" % r_g)
    assert abs(sc.item() - ref["sc"]) <= ref["sc_bound"] and abs(mag.item() - ref["mag"]) <= ref["mag_bound"] and max(r_g) <= 1.0
    with pytest.raises(ValueError, match="must not require a gradient"):
        loss(x.detach(), y.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="reduction"):
        loss(x.detach(), y, reduction="mean")


def _write_wav(path, x, rate=22050):
    pcm = np.clip(np.rint(np.asarray(x, dtype=np.float64) * 32767.0), -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(rate)
        f.writeframes(pcm.tobytes())
    return pcm.astype(np.float32) / np.float32(32768.0)


def test_evaluate_aligned_driver(SL, tmp_path):
    """python -m fcl_taco2_amd.evaluate --aligned on three tiny wav pairs (one synthesised file 100 samples longer than its recording): the records
    carry distances()'s values on the pairs cut to the shorter side, the corpus figures are their means, a pair beyond --aligned-max-diff is refused
    by id, and without --aligned the document has none of the new keys"""
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
    names = [n for c in S.DEFAULT_RESOLUTIONS for n in kernel_names(c[0])[:2]]
    with launched(*names):
        doc = E.main(["--ref-wav-dir", str(rd), "--syn-wav-dir", str(sd), "--aligned", "--out", str(out), "--verbose", "0", "--aligned-batch-samples", "10000"])
    assert json.loads(out.read_text()) == doc and doc["settings"]["aligned"]["max_diff"] == 512
    n = [min(len(refs[u]), len(syns[u])) for u in ids]
    assert n == [4500, 5200, 4740]
    loss = SL.MultiResolutionSTFTLoss(DEV)
    sc, mag = loss.distances([syns[u][:k] for u, k in zip(ids, n)], None, [refs[u][:k] for u, k in zip(ids, n)])
    for k, r in enumerate(doc["utterances"]):
        assert r["id"] == ids[k] and r["aligned_samples"] == n[k] and "mcd_db" in r
        assert r["stft_sc"] == float(np.mean(sc[k])) and r["stft_log_mag"] == float(np.mean(mag[k]))
        assert [(d["n_fft"], d["hop"], d["win_length"]) for d in r["stft"]] == S.DEFAULT_RESOLUTIONS
        assert [d["sc"] for d in r["stft"]] == list(sc[k]) and [d["log_mag"] for d in r["stft"]] == list(mag[k])
        # against float64, loosely: the figure is the statement's (the kernels' own bounds are the tests' above)
        want = [S.figures(*S.utt_sums([syns[ids[k]][: n[k]]], [refs[ids[k]][: n[k]]], S.window(c), c[1]), "utterance") for c in S.DEFAULT_RESOLUTIONS]
        assert np.allclose(sc[k], [w[0] for w in want], rtol=1e-4) and np.allclose(mag[k], [w[1] for w in want], rtol=1e-4)
    assert doc["stft_sc"] == float(np.mean([r["stft_sc"] for r in doc["utterances"]]))
    assert doc["stft_log_mag"] == float(np.mean([r["stft_log_mag"] for r in doc["utterances"]]))
    assert "STFT spectral convergence %.4f" % doc["stft_sc"] in E.summary_line(doc)
    with pytest.raises(ValueError, match="utterance ub has 5200 reference and 5300 synthesised samples"):
        E.main(["--ref-wav-dir", str(rd), "--syn-wav-dir", str(sd), "--aligned", "--aligned-max-diff", "99", "--verbose", "0"])
    plain = E.main(["--ref-wav-dir", str(rd), "--syn-wav-dir", str(sd), "--verbose", "0"])
    assert "stft_sc" not in plain and "aligned" not in plain["settings"] and "STFT" not in E.summary_line(plain)
    assert all(not ({"stft_sc", "stft_log_mag", "stft", "aligned_samples"} & set(r)) for r in plain["utterances"])
    for r, q in zip(plain["utterances"], doc["utterances"]):
        assert r == {k: v for k, v in q.items() if k in r}  # the other figures are untouched by the flag
