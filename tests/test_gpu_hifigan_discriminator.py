"""The hpd_* kernels of csrc/hifigan_disc.hip and the autograd modules on them against the float64 statement of tests/hfgd_ref.py.  Every
buffer a kernel writes sits between guard zones filled with a NaN bit pattern, which must survive, and starts as NaN itself; every case reads the library's
launch record.  The chained cases, their inputs, their bounds and the gain are built and checked in hfgd_ref.py / test_hifigan_discriminator_cpu.py."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import hfgd_ref as R
import hifigan_ref as H
from test_gpu_features import DEV, Guarded, launched
from test_gpu_pwg_discriminator import share, t
from test_gpu_pwg_generator import record

pytestmark = pytest.mark.gpu
MID = ("hpd_conv_kernel", "hpd_conv_dx_kernel", "hpd_dw_kernel", "hpd_dw_reduce_kernel")
FIRST = ("hpd_expand_kernel<fwd>", "hpd_reduce_kernel<dx>", "hpd_dw_small_kernel<first>", "hpd_dw_reduce_kernel")
SCORE = ("hpd_reduce_kernel<fwd>", "hpd_expand_kernel<dx>", "hpd_dw_small_kernel<score>", "hpd_dw_reduce_kernel")
FWD_KERNELS = (FIRST[0], MID[0], SCORE[0])
DX_KERNELS = (SCORE[1], MID[1])
FIRST_DX = FIRST[1]
DW_KERNELS = (MID[2], FIRST[2], SCORE[2], MID[3])


@pytest.fixture(scope="module")
def P():
    assert torch.cuda.is_available()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, hifigan_discriminator

    _lib.load()
    return hifigan_discriminator


# ---- every launch alone, on given inputs ----------------------------------------------------------------------------------------------------------------

def heights(s, big=True):
    """segments of one row, every residue of H mod 3, edges inside a 128-row tile, one segment across a weight-gradient chunk (more than 1 024 output
    rows), a total that is no multiple of a tile"""
    return [1, 2, 3, 4, 5, 130, 1, 77] + ([1030 * s + 1] if big else [])


def layer_case(P, ci, co, k, s, pad, hs, seed):
    """one layer on given inputs: forward, the input gradient with and without extra, the weight and bias gradients, each against float64 on the same inputs"""
    from fcl_taco2_amd import _lib, ops

    plan, maps = P.LayerPlan(DEV, ci, co, k, s, pad, 0.1), P.LayerMaps(hs, k, s, pad, DEV)
    n_in, n_out = maps.rows
    W = R.normal((k, co, ci), seed, np.sqrt(2.0 / (ci * k))).transpose(1, 2, 0)  # [cout, cin, k] with each tap's matrix contiguous: the reference's products run in BLAS
    b = R.normal((co,), seed + 1, 0.1)
    hin = [R.leaky(R.normal((1, h, ci), seed + 2 + i), 0.1) for i, h in enumerate(hs)]
    for a in hin:
        a[:, ::5, ::3] = 0.0  # stored activations that are exactly zero take the slope
    outs = [R.out_rows(h, k, s, pad) for h in hs]
    g = [R.normal((1, o, co), seed + 40 + i) for i, o in enumerate(outs)]
    ex = [R.normal((1, h, ci), seed + 80 + i, 0.3) for i, h in enumerate(hs)]
    wf, wb, bias = P.pack_weights(plan, [t(W)[..., None]], [t(b)])[0]
    names = FIRST if ci == 1 else SCORE if co == 1 else MID
    x = Guarded(n_in, ci).set(R.pack(hin))
    y = Guarded(n_out, co)
    with launched(names[0]):
        P.launch_forward(plan, maps, x.t, [(wf, wb, bias)], [y.t])
    got = R.unpack(y.np(), g)
    r_f = max(share(a - w, e) for a, (w, e) in zip(got, (R.layer_forward(W, b, h, s, pad, 0.1, act=co > 1) for h in hin)))
    gd = Guarded(n_out, co).set(R.pack(g))
    r_x = []
    for extra in ([None, Guarded(n_in, ci).set(R.pack(ex))] if ci > 1 else [None]):
        dx = Guarded(n_in, ci)
        args = P._args(plan, maps, 0, g=gd.t, w=wb, y=dx.t, h=x.t if ci > 1 else None, extra=None if extra is None else extra.t)
        with launched(names[1]):
            _lib.check(_lib.load().fcl_hpd_layer_dx(C.byref(args), ops._stream()))
        assert dx.intact() and np.isfinite(dx.np()).all()  # every input row is written
        want = [R.layer_dx(W, gg, h, None if extra is None else e, s, pad, 0.1, mask=ci > 1) for gg, h, e in zip(g, hin, ex)]
        r_x.append(max(share(a - w, e) for a, (w, e) in zip(R.unpack(dx.np(), hin), want)))
        assert extra is None or extra.intact()
    dw, db, work = Guarded(k, ci, co), Guarded(co), Guarded(plan.workspace_floats(maps.rows))
    with launched(names[2], names[3]):
        P.launch_backward(plan, maps, gd.t, [], [(wf, wb, bias)], [], None, [(dw.t, db.t)], x=x.t, grads=[], workspace=work.t)
    ref = [R.layer_dw(gg, h, k, s, pad, n_out) for gg, h in zip(g, hin)]
    r_w = share(dw.np().transpose(2, 1, 0) - sum(r[0] for r in ref), sum(r[1] for r in ref))
    r_b = share(db.np() - sum(r[2] for r in ref), sum(r[3] for r in ref))
    assert all(buf.intact() for buf in (x, y, gd, dw, db, work))
    print("layer %d -> %d k %d s %d: share of the bound: forward %.3g, dx %s, dW %.3g, db %.3g" % (ci, co, k, s, r_f, np.round(r_x, 3), r_w, r_b))
    assert r_f <= 1.0 and max(r_x) <= 1.0 and r_w <= 1.0 and r_b <= 1.0


@pytest.mark.parametrize("widths", [(16, 64), (32, 128), (128, 512)])
@pytest.mark.parametrize("s", [1, 2, 3, 4])
@pytest.mark.parametrize("k", [3, 5])
def test_every_strided_launch_alone_vs_float64(P, k, s, widths):
    layer_case(P, widths[0], widths[1], k, s, (k - 1) // 2, heights(s), 7 * k + s)


@pytest.mark.parametrize("ci,co,s", [(512, 1024, 3), (1024, 1024, 1), (48, 80, 2)])
def test_the_full_widths_alone_vs_float64(P, ci, co, s):
    """about 70 output rows at the default widths (and one width of a single column tile per workgroup)"""
    layer_case(P, ci, co, 5, s, 2, [1, 4, 11 * s, 47 * s + 1, 2, 9 * s - 1], 90 + s)


@pytest.mark.parametrize("co,k,s", [(16, 5, 3), (144, 3, 4), (32, 3, 1), (1024, 5, 2)])
def test_the_first_layer_alone_vs_float64(P, co, k, s):
    layer_case(P, 1, co, k, s, (k - 1) // 2, heights(s), 200 + s)


@pytest.mark.parametrize("ci,k", [(64, 2), (144, 3), (1024, 2)])
def test_the_score_layer_alone_vs_float64(P, ci, k):
    layer_case(P, ci, 1, k, 1, 1, heights(1), 300 + k)


# ---- one period end to end --------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def case(p):
    """computed once per period and shared, read-only"""
    c = R.period_case(p)
    for a in c["xs"] + c["ds"] + [w for W, b in c["ws"] for w in (W, b)] + [v for r in c["fw"] for key in ("h", "e", "pre") for v in r[key]]:
        a.setflags(write=False)
    return c


class Run(object):
    """one forward pass (and, given dscore, one backward pass) of a packed batch under one period on guarded buffers"""

    def __init__(self, P, cfg, p, ws, xs, ds=None, ex=None, need_x=True, need_w=True):
        self.plan = plan = P.PeriodPlan(DEV, period=p, **cfg)
        self.maps = maps = P.PeriodMaps(plan, [len(x) for x in xs])
        self.like = [R.fold(x, p) for x in xs]
        self.packed = packed = P.pack_weights(plan, [t(W)[..., None] for W, _ in ws], [None if b is None else t(b) for _, b in ws])
        x = Guarded(maps.rows[0]).set(R.pack(self.like))
        assert torch.equal(x.t, t(np.concatenate(xs))[maps.gather])  # the device's fold is the statement's
        self.acts = [Guarded(*s) for s in plan.act_shapes(maps.rows)]
        held = [x] + self.acts
        with launched(*FWD_KERNELS):
            P.launch_forward(plan, maps, x.t, packed, [a.t for a in self.acts])
        if ds is not None:
            L = plan.layers
            dscore = Guarded(maps.rows[-1]).set(R.pack(ds))
            extras = [None if ex is None or ex[0][l] is None else Guarded(*self.acts[l].shape).set(R.pack([e[l] for e in ex])) for l in range(L - 1)]
            self.gx = Guarded(maps.rows[0]) if need_x else None
            self.dws = [(Guarded(*sw), Guarded(*sb) if cfg["bias"] else None) for sw, sb in plan.dweight_shapes()] if need_w else None
            grads, work = [Guarded(*a.shape) for a in self.acts[:-1]], Guarded(plan.workspace_floats(maps.rows))
            with launched(*(DX_KERNELS + ((FIRST_DX,) if need_x else ()) + (DW_KERNELS if need_w else ()))):
                P.launch_backward(plan, maps, dscore.t, [None if e is None else e.t for e in extras], packed, [a.t for a in self.acts[:-1]],
                                  None if self.gx is None else self.gx.t,
                                  None if self.dws is None else [(dw.t, None if db is None else db.t) for dw, db in self.dws], x=x.t,
                                  grads=[g.t for g in grads], workspace=work.t)
            held += [dscore, work] + grads + [e for e in extras if e is not None] + ([self.gx] if need_x else [])
            held += [b for pair in (self.dws or []) for b in pair if b is not None]
            assert all(np.isfinite(g.np()).all() for g in grads)
        assert all(b.intact() for b in held)

    def h(self, l, like):
        """per utterance the map of layer l (the scores: C = 1) as [p, H, C] float64"""
        return R.unpack(self.acts[l].np(), like)

    def gx_unfolded(self, xs, p):
        return [R.unfold_adjoint(g, len(x), p) for g, x in zip(R.unpack(self.gx.np(), self.like), xs)]

    def bits(self, u):
        """utterance u's part of every map, of the scores and of the packed waveform gradient, as bytes"""
        per = np.array([self.plan.heights(n) for n in self.maps.lens])
        out = []
        for l, buf in enumerate([self.gx] + self.acts):
            lo, n = self.plan.period * int(per[:u, l].sum()), self.plan.period * int(per[u, l])
            out.append(buf.t.reshape(self.maps.rows[l], -1)[lo : lo + n].cpu().numpy().tobytes())
        return out

    def weight_bits(self):
        return [b.bits() for pair in self.dws for b in pair if b is not None]


@pytest.mark.parametrize("p", R.PERIODS)
def test_one_period_end_to_end_vs_float64(P, p):
    """SMALL at gain 1/4 on (11, 130, 1100, 77, 401) samples: every map and the scores within the running bound, every layer alone on the device's own input
    within the first term of its bound; then the device's backward on the device's maps: the waveform gradient per utterance in norm, every dW and db per
    element, within the running bounds (unsure mask cells charged their jump)"""
    c = case(p)
    cfg, ws, xs, fw, bw = c["cfg"], c["ws"], c["xs"], c["fw"], c["bw"]
    run = Run(P, cfg, p, ws, xs, c["ds"], c["ex"])
    geo = R.geometry(cfg)
    worst, local = 0.0, 0.0
    prev = [r["x"] for r in fw]
    for l, ((W, b), (ci, co, k, s, pad)) in enumerate(zip(ws, geo)):
        got = run.h(l, [r["h"][l] for r in fw])
        for u, r in enumerate(fw):
            worst = max(worst, share(got[u] - r["h"][l], r["e"][l]))
            want, e = R.layer_forward(W, b, prev[u], s, pad, cfg["negative_slope"], act=l < len(geo) - 1)
            local = max(local, share(got[u] - want, e))
        prev = got
    r_x = [share(np.linalg.norm(a - b), np.linalg.norm(e)) for a, b, e in zip(run.gx_unfolded(xs, p), bw["gx"], bw["gx_e"])]
    r_w = [share(run.dws[l][0].np().transpose(2, 1, 0) - bw["dw"][l], bw["dw_e"][l]) for l in range(len(geo))]
    r_b = [share(run.dws[l][1].np() - bw["db"][l], bw["db_e"][l]) for l in range(len(geo))]
    print("period %d: forward share of the running bound %.3g, of a layer's own %.3g; backward: gx %s, dW %s, db %s" % (
        p, worst, local, np.round(r_x, 4), np.round(r_w, 4), np.round(r_b, 4)))
    assert worst <= 1.0 and local <= 1.0 and max(r_x) <= 1.0 and max(r_w) <= 1.0 and max(r_b) <= 1.0


@pytest.mark.parametrize("p", (3, 11))
def test_batch_equals_per_utterance_runs_and_two_runs_give_the_same_bits(P, p):
    c = case(p)
    cfg, ws, xs, ds, ex = c["cfg"], c["ws"], c["xs"], c["ds"], c["ex"]
    run, again = Run(P, cfg, p, ws, xs, ds, ex), Run(P, cfg, p, ws, xs, ds, ex)
    assert run.weight_bits() == again.weight_bits() and run.gx.bits() == again.gx.bits()
    for u in range(len(xs)):
        one = Run(P, cfg, p, ws, [xs[u]], [ds[u]], [ex[u]], need_w=False)
        assert one.bits(0) == run.bits(u), u


def test_changing_one_utterance_leaves_the_others_bit_identical(P):
    p = 5
    c = case(p)
    other = list(c["xs"])
    other[2] = R.signals([len(other[2])], 9)[0]
    a = Run(P, c["cfg"], p, c["ws"], c["xs"], c["ds"], c["ex"], need_w=False)
    b = Run(P, c["cfg"], p, c["ws"], other, c["ds"], c["ex"], need_w=False)
    for u in range(len(other)):
        same = [x == y for x, y in zip(a.bits(u), b.bits(u))]
        assert all(same) if u != 2 else not any(same), (u, same)


# ---- the modules ------------------------------------------------------------------------------------------------------------------------------------------

def load(disc, ws):
    with torch.no_grad():
        for c, (W, b) in zip(disc.conv_list(), ws):
            w = t(W)[..., None]
            if "weight" in c._parameters:
                c.weight.copy_(w)
            else:
                c.weight_v.copy_(w), c.weight_g.copy_(torch.linalg.vector_norm(w, dim=(1, 2, 3), keepdim=True))
            if b is not None:
                c.bias.copy_(t(b))
    return disc


def test_module_input_forms_agree_and_padding_gets_zero_gradient(P):
    c = case(3)
    m = load(P.HiFiGANPeriodDiscriminator(period=3, use_weight_norm=False, **c["cfg"]).to(DEV), c["ws"])
    lens = [40, 64, 11]
    xs = R.signals(lens, 5)
    T = 64
    eq = t(np.stack(R.signals([T, T], 6)))
    with launched(*FWD_KERNELS):
        o2 = m(eq)
    assert len(o2) == 6 and o2[0].shape == (2 * 3 * 8, 16) and o2[-1].dim() == 1
    for other in (m(eq[:, None, :]), m(eq.reshape(-1), lens=[T, T])):
        assert all(torch.equal(a, b) for a, b in zip(other, o2))
    views = P.to_reference_layout(o2, 3, 2)
    assert views[0].shape == (2, 16, 8, 3) and views[-1].shape == (2, o2[-1].numel() // 2)
    fw = R.forward(c["cfg"], c["ws"], [eq[1].cpu().numpy().astype(np.float64)], 3)[0]
    assert np.allclose(views[1][1].detach().cpu().numpy(), fw["h"][1].transpose(2, 1, 0), rtol=1e-4, atol=1e-6)  # [C, H, p] of utterance 1
    x = t(np.concatenate(xs)).requires_grad_(True)
    out = m(x, lens=lens)
    gs = [torch.randn_like(o) for o in out]
    torch.autograd.backward(out, gs)
    xp = t(np.stack([np.concatenate([v, np.full(T - len(v), 0.25)]) for v in xs])).requires_grad_(True)  # the padding would matter if it were read
    outp = m(xp, lens=lens)
    assert all(torch.equal(a, b) for a, b in zip(outp, out))
    torch.autograd.backward(outp, gs)
    for b, n in enumerate(lens):
        assert torch.equal(xp.grad[b, :n], x.grad[sum(lens[:b]) : sum(lens[:b]) + n]) and not bool(xp.grad[b, n:].any())
    keep = m._maps
    m(x.detach(), lens=lens)
    assert m._maps is keep  # the maps are kept for the next batch of the same lengths
    with pytest.raises(ValueError, match="lens="):
        m(torch.zeros(101, device=DEV), lens=[100, 1])


def test_modules_omit_the_gradients_nobody_asks_for(P):
    m = P.HiFiGANMultiPeriodDiscriminator(periods=(2, 5), discriminator_params=dict(R.SMALL)).to(DEV)
    lens = list(R.MPD_LENS)
    x, y = t(np.concatenate(R.signals(lens, 1))), t(np.concatenate(R.signals(lens, 2)))
    with record() as seen:  # the generator's update: the weights are frozen, the feature maps carry gradients
        for q in m.parameters():
            q.requires_grad_(False)
        xr = x.clone().requires_grad_(True)
        outs = m(xr, lens=lens)
        with torch.no_grad():
            real = m(y, lens=lens)
        (P.generator_adversarial_loss(outs) + 2.0 * P.feature_match_loss(outs, real)).backward()
    assert not [k for k in seen if k.startswith("hpd_dw")], sorted(seen)
    assert seen[FIRST_DX]["launches"] == 2 and seen[MID[1]]["launches"] == 2 * 4 and seen[SCORE[1]]["launches"] == 2
    assert seen[MID[0]]["launches"] == 2 * 2 * 4  # no launch of their own for the feature-map gradients: nothing else ran
    assert set(seen) == set(FWD_KERNELS) | set(DX_KERNELS) | {FIRST_DX}
    assert xr.grad is not None and bool(xr.grad.abs().sum() > 0) and all(q.grad is None for q in m.parameters())
    with record() as seen:  # the discriminator's update: the fake is detached
        for q in m.parameters():
            q.requires_grad_(True)
        sum(P.discriminator_adversarial_loss(m(y, lens=lens), m(xr.detach(), lens=lens))).backward()
    assert set(DW_KERNELS) <= seen.keys() and FIRST_DX not in seen, sorted(seen)
    assert seen[MID[2]]["launches"] == 2 * 2 * 4 and seen[MID[3]]["launches"] == 2 * 2 * 6
    assert all(q.grad is not None and bool(torch.isfinite(q.grad).all()) for q in m.parameters())
    with record() as seen:
        with torch.no_grad():
            m(x, lens=lens)
    assert set(FWD_KERNELS) == set(seen)


def test_weight_norm_state_dict_loads_into_a_plain_module_with_the_same_scores(P):
    a = P.HiFiGANMultiPeriodDiscriminator(discriminator_params=dict(R.SMALL)).to(DEV)
    with torch.no_grad():
        for d in a.discriminators:
            for c in d.conv_list():
                c.weight_g.mul_(torch.rand_like(c.weight_g) + 0.5), c.bias.normal_(0, 0.1)
    b = P.HiFiGANMultiPeriodDiscriminator(discriminator_params=dict(R.SMALL, use_weight_norm=False)).to(DEV)
    b.load_state_dict({"model": {"discriminator": a.state_dict()}})
    x = t(np.stack(R.signals([300, 300], 3)))
    with torch.no_grad():
        oa, ob = a(x), b(x)
        assert all(torch.equal(u, v) for pa, pb in zip(oa, ob) for u, v in zip(pa, pb)) and all(bool(pa[-1].abs().sum() > 0) for pa in oa)
        a.remove_weight_norm()
        assert all(torch.equal(u, v) for pa, pb in zip(a(x), ob) for u, v in zip(pa, pb))


def test_multi_period_discriminator_and_the_three_losses_vs_float64(P):
    """the real and the fake batch packed into one forward; the three losses within the bounds that the scores' and the maps' bounds give them, and the gradient
    of adv + 2 fm to the fake waveform per utterance within the running bound (unsure mask and L1 cells charged their jumps)"""
    m = R.mpd_case()
    ref, cfg = m["ref"], m["cfg"]
    assert ref["unsure"] <= R.CAP
    mpd = P.HiFiGANMultiPeriodDiscriminator(discriminator_params=dict(cfg, use_weight_norm=False)).to(DEV)
    for d, ws in zip(mpd.discriminators, m["wss"]):
        load(d, ws)
        for q in d.parameters():
            q.requires_grad_(False)
    lens = list(R.MPD_LENS)
    fake = t(np.concatenate(m["fake"])).requires_grad_(True)
    real = t(np.concatenate(m["real"]))
    with launched(*FWD_KERNELS):
        outs_real, outs_fake = P.split_batch(mpd(torch.cat([real, fake]), lens=lens + lens))
    adv, fm = P.generator_adversarial_loss(outs_fake), P.feature_match_loss(outs_fake, outs_real)
    d_real, d_fake = P.discriminator_adversarial_loss(outs_real, outs_fake)
    (adv + 2.0 * fm).backward()
    got = dict(adv=adv.item(), fm=fm.item(), d_real=d_real.item(), d_fake=d_fake.item())
    # beside the statement's bound, the device's own float32 evaluation of a loss: two roundings per cell, a tree sum of fewer than 2^14 cells (16), the
    # mean and the averages over layers and discriminators (4) -> below 32 u of the value
    shares = {k: abs(v - ref[k]) / (ref[k + "_e"] + 32 * R.U * abs(ref[k])) for k, v in got.items()}
    gx = np.split(fake.grad.cpu().numpy().astype(np.float64), np.cumsum(lens)[:-1])
    r = [share(np.linalg.norm(a - b), np.linalg.norm(e)) for a, b, e in zip(gx, ref["gx"], ref["gx_e"])]
    print("multi-period: losses %s, their shares of the bound %s, gradient share per utterance %s" % (got, {k: round(v, 4) for k, v in shares.items()}, np.round(r, 4)))
    assert max(shares.values()) <= 1.0 and max(r) <= 1.0


def test_one_generator_and_one_discriminator_step_of_the_integration_example(P):
    """INTEGRATION.md "Training a HiFi-GAN generator against the period discriminator" on the small generator: the discriminator's update on the detached
    fake, then the generator's update with 45 mel + adv + 2 fm"""
    from fcl_taco2_amd import hifigan_generator, mel_loss

    torch.manual_seed(0)
    gen = hifigan_generator.TrainableHiFiGANGenerator(**{k: v for k, v in H.SMALL.items() if k != "negative_slope"}).to(DEV)
    mpd = P.HiFiGANMultiPeriodDiscriminator(discriminator_params=dict(R.SMALL)).to(DEV)
    mel_fn = mel_loss.MelSpectrogramLoss(DEV, fft_sizes=(512,), hop_sizes=(128,), win_lengths=(512,))
    opt_g, opt_d = torch.optim.Adam(gen.parameters(), 2e-4, betas=(0.5, 0.9)), torch.optim.Adam(mpd.parameters(), 2e-4, betas=(0.5, 0.9))
    before = [q.detach().clone() for q in list(gen.parameters()) + list(mpd.parameters())]
    frames = [40, 40]
    lens = [n * gen.hop for n in frames]
    mel = torch.randn(2, 80, 40, device=DEV)
    wav = 0.1 * torch.randn(2, 1, lens[0], device=DEV)
    fake = gen(mel, frames)
    # the discriminator's step
    real_loss, fake_loss = P.discriminator_adversarial_loss(mpd(wav), mpd(fake.detach()))
    opt_d.zero_grad()
    (real_loss + fake_loss).backward()
    opt_d.step()
    # the generator's step: real and fake in one forward
    both = torch.cat([wav.reshape(2, -1), fake.reshape(2, -1)])
    outs_real, outs_fake = P.split_batch(mpd(both))
    mel_l = mel_fn(fake, wav, lens)
    adv, fm = P.generator_adversarial_loss(outs_fake), P.feature_match_loss(outs_fake, outs_real)
    opt_g.zero_grad()
    (45.0 * mel_l + 1.0 * adv + 2.0 * fm).backward()
    opt_g.step()
    vals = [v.item() for v in (real_loss, fake_loss, mel_l, adv, fm)]
    print("one HiFi-GAN step: real %.4f fake %.4f mel %.4f adv %.4f fm %.4f" % tuple(vals))
    assert np.isfinite(vals).all()
    after = list(gen.parameters()) + list(mpd.parameters())
    assert all(bool(torch.isfinite(q).all()) and not torch.equal(q, r) for q, r in zip(after, before))
