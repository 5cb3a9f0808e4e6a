"""The hsd_* kernels of csrc/hifigan_sdisc.hip and the autograd modules on them against the float64 statement of tests/hfgs_ref.py.  Every
buffer a kernel writes sits between guard zones filled with a NaN bit pattern, which must survive, and starts as NaN itself; every case reads the library's
launch record.  The chained cases, their inputs, their bounds and the gain are built and checked in hfgs_ref.py / test_hifigan_scale_discriminator_cpu.py."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import hfgd_ref as D
import hfgs_ref as R
import hifigan_ref as H
from test_gpu_features import DEV, Guarded, launched
from test_gpu_pwg_discriminator import share, t
from test_gpu_pwg_generator import record

pytestmark = pytest.mark.gpu
GROUPED = ("hsd_conv_kernel", "hsd_conv_dx_kernel", "hsd_dw_kernel", "hsd_dw_reduce_kernel")
FIRST = ("hsd_first_kernel<fwd>", "hsd_first_kernel<dx>", "hsd_first_kernel<dw>", "hsd_dw_reduce_kernel")
DENSE = ("hpd_conv_kernel", "hpd_conv_dx_kernel", "hpd_dw_kernel", "hpd_dw_reduce_kernel")
SCORE = ("hpd_reduce_kernel<fwd>", "hpd_expand_kernel<dx>", "hpd_dw_small_kernel<score>", "hpd_dw_reduce_kernel")
POOL = ("hsd_pool_kernel<fwd>", "hsd_pool_kernel<dx>")
FWD_KERNELS = (FIRST[0], GROUPED[0], DENSE[0], SCORE[0])
DX_KERNELS = (SCORE[1], DENSE[1], GROUPED[1])
FIRST_DX = FIRST[1]
DW_KERNELS = (GROUPED[2], GROUPED[3], FIRST[2], DENSE[2], DENSE[3], SCORE[2])
SEGMENTS = (1, 2, 40, 41, 130, 7, 300)  # utterances shorter than the kernel among them; 521 rows, the edges inside 128-row tiles


@pytest.fixture(scope="module")
def P():
    assert torch.cuda.is_available()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, hifigan_scale_discriminator

    _lib.load()
    return hifigan_scale_discriminator


# ---- every launch alone, on given inputs ----------------------------------------------------------------------------------------------------------------

def heights(s):
    """SEGMENTS and one more utterance that brings the output rows to 1 061: a second weight-gradient chunk, and no multiple of a 128-row tile"""
    base = sum((h - 1) // s + 1 for h in SEGMENTS)
    return list(SEGMENTS) + [s * (1061 - base)]


def layer_case(P, ci, co, gr, k, s, hs, seed):
    """one layer on given inputs: forward, the input gradient with and without extra, the weight and bias gradients, each against float64 on the same inputs"""
    from fcl_taco2_amd import _lib, ops

    pad = (k - 1) // 2
    plan, maps = P.LayerPlan(DEV, ci, co, k, s, pad, gr, 0.1), P.LayerMaps(hs, k, s, pad, DEV)
    names = dict(first=FIRST, grouped=GROUPED, dense=DENSE, score=SCORE)[plan.kinds[0]]
    n_in, n_out = maps.rows
    cig = ci // gr
    W = R.normal((k, co, cig), seed, np.sqrt(2.0 / (cig * k))).transpose(1, 2, 0)  # [cout, cin / groups, k] with each tap's matrix contiguous
    b = R.normal((co,), seed + 1, 0.1)
    hin = [R.leaky(R.normal((1, h, ci), seed + 2 + i), 0.1) for i, h in enumerate(hs)]
    for a in hin:
        a[:, ::5, ::3] = 0.0  # stored activations that are exactly zero take the slope
    outs = [R.out_rows(h, k, s, pad) for h in hs]
    g = [R.normal((1, o, co), seed + 40 + i) for i, o in enumerate(outs)]
    ex = [R.normal((1, h, ci), seed + 80 + i, 0.3) for i, h in enumerate(hs)]
    wf, wb, bias = P.pack_weights(plan, [t(W)], [t(b)])[0]
    x = Guarded(n_in, ci).set(R.pack(hin))
    y = Guarded(n_out, co)
    with launched(names[0]):
        P.launch_forward(plan, maps, x.t, [(wf, wb, bias)], [y.t])
    got = R.unpack(y.np(), g)
    r_f = max(share(a - w, e) for a, (w, e) in zip(got, (R.layer_forward(W, b, h, s, pad, 0.1, gr, act=co > 1) for h in hin)))
    gd = Guarded(n_out, co).set(R.pack(g))
    r_x = []
    for extra in ([None, Guarded(n_in, ci).set(R.pack(ex))] if ci > 1 else [None]):
        dx = Guarded(n_in, ci)
        args = P._args(plan, maps, 0, g=gd.t, w=wb, y=dx.t, h=x.t if ci > 1 else None, extra=None if extra is None else extra.t)
        with launched(names[1]):
            _lib.check(P._entry(plan, 0, "dx")(C.byref(args), ops._stream()))
        assert dx.intact() and np.isfinite(dx.np()).all()  # every input row is written
        want = [R.layer_dx(W, gg, h, None if extra is None else e, s, pad, 0.1, gr, mask=ci > 1) for gg, h, e in zip(g, hin, ex)]
        r_x.append(max(share(a - w, e) for a, (w, e) in zip(R.unpack(dx.np(), hin), want)))
        assert extra is None or extra.intact()
    dw, db, work = Guarded(k, cig, co), Guarded(co), Guarded(plan.workspace_floats(maps.rows))
    with launched(names[2], names[3]):
        P.launch_backward(plan, maps, gd.t, [], [(wf, wb, bias)], [], None, [(dw.t, db.t)], x=x.t, grads=[], workspace=work.t)
    ref = [R.layer_dw(gg, h, k, s, pad, n_out, gr) for gg, h in zip(g, hin)]
    r_w = share(dw.np().transpose(2, 1, 0) - sum(r[0] for r in ref), sum(r[1] for r in ref))
    r_b = share(db.np() - sum(r[2] for r in ref), sum(r[3] for r in ref))
    assert all(buf.intact() for buf in (x, y, gd, dw, db, work))
    print("layer %d -> %d in %d groups, k %d s %d, %d -> %d rows: share of the bound: forward %.3g, dx %s, dW %.3g, db %.3g" % (
        ci, co, gr, k, s, n_in, n_out, r_f, np.round(r_x, 3), r_w, r_b))
    assert r_f <= 1.0 and max(r_x) <= 1.0 and r_w <= 1.0 and r_b <= 1.0


@pytest.mark.parametrize("k", [41, 11])
@pytest.mark.parametrize("ci,co,gr,s", [(128, 128, 4, 2), (128, 256, 16, 2), (256, 512, 16, 4), (1024, 1024, 16, 1), (64, 64, 4, 3)])
def test_every_grouped_launch_alone_vs_float64(P, ci, co, gr, s, k):
    hs = heights(s)
    assert sum(R.out_rows(h, k, s, (k - 1) // 2) for h in hs) == 1061
    layer_case(P, ci, co, gr, k, s, hs, 3 * k + s + gr)


@pytest.mark.parametrize("k", [3, 5, 15])
def test_the_first_layer_alone_vs_float64(P, k):
    layer_case(P, 1, 128 if k == 15 else 48, 1, k, 1, heights(1), 200 + k)


def test_the_dense_layer_alone_vs_float64(P):
    layer_case(P, 256, 512, 1, 5, 1, heights(1), 300)


def test_the_score_layer_alone_vs_float64(P):
    layer_case(P, 1024, 1, 1, 3, 1, heights(1), 310)


def test_the_pooling_and_its_adjoint_alone_vs_float64(P):
    lens = [1, 2, 3, 130, 401]
    pm = P.PoolMaps(lens, DEV)
    assert pm.out_lens == [R.pooled_length(n) for n in lens] == [1, 2, 2, 66, 201]
    xs = R.signals(lens, 77)
    x, y = Guarded(pm.rows_in).set(np.concatenate(xs)), Guarded(pm.rows_out)
    with launched(POOL[0]):
        P.launch_pool(pm, x.t, y.t)
    got = np.split(y.np(), np.cumsum(pm.out_lens)[:-1])
    r_f = max(share(a - R.pool(v), 3 * R.U * R.pool(np.abs(v))) for a, v in zip(got, xs))
    gs = [R.normal((n,), 500 + i) for i, n in enumerate(pm.out_lens)]
    g, dx = Guarded(pm.rows_out).set(np.concatenate(gs)), Guarded(pm.rows_in)
    with launched(POOL[1]):
        P.launch_pool(pm, g.t, dx.t, adjoint=True)
    back = np.split(dx.np(), np.cumsum(lens)[:-1])
    r_b = max(share(a - R.pool_adjoint(v, n), 3 * R.U * R.pool_adjoint(np.abs(v), n)) for a, v, n in zip(back, gs, lens))
    assert all(b.intact() for b in (x, y, g, dx)) and np.isfinite(dx.np()).all() and np.isfinite(y.np()).all()
    # the adjoint is the adjoint: <pool x, g> = <x, pool^T g> in float64 on the device's values
    assert np.isclose(sum(a @ v for a, v in zip(got, gs)), sum(a @ v for a, v in zip(back, xs)), rtol=1e-5)
    print("pooling: share of the bound: forward %.3g, adjoint %.3g" % (r_f, r_b))
    assert r_f <= 1.0 and r_b <= 1.0


# ---- one scale discriminator end to end ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def case(name):
    """computed once per chain and shared, read-only"""
    c = R.chain_case(name)
    for a in c["xs"] + c["ds"] + [w for W, b in c["ws"] for w in (W, b)] + [v for r in c["fw"] for key in ("h", "e", "pre") for v in r[key]]:
        a.setflags(write=False)
    return c


class Run(object):
    """one forward pass (and, given dscore, one backward pass) of a packed batch under one scale discriminator on guarded buffers"""

    def __init__(self, P, cfg, ws, xs, ds=None, ex=None, need_x=True, need_w=True):
        self.plan = plan = P.ScalePlan(DEV, **cfg)
        self.maps = maps = P.ScaleMaps(plan, [len(x) for x in xs])
        self.packed = packed = P.pack_weights(plan, [t(W) for W, _ in ws], [None if b is None else t(b) for _, b in ws])
        x = Guarded(maps.rows[0]).set(np.concatenate(xs))
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
        """per utterance the map of layer l (the scores: C = 1) as [1, T_l, C] float64"""
        return R.unpack(self.acts[l].np(), like)

    def bits(self, u):
        """utterance u's part of every map, of the scores and of the waveform gradient, as bytes"""
        per = np.array([self.plan.heights(n) for n in self.maps.lens])
        out = []
        for l, buf in enumerate([self.gx] + self.acts):
            lo, n = int(per[:u, l].sum()), int(per[u, l])
            out.append(buf.t.reshape(self.maps.rows[l], -1)[lo : lo + n].cpu().numpy().tobytes())
        return out

    def weight_bits(self):
        return [b.bits() for pair in self.dws for b in pair if b is not None]


@pytest.mark.parametrize("name", ["A", "B"])
def test_one_scale_discriminator_end_to_end_vs_float64(P, name):
    """a chain configuration at gain 1/4 on (130, 1100, 77, 401, 2500) samples: every map and the scores within the running bound, every layer alone on the
    device's own input within the first term of its bound; then the device's backward on the device's maps with given feature-map gradients: the waveform
    gradient per utterance in norm, every dW and db per element, within the running bounds (unsure mask cells charged their jump)"""
    c = case(name)
    cfg, ws, xs, fw, bw = c["cfg"], c["ws"], c["xs"], c["fw"], c["bw"]
    run = Run(P, cfg, ws, xs, c["ds"], c["ex"])
    geo = R.geometry(cfg)
    worst, local = 0.0, 0.0
    prev = [r["x"] for r in fw]
    for l, ((W, b), (ci, co, k, s, pad, gr)) in enumerate(zip(ws, geo)):
        got = run.h(l, [r["h"][l] for r in fw])
        for u, r in enumerate(fw):
            worst = max(worst, share(got[u] - r["h"][l], r["e"][l]))
            want, e = R.layer_forward(W, b, prev[u], s, pad, cfg["negative_slope"], gr, act=l < len(geo) - 1)
            local = max(local, share(got[u] - want, e))
        prev = got
    gx = np.split(run.gx.np(), np.cumsum([len(x) for x in xs])[:-1])
    r_x = [share(np.linalg.norm(a - b), np.linalg.norm(e)) for a, b, e in zip(gx, bw["gx"], bw["gx_e"])]
    r_w = [share(run.dws[l][0].np().transpose(2, 1, 0) - bw["dw"][l], bw["dw_e"][l]) for l in range(len(geo))]
    r_b = [share(run.dws[l][1].np() - bw["db"][l], bw["db_e"][l]) for l in range(len(geo))]
    print("chain %s: forward share of the running bound %.3g, of a layer's own %.3g; backward: gx %s, dW %s, db %s" % (
        name, worst, local, np.round(r_x, 4), np.round(r_w, 4), np.round(r_b, 4)))
    assert worst <= 1.0 and local <= 1.0 and max(r_x) <= 1.0 and max(r_w) <= 1.0 and max(r_b) <= 1.0


def test_batch_equals_per_utterance_runs_and_two_runs_give_the_same_bits(P):
    c = case("A")
    cfg, ws, xs, ds, ex = c["cfg"], c["ws"], c["xs"], c["ds"], c["ex"]
    run, again = Run(P, cfg, ws, xs, ds, ex), Run(P, cfg, ws, xs, ds, ex)
    assert run.weight_bits() == again.weight_bits() and run.gx.bits() == again.gx.bits()
    for u in range(len(xs)):
        one = Run(P, cfg, ws, [xs[u]], [ds[u]], [ex[u]], need_w=False)
        assert one.bits(0) == run.bits(u), u


def test_changing_one_utterance_leaves_the_others_bit_identical(P):
    c = case("B")
    other = list(c["xs"])
    other[2] = R.signals([len(other[2])], 9)[0]
    a = Run(P, c["cfg"], c["ws"], c["xs"], c["ds"], c["ex"], need_w=False)
    b = Run(P, c["cfg"], c["ws"], other, c["ds"], c["ex"], need_w=False)
    for u in range(len(other)):
        same = [x == y for x, y in zip(a.bits(u), b.bits(u))]
        assert all(same) if u != 2 else not any(same), (u, same)


# ---- the modules ------------------------------------------------------------------------------------------------------------------------------------------

def load(disc, ws, uv=None):
    """the given plain weights into a module of any norm form (weight norm: v = w, g = |w|; spectral norm: weight_orig = w with the given u, v)"""
    with torch.no_grad():
        for l, (c, (W, b)) in enumerate(zip(disc.conv_list(), ws)):
            w = t(W)
            if "weight" in c._parameters:
                c.weight.copy_(w)
            elif "weight_orig" in c._parameters:
                c.weight_orig.copy_(w), c.weight_u.copy_(t(uv[l][0])), c.weight_v.copy_(t(uv[l][1]))
            else:
                c.weight_v.copy_(w), c.weight_g.copy_(torch.linalg.vector_norm(w, dim=(1, 2), keepdim=True))
            if b is not None:
                c.bias.copy_(t(b))
    return disc


def test_module_input_forms_agree_and_padding_gets_zero_gradient(P):
    c = case("B")
    m = load(P.HiFiGANScaleDiscriminator(use_weight_norm=False, **c["cfg"]).to(DEV), c["ws"])
    lens = [40, 64, 1]
    xs = R.signals(lens, 5)
    T = 64
    eq = t(np.stack(R.signals([T, T], 6)))
    with launched(*FWD_KERNELS):
        o2 = m(eq)
    assert len(o2) == 4 and o2[0].shape == (2 * 64, 64) and o2[1].shape == (2 * 16, 64) and o2[2].shape == (2 * 16, 128) and o2[-1].shape == (2 * 16,)
    for other in (m(eq[:, None, :]), m(eq.reshape(-1), lens=[T, T])):
        assert all(torch.equal(a, b) for a, b in zip(other, o2))
    views = P.to_reference_layout(o2, 2)
    assert views[0].shape == (2, 64, 64) and views[1].shape == (2, 64, 16) and views[-1].shape == (2, 1, 16)
    fw = R.forward(c["cfg"], c["ws"], [eq[1].cpu().numpy().astype(np.float64)])[0]
    assert np.allclose(views[1][1].detach().cpu().numpy(), fw["h"][1][0].T, rtol=1e-4, atol=1e-6)  # [C, T_1] of utterance 1
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
    with pytest.raises(ValueError, match="lens"):
        m(torch.zeros(101, device=DEV), lens=[100, 2])


def test_modules_omit_the_gradients_nobody_asks_for(P):
    m = P.HiFiGANMultiScaleDiscriminator(scales=2, discriminator_params=dict(R.CHAIN_A)).to(DEV)
    lens = list(R.MSD_LENS)
    x, y = t(np.concatenate(R.signals(lens, 1))), t(np.concatenate(R.signals(lens, 2)))
    with record() as seen:  # the generator's update: the weights are frozen, the feature maps carry gradients
        for q in m.parameters():
            q.requires_grad_(False)
        xr = x.clone().requires_grad_(True)
        outs = m(xr, lens=lens)
        with torch.no_grad():
            real = m(y, lens=lens)
        (P.generator_adversarial_loss(outs) + 2.0 * P.feature_match_loss(outs, real)).backward()
    assert not [k for k in seen if "dw" in k], sorted(seen)
    assert seen[FIRST_DX]["launches"] == 2 and seen[GROUPED[1]]["launches"] == 2 * 2 and seen[DENSE[1]]["launches"] == 2 and seen[SCORE[1]]["launches"] == 2
    assert seen[GROUPED[0]]["launches"] == 2 * 2 * 2 and seen[POOL[0]]["launches"] == 2 and seen[POOL[1]]["launches"] == 1
    assert set(seen) == set(FWD_KERNELS) | set(DX_KERNELS) | {FIRST_DX} | set(POOL)  # no launch of their own for the feature-map gradients
    assert xr.grad is not None and bool(xr.grad.abs().sum() > 0) and all(q.grad is None for q in m.parameters())
    with record() as seen:  # the discriminator's update: the fake is detached
        for q in m.parameters():
            q.requires_grad_(True)
        sum(P.discriminator_adversarial_loss(m(y, lens=lens), m(xr.detach(), lens=lens))).backward()
    assert set(DW_KERNELS) <= seen.keys() and FIRST_DX not in seen and POOL[1] not in seen, sorted(seen)
    assert seen[GROUPED[2]]["launches"] == 2 * 2 * 2 and seen[FIRST[2]]["launches"] == 2 * 2
    assert all(q.grad is not None and bool(torch.isfinite(q.grad).all()) for q in m.parameters())
    with record() as seen:
        with torch.no_grad():
            m(x, lens=lens)
    assert set(seen) == set(FWD_KERNELS) | {POOL[0]}


def test_multi_scale_discriminator_and_the_three_losses_vs_float64(P):
    """three scales on MSD_CFG, discriminator 0 under spectral norm (eval mode), the others under weight norm; the real and the fake batch packed into one
    forward.  The module's own float32 folded weights are first checked against the float64 fold (spectral norm: within the worst case of a float32
    sigma; weight norm: 4 u), then the reference runs on them: the three losses within their bounds, and the gradient of adv + 2 fm to the fake waveform
    -- the sum over the scales through the pooling's adjoints -- per utterance within the running bound (unsure mask and L1 cells charged their jumps)"""
    inp = R.msd_inputs()
    cfg = inp["cfg"]
    msd = P.HiFiGANMultiScaleDiscriminator(scales=3, discriminator_params=dict(cfg), follow_official_norm=True).to(DEV).eval()
    assert [d.use_spectral_norm for d in msd.discriminators] == [True, False, False]
    folded = []
    for i, (d, ws) in enumerate(zip(msd.discriminators, inp["orig"])):
        load(d, ws, inp["uv"])
        for q in d.parameters():
            q.requires_grad_(False)
        mine = [c.folded().detach().cpu().numpy().astype(np.float64) for c in d.conv_list()]
        for l, (w, (W, _)) in enumerate(zip(mine, ws)):
            want, ulps = (inp["fold64"][l], R.spectral_w_ulps(W, *inp["uv"][l])) if i == 0 else (W, 4)
            assert share(w - want, ulps * R.U * np.abs(want)) <= 1.0, (i, l)
        folded.append(mine)
    m = R.msd_case(folded)
    ref = m["ref"]
    assert ref["unsure"] <= R.CAP, ref["shares"]
    lens = list(R.MSD_LENS)
    fake = t(np.concatenate(m["fake"])).requires_grad_(True)
    real = t(np.concatenate(m["real"]))
    with launched(*(FWD_KERNELS + POOL[:1])):
        outs_real, outs_fake = P.split_batch(msd(torch.cat([real, fake]), lens=lens + lens))
    adv, fm = P.generator_adversarial_loss(outs_fake), P.feature_match_loss(outs_fake, outs_real)
    d_real, d_fake = P.discriminator_adversarial_loss(outs_real, outs_fake)
    with launched(POOL[1], FIRST_DX):
        (adv + 2.0 * fm).backward()
    got = dict(adv=adv.item(), fm=fm.item(), d_real=d_real.item(), d_fake=d_fake.item())
    # beside the statement's bound, the device's own float32 evaluation of a loss: below 32 u of the value (as for the periods)
    shares = {k: abs(v - ref[k]) / (ref[k + "_e"] + 32 * R.U * abs(ref[k])) for k, v in got.items()}
    gx = np.split(fake.grad.cpu().numpy().astype(np.float64), np.cumsum(lens)[:-1])
    r = [share(np.linalg.norm(a - b), np.linalg.norm(e)) for a, b, e in zip(gx, ref["gx"], ref["gx_e"])]
    print("multi-scale: losses %s, their shares of the bound %s, gradient share per utterance %s, unsure cells %.4f" % (
        got, {k: round(v, 4) for k, v in shares.items()}, np.round(r, 4), ref["unsure"]))
    assert max(shares.values()) <= 1.0 and max(r) <= 1.0


def test_one_generator_and_one_discriminator_step_of_the_integration_example(P):
    """INTEGRATION.md "Training a HiFi-GAN generator against the multi-scale multi-period discriminator" on small networks: the discriminator's update on
    the detached fake, then the generator's update with 45 mel + adv + 2 fm against the frozen discriminator; every parameter gets a gradient exactly where
    it should"""
    from fcl_taco2_amd import hifigan_generator, mel_loss

    torch.manual_seed(0)
    gen = hifigan_generator.TrainableHiFiGANGenerator(**{k: v for k, v in H.SMALL.items() if k != "negative_slope"}).to(DEV)
    disc = P.HiFiGANMultiScaleMultiPeriodDiscriminator(scales=2, scale_discriminator_params=dict(R.MSD_CFG), periods=(2, 3),
                                                       period_discriminator_params=dict(D.SMALL)).to(DEV)
    assert disc.msd.discriminators[0].use_spectral_norm and disc.msd.discriminators[1].use_weight_norm
    mel_fn = mel_loss.MelSpectrogramLoss(DEV, fft_sizes=(512,), hop_sizes=(128,), win_lengths=(512,))
    opt_g, opt_d = torch.optim.Adam(gen.parameters(), 2e-4, betas=(0.5, 0.9)), torch.optim.Adam(disc.parameters(), 2e-4, betas=(0.5, 0.9))
    before = [q.detach().clone() for q in list(gen.parameters()) + list(disc.parameters())]
    u0 = disc.msd.discriminators[0].layers[0][0].weight_u.clone()
    frames = [40, 40]
    lens = [n * gen.hop for n in frames]
    mel = torch.randn(2, 80, 40, device=DEV)
    wav = 0.1 * torch.randn(2, 1, lens[0], device=DEV)
    fake = gen(mel, frames)
    # the discriminator's step
    outs = disc(wav)
    assert len(outs) == 2 + 2 and [len(o) for o in outs] == [4, 4, 6, 6]
    real_loss, fake_loss = P.discriminator_adversarial_loss(outs, disc(fake.detach()))
    opt_d.zero_grad()
    (real_loss + fake_loss).backward()
    assert all(q.grad is not None and bool(torch.isfinite(q.grad).all()) and bool(q.grad.abs().sum() > 0) for q in disc.parameters())
    assert all(q.grad is None for q in gen.parameters())
    assert not torch.equal(disc.msd.discriminators[0].layers[0][0].weight_u, u0)  # training mode: the power iteration ran
    opt_d.step()
    # the generator's step against the frozen discriminator: real and fake in one forward, no weight-gradient launch
    opt_d.zero_grad(set_to_none=True)
    for q in disc.parameters():
        q.requires_grad_(False)
    with record() as seen:
        both = torch.cat([wav.reshape(2, -1), fake.reshape(2, -1)])
        outs_real, outs_fake = P.split_batch(disc(both))
        mel_l = mel_fn(fake, wav, lens)
        adv, fm = P.generator_adversarial_loss(outs_fake), P.feature_match_loss(outs_fake, outs_real)
        opt_g.zero_grad()
        (45.0 * mel_l + 1.0 * adv + 2.0 * fm).backward()
    assert not [k for k in seen if k.startswith(("hsd_", "hpd_")) and "dw" in k], sorted(seen)
    assert all(q.grad is not None and bool(torch.isfinite(q.grad).all()) for q in gen.parameters()) and all(q.grad is None for q in disc.parameters())
    opt_g.step()
    for q in disc.parameters():
        q.requires_grad_(True)
    vals = [v.item() for v in (real_loss, fake_loss, mel_l, adv, fm)]
    print("one HiFi-GAN step against scales and periods: real %.4f fake %.4f mel %.4f adv %.4f fm %.4f" % tuple(vals))
    assert np.isfinite(vals).all()
    after = list(gen.parameters()) + list(disc.parameters())
    assert all(bool(torch.isfinite(q).all()) and not torch.equal(q, r) for q, r in zip(after, before))
