"""The hft_* kernels of csrc/hifigan_train.hip and the autograd module on them against the float64 statement of tests/hfgt_ref.py.
Every buffer a kernel writes sits between guard zones filled with a NaN bit pattern, which must survive, and starts as NaN; every kernel test reads the
library's launch record and fails if its kernels did not run.  The cases, their inputs and their bounds are built and checked in hfgt_ref.py /
test_hifigan_generator_cpu.py."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import hfgt_ref as R
import hifigan_ref as H
from test_gpu_features import DEV, Guarded, launched
from test_gpu_pwg_discriminator import share, split, t
from test_gpu_pwg_generator import record

pytestmark = pytest.mark.gpu
LENS, N = list(R.LENS), sum(R.LENS)
F64 = np.float64


@pytest.fixture(scope="module")
def G():
    assert torch.cuda.is_available()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, hifigan_generator

    _lib.load()
    return hifigan_generator


def call(G, entry, args):
    from fcl_taco2_amd import _lib, ops

    _lib.check(getattr(_lib.load(), entry)(C.byref(args), ops._stream()))


def conv_cell(G, x, w, b, res, g, d, act):
    """every convolution launch alone on the statement's own inputs, to the first term of its bound"""
    cout, cin, k = w.shape
    maps = G.Maps(LENS, DEV)
    wf, wdx = G.pack_conv(t(w))
    x64, w64, b64, r64, g64 = (np.asarray(v, F64) for v in (x, w, b, res, g))
    xb, rb, gb, bias = Guarded(N, cin).set(x), Guarded(N, cout).set(res), Guarded(N, cout).set(g), t(b)
    held, shares = [xb, rb, gb], {}
    for name, rs in (("bias", None), ("bias+res", rb)):
        y = Guarded(N, cout)
        with launched(G.CONV_FWD):
            call(G, "fcl_hft_conv_fwd", G.conv_args(maps, cin, cout, k, d, R.SLOPE, act, x=xb.t, w=wf, bias=bias, res=None if rs is None else rs.t, y=y.t))
        want, e = R.conv_fwd(x64, w64, b64, d, LENS, act=act, res=None if rs is None else r64)
        shares["fwd " + name] = share(y.np() - want, e)
        held.append(y)
    # the input gradient: g [N, cout] -> [N, cin]; the mask's pre-activation and the carry are arrays of the case, taken as given
    pre = r64[:, ::-1][:, :cin].copy()
    carry = x64[::-1].copy()
    pb, cb = Guarded(N, cin).set(pre), Guarded(N, cin).set(carry)
    for name, p, cy in (("mask", pb, None), ("mask+carry", pb, cb), ("plain", None, None)):
        dx = Guarded(N, cin)
        with launched(G.CONV_DX):
            call(G, "fcl_hft_conv_dx", G.conv_args(maps, cout, cin, k, d, R.SLOPE, x=gb.t, w=wdx, pre=None if p is None else p.t,
                                                   res=None if cy is None else cy.t, y=dx.t))
        want, e, _ = R.conv_dx(g64, w64, d, LENS, pre=None if p is None else pb.np(), carry=None if cy is None else cb.np())
        shares["dx " + name] = share(dx.np() - want, e)
        held.append(dx)
    dw, db = Guarded(k, cin, cout), Guarded(cout)
    from fcl_taco2_amd import _lib

    work = Guarded(_lib.load().fcl_hft_workspace_bytes(N, cin, cout, k, 1) // 4)
    with launched(*G.CONV_DW):
        call(G, "fcl_hft_conv_dw", G.conv_args(maps, cin, cout, k, d, R.SLOPE, act, x=xb.t, g=gb.t, dw=dw.t, db=db.t, workspace=work.t))
    wW, wb_, eW, eb = R.conv_dw(x64, g64, k, d, LENS, act=act)
    shares["dw"], shares["db"] = share(dw.np().transpose(2, 1, 0) - wW, eW), share(db.np() - wb_, eb)
    held += [pb, cb, dw, db, work]
    print({n: round(v, 4) for n, v in shares.items()})
    assert all(np.isfinite(b_.np()).all() for b_ in held if b_ is not work)
    assert max(shares.values()) <= 1.0
    assert all(b_.intact() for b_ in held)


@pytest.mark.parametrize("k,d,c", R.CONV_CELLS)
def test_convolution_launches_alone_vs_float64(G, k, d, c):
    x, w, b, res, g = R.conv_case(k, d, c)
    conv_cell(G, x, w, b, res, g, d, 1)


def test_input_conv_shape_alone_vs_float64(G):
    """80 -> 512 at k 7 with the plain operand: 8 column blocks forward, 5 one-tile column blocks in the input gradient"""
    x, w, b, res, g = R.conv_case(7, 1, 80, 512)
    conv_cell(G, x, w, b, res, g, 1, 0)


@pytest.mark.parametrize("s,cin,lens", R.TCONV_CELLS)
def test_transposed_convolution_alone_vs_float64(G, s, cin, lens):
    from fcl_taco2_amd import _lib

    x, w, b = H.tconv_case(H.SEEDS["tconv"], s, cin, lens)
    n, cout = sum(lens), cin // 2
    du_ = np.random.RandomState(s).standard_normal((n * s, cout)).astype(np.float32)
    maps = G.Maps(lens, DEV)
    wf, wdx = G.pack_tconv(t(w), s)
    xb, dub, u, dc, dw, db = Guarded(n, cin).set(x), Guarded(n * s, cout).set(du_), Guarded(n * s, cout), Guarded(n, cin), Guarded(2 * s, cin, cout), Guarded(cout)
    work = Guarded(_lib.load().fcl_hft_workspace_bytes(n, cin, cout, 2 * s, s) // 4)
    with launched(G.TCONV_FWD):
        call(G, "fcl_hft_tconv_fwd", G.tconv_args(maps, cin, cout, s, R.SLOPE, c=xb.t, w=wf, bias=t(b), u=u.t))
    with launched(G.TCONV_DX):
        call(G, "fcl_hft_tconv_dx", G.tconv_args(maps, cin, cout, s, R.SLOPE, c=xb.t, w=wdx, du=dub.t, dc=dc.t))
    with launched(*G.TCONV_DW):
        call(G, "fcl_hft_tconv_dw", G.tconv_args(maps, cin, cout, s, R.SLOPE, c=xb.t, du=dub.t, dw=dw.t, db=db.t, workspace=work.t))
    x64, w64, b64, du64 = (np.asarray(v, F64) for v in (x, w, b, du_))
    wu, eu = R.tconv_fwd(x64, w64, b64, s, lens)
    assert np.abs(wu - G.hifigan.tconv_rule(R.lrelu(x64, R.SLOPE), w64, b64, s, lens)).max() < 1e-12  # the package's own index rule on l(x)
    wdc, edc, _ = R.tconv_dx(x64, w64, s, lens, du64)
    wW, wb_, eW, eb = R.tconv_dw(x64, s, lens, du64)
    shares = dict(u=share(u.np() - wu, eu), dc=share(dc.np() - wdc, edc), dw=share(dw.np().transpose(1, 2, 0) - wW, eW), db=share(db.np() - wb_, eb))
    print({n_: round(v, 4) for n_, v in shares.items()})
    assert all(np.isfinite(b_.np()).all() for b_ in (u, dc, dw, db)) and max(shares.values()) <= 1.0
    assert all(b_.intact() for b_ in (xb, dub, u, dc, dw, db, work))


@pytest.mark.parametrize("k,d,c", R.UNIT_CELLS)
def test_unit_end_to_end_vs_the_running_bound(G, k, d, c):
    """forward, then backward on the device's own xt"""
    from fcl_taco2_amd import _lib

    x, w1, b1, w2, b2, g = H.unit_case(H.SEEDS["unit"], k, d, c, LENS)
    maps = G.Maps(LENS, DEV)
    (f1, x1), (f2, x2) = G.pack_conv(t(w1)), G.pack_conv(t(w2))
    xb, gb, xt, xo, dxt, dx = Guarded(N, c).set(x), Guarded(N, c).set(g), Guarded(N, c), Guarded(N, c), Guarded(N, c), Guarded(N, c)
    dws, work = [Guarded(k, c, c), Guarded(c), Guarded(k, c, c), Guarded(c)], Guarded(_lib.load().fcl_hft_workspace_bytes(N, c, c, k, 1) // 4)
    A = functools.partial(G.conv_args, maps, c, c, k)
    with launched(G.CONV_FWD, G.CONV_DX, *G.CONV_DW):
        call(G, "fcl_hft_conv_fwd", A(d, R.SLOPE, 1, x=xb.t, w=f1, bias=t(b1), y=xt.t))
        call(G, "fcl_hft_conv_fwd", A(1, R.SLOPE, 1, x=xt.t, w=f2, bias=t(b2), res=xb.t, y=xo.t))
        call(G, "fcl_hft_conv_dw", A(1, R.SLOPE, 1, x=xt.t, g=gb.t, dw=dws[2].t, db=dws[3].t, workspace=work.t))
        call(G, "fcl_hft_conv_dx", A(1, R.SLOPE, x=gb.t, w=x2, pre=xt.t, y=dxt.t))
        call(G, "fcl_hft_conv_dw", A(d, R.SLOPE, 1, x=xb.t, g=dxt.t, dw=dws[0].t, db=dws[1].t, workspace=work.t))
        call(G, "fcl_hft_conv_dx", A(d, R.SLOPE, x=dxt.t, w=x1, pre=xb.t, res=gb.t, y=dx.t))
    x64, g64 = x.astype(F64), g.astype(F64)
    W = [np.asarray(v, F64) for v in (w1, b1, w2, b2)]
    fw = R.unit_fwd(x64, W[0], W[1], W[2], W[3], d, LENS)
    bw = R.unit_bwd(x64, xt.np(), W[0], W[2], d, LENS, g64)
    got = [dws[0].np().transpose(2, 1, 0), dws[1].np(), dws[2].np().transpose(2, 1, 0), dws[3].np()]
    shares = dict(xt=share(xt.np() - fw["xt"], fw["e_xt"]), xo=share(xo.np() - fw["xo"], fw["e_xo"]), dxt=share(dxt.np() - bw["dxt"], bw["e_dxt"]),
                  dx=share(dx.np() - bw["dx"], bw["e_dx"]), grads=max(share(a - b, e) for a, b, e in zip(got, bw["grads"], bw["e_grads"])))
    print({n: round(v, 4) for n, v in shares.items()})
    assert max(shares.values()) <= 1.0 and all(b_.intact() for b_ in [xb, gb, xt, xo, dxt, dx, work] + dws)


# ---- the stages on guarded buffers -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small():
    sd, mel, dout = R.small_case()
    lens = list(H.GENERATOR_LENS)
    fw = R.generator_fwd(sd, R.SMALL, mel.astype(F64), lens)
    bw = R.generator_bwd(sd, R.SMALL, mel.astype(F64), lens, fw, dout.astype(F64))
    assert bw["unsure"] <= R.MASK_CAP
    return sd, mel, dout, lens, fw, bw


SMALL_ARGS = {k: v for k, v in R.SMALL.items() if k != "negative_slope"}


def stage_params(sd, cfg, i):
    """stage i's parameters in TrainingPlan.stage_params order (numpy)"""
    wt, bt, blocks = R.stage_weights(sd, cfg, i)
    return [wt, bt] + [p for blk in blocks for unit in blk for p in unit]


class Run(object):
    """input_conv and every stage forward, then backward, over a packed batch on guarded buffers"""

    def __init__(self, G, sd, mel, dout, lens, need_c=True, need_w=True):
        from fcl_taco2_amd import _lib

        cfg = R.SMALL
        self.plan = plan = G.TrainingPlan(DEV, **SMALL_ARGS)
        self.maps = maps = G.StageMaps(lens, plan.scales, DEV)
        n0, ci, c0w, k = maps.maps[0].samples, plan.in_channels, plan.widths[0], plan.kernel_size
        melb, self.c0 = Guarded(n0, ci).set(mel), Guarded(n0, c0w)
        wf, wdx = G.pack_conv(t(sd["input_conv.weight"]))
        call(G, "fcl_hft_conv_fwd", G.conv_args(maps.maps[0], ci, c0w, k, 1, R.SLOPE, x=melb.t, w=wf, bias=t(sd["input_conv.bias"]), y=self.c0.t))
        held, c, self.kept, packed = [melb, self.c0], self.c0, [], []
        for i in range(len(plan.scales)):
            w = G.pack_weights(plan, i, [t(p) for p in stage_params(sd, cfg, i)])
            su, sunits, sout = plan.kept_shapes(maps, i)
            u, units, out = Guarded(*su), [[(Guarded(*a), Guarded(*b)) for a, b in blk] for blk in sunits], Guarded(*sout)
            G.launch_stage_forward(plan, maps, i, c.t, w, u.t, [[(a.t, b.t) for a, b in blk] for blk in units], out.t)
            self.kept.append((c, u, units, out))
            packed.append(w)
            held += [u, out] + [b for blk in units for pair in blk for b in pair]
            c = out
        self.out = c
        g, self.grads = Guarded(*self.out.shape).set(dout), {}
        held.append(g)
        work = Guarded(plan.workspace_floats(maps)) if need_w else None
        for i in range(len(plan.scales) - 1, -1, -1):
            c, u, units, _ = self.kept[i]
            dws = None
            if need_w:
                st, sb, su = plan.dweight_shapes(i)
                dws = (Guarded(*st), Guarded(*sb), [[tuple(Guarded(*s) for s in unit) for unit in blk] for blk in su])
                held += [dws[0], dws[1]] + [b for blk in dws[2] for unit in blk for b in unit]
            dc = Guarded(*c.shape) if i > 0 or need_c else None
            scratch = [Guarded(*u.shape) for _ in range(5 + plan.nk)]
            G.launch_stage_backward(plan, maps, i, g.t, c.t, packed[i], u.t, [[(a.t, b.t) for a, b in blk] for blk in units], None if dc is None else dc.t,
                                    None if dws is None else (dws[0].t, dws[1].t, [[tuple(b.t for b in unit) for unit in blk] for blk in dws[2]]),
                                    scratch[0].t, scratch[1].t, [scratch[2].t, scratch[3].t], [s.t for s in scratch[5:]], scratch[4].t,
                                    None if work is None else work.t)
            held += scratch + ([dc] if dc is not None else [])
            if need_w:
                names = [n for n in bw_names(cfg, i)]
                flat = G.unpack_dweights(dws[0].t.reshape(st), dws[1].t, [[tuple(b.t.reshape(b.shape) for b in unit) for unit in blk] for blk in dws[2]])
                self.grads.update({n: v.cpu().numpy().astype(F64) for n, v in zip(names, flat)})
            g = dc
        self.dc0 = g
        self.dmel = None
        if need_c:
            self.dmel = Guarded(n0, ci)
            call(G, "fcl_hft_conv_dx", G.conv_args(maps.maps[0], c0w, ci, k, 1, R.SLOPE, x=g.t, w=wdx, y=self.dmel.t))
            held.append(self.dmel)
        if need_w:
            dw, db, wk = Guarded(k, ci, c0w), Guarded(c0w), Guarded(_lib.load().fcl_hft_workspace_bytes(n0, ci, c0w, k, 1) // 4)
            call(G, "fcl_hft_conv_dw", G.conv_args(maps.maps[0], ci, c0w, k, 1, R.SLOPE, x=melb.t, g=g.t, dw=dw.t, db=db.t, workspace=wk.t))
            self.grads["input_conv.weight"], self.grads["input_conv.bias"] = dw.np().transpose(2, 1, 0), db.np()
            held += [dw, db, wk, work]
        torch.cuda.synchronize()
        assert all(b.intact() for b in held)

    def activations(self):
        """every kept array and input gradient of the batch, in a fixed order"""
        out = [self.c0]
        for c, u, units, o in self.kept:
            out += [u, o] + [b for blk in units for pair in blk for b in pair]
        return out + [self.dc0] + ([self.dmel] if self.dmel is not None else [])


def bw_names(cfg, i):
    nk = len(cfg["resblock_kernel_sizes"])
    names = ["upsamples.%d.1.weight" % i, "upsamples.%d.1.bias" % i]
    for j in range(nk):
        for d in range(len(cfg["resblock_dilations"][j])):
            p = "blocks.%d." % (i * nk + j)
            names += [p + "convs1.%d.1.weight" % d, p + "convs1.%d.1.bias" % d, p + "convs2.%d.1.weight" % d, p + "convs2.%d.1.bias" % d]
    return names


def shares_of(fw, bw, c0, stage_out, us, dmel, grads):
    out = {"c0": share(c0 - fw["c0"], fw["e_c0"])}
    for i, st in enumerate(fw["stages"]):
        out["u%d" % i], out["out%d" % i] = share(us[i] - st["u"], st["e_u"]), share(stage_out[i] - st["out"], st["e_out"])
    if dmel is not None:
        out["dmel"] = share(dmel - bw["dmel"], bw["e_dmel"])
    for k, g in grads.items():
        out[k] = share(g - bw["grads"][k], bw["e_grads"][k])
    return out


def test_stages_vs_the_running_bound_twice_the_same_bits(G):
    sd, mel, dout, lens, fw, bw = small()
    with record() as seen:
        run = Run(G, sd, mel, dout, lens)
    units = sum(len(d) for d in R.SMALL["resblock_dilations"])
    n_st = len(R.SMALL["upsample_scales"])
    assert seen[G.CONV_FWD]["launches"] == 1 + 2 * units * n_st and seen[G.CONV_DX]["launches"] == 1 + 2 * units * n_st and seen[G.CONV_DW[0]]["launches"] == 1 + 2 * units * n_st
    assert seen[G.TCONV_FWD]["launches"] == seen[G.TCONV_DX]["launches"] == seen[G.TCONV_DW[0]]["launches"] == n_st and seen[G.SUM_KERNEL]["launches"] == 3 * n_st
    for i, (c, u, units_, out) in enumerate(run.kept):  # every unit's pre-activations too
        for j, blk in enumerate(units_):
            for d, (xt, xo) in enumerate(blk):
                r = fw["stages"][i]["units"][j][d]
                assert share(xt.np() - r["xt"], r["e_xt"]) <= 1.0 and share(xo.np() - r["xo"], r["e_xo"]) <= 1.0, (i, j, d)
    shares = shares_of(fw, bw, run.c0.np(), [k[3].np() for k in run.kept], [k[1].np() for k in run.kept], run.dmel.np(), run.grads)
    print({k: round(v, 4) for k, v in shares.items()})
    assert set(run.grads) == set(bw["grads"]) and max(shares.values()) <= 1.0
    again = Run(G, sd, mel, dout, lens)
    assert all(a.bits() == b.bits() for a, b in zip(run.activations(), again.activations()))
    assert all(np.array_equal(run.grads[k], again.grads[k]) for k in run.grads)


def test_batch_is_its_utterances_alone_bit_for_bit_and_in_another_order(G):
    sd, mel, dout, lens, fw, bw = small()
    hop = int(np.prod(R.SMALL["upsample_scales"]))
    batch = Run(G, sd, mel, dout, lens, need_w=False)
    mels, douts = split(mel, lens), split(dout, [n * hop for n in lens])
    rates = [1] + list(batch.maps.rates[1:])
    rate_of = [1] + [r for r in rates[1:] for _ in range(2 + 2 * sum(len(d) for d in R.SMALL["resblock_dilations"]))] + [1, 1]
    parts = [split(a.np(), [n * r for n in lens]) for a, r in zip(batch.activations(), rate_of)]
    for b, n in enumerate(lens):
        alone = Run(G, sd, mels[b], douts[b], [n], need_w=False)
        for a, p in zip(alone.activations(), parts):
            assert np.array_equal(a.np(), p[b]), b
    order = [3, 0, 5, 1, 4, 2]
    other = Run(G, sd, np.concatenate([mels[b] for b in order]), np.concatenate([douts[b] for b in order]), [lens[b] for b in order])
    got = split(other.dmel.np(), [lens[b] for b in order])
    want = split(batch.dmel.np(), lens)
    assert all(np.array_equal(got[i], want[b]) for i, b in enumerate(order))
    shares = {k: share(other.grads[k] - bw["grads"][k], bw["e_grads"][k]) for k in other.grads}  # the weight gradients sum in another order: the bound
    assert max(shares.values()) <= 1.0


def test_omission_rules_by_launch_counts(G):
    sd, mel, dout, lens, fw, bw = small()
    n_st = len(R.SMALL["upsample_scales"])
    with record() as seen:
        Run(G, sd, mel, dout, lens, need_c=False, need_w=False)
    assert G.CONV_DW[0] not in seen and G.TCONV_DW[0] not in seen and "hft_dw_reduce_kernel" not in seen
    assert seen[G.TCONV_DX]["launches"] == n_st - 1  # stage 0's input gradient was not asked for


def module_inputs(G, weight_norm):
    sd, mel, dout, lens, fw, bw = small()
    gen = G.TrainableHiFiGANGenerator(use_weight_norm=weight_norm, **SMALL_ARGS)
    src = H.with_weight_norm(sd, np.random.RandomState(2)) if weight_norm else sd
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in src.items()})
    return gen.to(DEV), sd, mel, dout, lens


@pytest.mark.parametrize("weight_norm", [False, True])
def test_autograd_function_and_module_vs_the_running_bound(G, weight_norm):
    """input_conv and upsampling_stages under autograd on the module's own (folded) parameters: the reference takes the device's folded float32 weights as
    given, so the bound is the statement's; the omission rules by launch counts; the module's waveform against the statement carried through the output
    end (a contraction of 7 x 32 products in torch, then tanh at pwgt_ref.E_T = 4 u)"""
    gen, sd, mel, dout, lens = module_inputs(G, weight_norm)
    plan, maps = gen.plan(), gen.maps(lens)
    ws = gen.stage_parameters()
    w_in = gen.input_conv.folded()
    names = [n for i in range(len(plan.scales)) for n in bw_names(R.SMALL, i)]
    own = {n: w.detach().cpu().numpy() for n, w in zip(names, ws)}
    own.update({"input_conv.weight": w_in.detach().cpu().numpy(), "input_conv.bias": gen.input_conv.bias.detach().cpu().numpy()})
    fw = R.generator_fwd(own, R.SMALL, mel.astype(F64), lens)
    bw = R.generator_bwd(own, R.SMALL, mel.astype(F64), lens, fw, dout.astype(F64))
    assert bw["unsure"] <= R.MASK_CAP
    melt = t(mel).requires_grad_(True)
    with record() as seen:
        c0 = G.input_conv(plan, maps, melt, w_in, gen.input_conv.bias)
        x = G.upsampling_stages(plan, maps, c0, *ws)
        grads = torch.autograd.grad(x, [melt, w_in, gen.input_conv.bias] + ws, grad_outputs=t(dout))
    assert seen[G.TCONV_DX]["launches"] == len(plan.scales) and G.CONV_DW[0] in seen and G.TCONV_DW[0] in seen
    got = {n: g.cpu().numpy().astype(F64) for n, g in zip(["mel", "input_conv.weight", "input_conv.bias"] + names, grads)}
    shares = {"out": share(x.detach().cpu().numpy() - fw["out"], fw["e_out"]), "dmel": share(got.pop("mel") - bw["dmel"], bw["e_dmel"])}
    shares.update({k: share(g - bw["grads"][k], bw["e_grads"][k]) for k, g in got.items()})
    print({k: round(v, 4) for k, v in shares.items()})
    assert max(shares.values()) <= 1.0
    # c0 asks for no gradient: one input gradient fewer; no weight asks for one: no weight-gradient launch
    with record() as seen:
        last = ws[-1].detach().requires_grad_(True)
        torch.autograd.grad(G.upsampling_stages(plan, maps, c0.detach(), *[w.detach() for w in ws[:-1]], last), [last], grad_outputs=t(dout))
    assert seen[G.TCONV_DX]["launches"] == len(plan.scales) - 1 and G.CONV_DW[0] in seen
    with record() as seen:
        c0d = c0.detach().requires_grad_(True)
        torch.autograd.grad(G.upsampling_stages(plan, maps, c0d, *[w.detach() for w in ws]), [c0d], grad_outputs=t(dout))
    assert G.CONV_DW[0] not in seen and G.TCONV_DW[0] not in seen and seen[G.TCONV_DX]["launches"] == len(plan.scales)
    # the module's forward on the padded batch
    T, hop = max(lens), plan.hop
    padded = np.zeros((len(lens), 80, T), np.float32)
    for b, m in enumerate(split(mel, lens)):
        padded[b, :, : lens[b]] = m.T
    wav = gen(t(padded), lens)
    assert tuple(wav.shape) == (len(lens), 1, T * hop)
    oc = gen.output_conv.conv
    wo, bo = oc.folded().detach().cpu().numpy().astype(F64), oc.bias.detach().cpu().numpy().astype(F64)
    pre, e_pre = R.conv_fwd(fw["out"], wo, bo, 1, [n * hop for n in lens], slope=float(np.float32(H.OUT_SLOPE)), ex=fw["e_out"])
    off = 0
    for b, n in enumerate(lens):
        got_w = wav[b, 0].detach().cpu().numpy().astype(F64)
        assert share(got_w[: n * hop, None] - np.tanh(pre[off : off + n * hop]), e_pre[off : off + n * hop] + 4 * R.U) <= 1.0, b
        assert not got_w[n * hop :].any()
        off += n * hop


@pytest.mark.parametrize("weight_norm", [False, True])
def test_state_dict_loads_into_the_inference_plan(G, weight_norm):
    """the module's state_dict() in HiFiGANPlan: synthesize_packed's waveform within hifigan_ref.bound of the float64 generator, the module's own forward
    within the training statement's bound of the same waveform"""
    from fcl_taco2_amd import hifigan, vocoder

    gen, sd, mel, dout, lens = module_inputs(G, weight_norm)
    cfg = dict(R.SMALL, negative_slope=0.1)
    inf = hifigan.HiFiGANGenerator(hifigan.HiFiGANPlan(gen.state_dict(), DEV, H.plan_cfg(cfg)))
    wavs = inf.synthesize_packed(t(mel), lens)
    T, hop = max(lens), gen.hop
    padded = np.zeros((len(lens), 80, T), np.float32)
    for b, m in enumerate(split(mel, lens)):
        padded[b, :, : lens[b]] = m.T
    own = gen(t(padded), lens)
    folded = vocoder.fold_weight_norm(gen.state_dict())  # what the plan itself made of the state dict
    for b, (m, w) in enumerate(zip(split(mel, lens), wavs)):
        ref, mod = H.generator_f64(folded, m, cfg), H.generator_f64(folded, m, cfg, rnd=H.plane_round)
        peak = float(ref["wav"].abs().max())
        e_model = float((mod["wav"] - ref["wav"]).abs().max())
        assert float((w.cpu().double().reshape(-1, 1) - ref["wav"]).abs().max()) <= H.bound(e_model, peak), b
        # the module's own forward (exact fp32; its own, far tighter bound is asserted in the test above) meets the inference path's bound too
        assert float((own[b, 0, : lens[b] * hop].detach().cpu().double().reshape(-1, 1) - ref["wav"]).abs().max()) <= H.bound(e_model, peak), b


def test_three_adam_steps_on_the_mel_loss(G):
    from fcl_taco2_amd import mel_loss

    torch.manual_seed(0)
    gen = G.TrainableHiFiGANGenerator(**SMALL_ARGS).to(DEV)
    hop = gen.hop
    lens = [40, 33]
    mel = torch.randn(2, 80, 40, device=DEV)
    real = 0.1 * torch.randn(2, 1, 40 * hop, device=DEV)
    loss_fn = mel_loss.MelSpectrogramLoss(DEV, fft_sizes=(512,), hop_sizes=(128,), win_lengths=(512,))  # 320 and 264 samples: above n_fft / 2 + 1
    opt = torch.optim.Adam(gen.parameters(), lr=1e-3)
    before = {k: v.detach().clone() for k, v in gen.named_parameters()}
    for _ in range(3):
        opt.zero_grad()
        loss = loss_fn(gen(mel, lens), real, [n * hop for n in lens])
        loss.backward()
        assert bool(torch.isfinite(loss))
        opt.step()
    torch.cuda.synchronize()
    for k, v in gen.named_parameters():
        assert v.grad is not None and bool(torch.isfinite(v.grad).all()) and bool(v.grad.abs().max() > 0), k
        assert not torch.equal(v.detach(), before[k]), k
    torch.cuda.synchronize()  # no launch left an error on the device
    assert torch.cuda.current_stream().query()
