"""The pwt_* kernels of csrc/pwg_train.hip and the autograd module on them against the float64 statement of tests/pwgt_ref.py.  Every
buffer a kernel writes sits between guard zones filled with a NaN bit pattern, which must survive; what a first / last block writes (skips, dc) starts as
NaN; every kernel test reads the library's launch record and fails if its kernels did not run.  The cases, their inputs and their bounds are built and
checked in pwgt_ref.py / test_pwg_generator_cpu.py."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import helpers as H
import pwgt_ref as R
from test_gpu_features import DEV, Guarded, launched
from test_gpu_pwg_discriminator import share, t

pytestmark = pytest.mark.gpu
LENS, N = list(R.LENS), sum(R.LENS)


@pytest.fixture(scope="module")
def G():
    assert torch.cuda.is_available()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, pwg_generator

    _lib.load()
    return pwg_generator


@contextlib.contextmanager
def record():
    """-> {kernel name: its entry of the library's launch record (launches, ...)} for the launches inside"""
    from fcl_taco2_amd import _lib

    seen = {}
    _lib.prof_enable(True)
    try:
        yield seen
        torch.cuda.synchronize()
        seen.update(_lib.prof_collect())
    finally:
        _lib.prof_enable(False)


def torch_params(w):
    """a block's weights (pwgt_ref.block_weights) as the seven device tensors in BLOCK_PARAMS order"""
    return (t(w["conv"]), t(w["b_conv"]), t(w["aux"][:, :, None]), t(w["out"][:, :, None]), t(w["b_out"]), t(w["skip"][:, :, None]), t(w["b_skip"]))


def plan_of(G, R_, A, k, dils):
    plan = G.GeneratorPlan(DEV, layers=len(dils), stacks=1, residual_channels=R_, gate_channels=2 * R_, skip_channels=R_, aux_channels=A, kernel_size=k)
    plan.dilations = list(dils)  # (a block-level cell takes any dilation)
    return plan


def grads_np(G, plan, bufs):
    return [g.cpu().numpy().astype(np.float64) for g in G.unpack_dweights(plan, *[b.t.reshape(b.shape) for b in bufs])]


@pytest.mark.parametrize("first,last", [(True, False), (False, True)])
@pytest.mark.parametrize("d", R.DILATIONS)
@pytest.mark.parametrize("name", list(R.BLOCK_CONFIGS))
def test_block_launches_alone_vs_float64(G, name, d, first, last):
    """every launch of one block on the device's own inputs, to the first term of its bound: z, a, b; x_out and skips from the stored ab; dz from ab, dxo and
    ds; dx, dc and the seven parameter gradients from the stored dz"""
    import ctypes as C

    from fcl_taco2_amd import _lib, ops

    Rc, A, k = R.BLOCK_CONFIGS[name]
    w, inp = R.block_case(name, d)
    plan, maps = plan_of(G, Rc, A, k, [d]), G.Maps(LENS, DEV)
    pk = G.pack_weights([torch_params(w)])[0]
    x, c = Guarded(N, Rc).set(inp["x"]), Guarded(N, A).set(inp["c"])
    ab, x_out, skips, z_out = Guarded(N, 2 * Rc), Guarded(N, Rc), Guarded(N, Rc), Guarded(N, 2 * Rc)
    if not first:
        skips.set(inp["skips"])
    lib, st = _lib.load(), ops._stream()
    a = G._args(plan, maps, 0, first=first, last=last, x=x.t, c=c.t, w_gate=pk["w_gate"], b_gate=pk["b_gate"], w_out=pk["w_out"], b_out=pk["b_out"],
                ab=ab.t, x_out=x_out.t, skips=skips.t, z_out=z_out.t)
    with launched(*G.FWD_KERNELS):
        _lib.check(lib.fcl_pwt_block_fwd(C.byref(a), st))
    x64, c64 = inp["x"].astype(np.float64), inp["c"].astype(np.float64)
    gt = R.gate_forward(w, x64, c64, LENS, d)
    z_dev, ab_dev = z_out.np(), ab.np()
    a_dev, b_dev = ab_dev[:, :Rc], ab_dev[:, Rc:]
    # the device functions' own errors: the stored a, b against float64 tanh / sigmoid of the device's own float32 z
    f_t = float(np.abs(a_dev - np.tanh(z_dev[:, :Rc])).max() / R.U)
    f_s = float(np.abs(b_dev - 1.0 / (1.0 + np.exp(-z_dev[:, Rc:]))).max() / R.U)
    r_z = share(z_dev - gt["z"], gt["e_z"])
    r_a, r_b = share(a_dev - gt["a"], gt["e_a"]), share(b_dev - gt["b"], gt["e_b"])
    o = R.out_forward(w, x64, a_dev, b_dev, None if first else inp["skips"].astype(np.float64))
    r_x, r_s = share(x_out.np() - o["x_out"], o["e_x"]), share(skips.np() - o["skips"], o["e_s"])
    print("block %s d %d first %d last %d: function error tanh %.3f u, sigmoid %.3f u; shares of the bounds: z %.3g a %.3g b %.3g x_out %.3g skips %.3g"
          % (name, d, first, last, f_t, f_s, r_z, r_a, r_b, r_x, r_s))
    assert np.isfinite(ab_dev).all() and f_t <= R.E_T / R.U and f_s <= R.E_S / R.U
    assert max(r_z, r_a, r_b, r_x, r_s) <= 1.0
    # backward
    ds = Guarded(N, Rc).set(inp["ds"])
    dxo = None if last else Guarded(N, Rc).set(inp["dxo"])
    dz, dx, dc = Guarded(N, 2 * Rc), Guarded(N, Rc), Guarded(N, A)
    dc_before = None if last else np.float32(0.5) * inp["c"][::-1]
    if not last:
        dc.set(dc_before)
    dws, work = [Guarded(*s) for s in plan.dweight_shapes()], Guarded(plan.workspace_floats(N))
    a = G._args(plan, maps, 0, first=first, last=last, x=x.t, c=c.t, ab=ab.t, dxo=None if last else dxo.t, ds=ds.t, w_dz=pk["w_dz"], w_dx=pk["w_dx"],
                w_dc=pk["w_dc"], dz=dz.t, dx=dx.t, dc=dc.t, workspace=work.t)
    a.dw_gate, a.db_gate, a.dw_out, a.db_out = (b.t.data_ptr() for b in dws)
    a.workspace_bytes = work.n * 4
    with launched(G.DZ_KERNEL, G.DX_KERNEL, G.DC_KERNEL, *G.DW_KERNELS):
        _lib.check(lib.fcl_pwt_block_dx(C.byref(a), st))
        _lib.check(lib.fcl_pwt_block_dw(C.byref(a), st))
    dxo64, ds64 = None if last else inp["dxo"].astype(np.float64), inp["ds"].astype(np.float64)
    rb = R.block_backward(w, x64, c64, a_dev, b_dev, dxo64, ds64, LENS, d)
    r_dz = share(dz.np() - rb["dz"], rb["e_dz"])
    fz = R.from_dz(w, x64, c64, a_dev, b_dev, dxo64, ds64, dz.np(), LENS, d)
    r_dx = share(dx.np() - fz["dx"], fz["e_dx"])
    want_dc = fz["dc"] if last else dc_before.astype(np.float64) + fz["dc"]
    r_dc = share(dc.np() - want_dc, fz["e_dc"] + (0 if last else R.U * np.abs(want_dc)))
    got = grads_np(G, plan, dws)
    r_w = [share(g - wnt, e) for g, wnt, e in zip(got, fz["grads"], fz["e_grads"])]
    print("  backward: dz %.3g dx %.3g dc %.3g, parameter gradients %s" % (r_dz, r_dx, r_dc, np.round(r_w, 4)))
    assert all(np.isfinite(b.np()).all() for b in [dz, dx, dc] + dws)
    assert max([r_dz, r_dx, r_dc] + r_w) <= 1.0
    if last:
        assert not got[3].any() and not got[4].any()  # conv1x1_out of the last block: exactly zero
    assert all(b.intact() for b in [x, c, ab, x_out, skips, z_out, ds, dz, dx, dc, work] + dws + ([] if last else [dxo]))


class Stack(object):
    """one forward and one backward pass of a stack over a packed batch on guarded buffers"""

    def __init__(self, G, cfg, ws, x0, c, ds, lens=LENS, need_x=True, need_c=True, need_w=True):
        n, Rc, A, L = sum(lens), cfg["residual_channels"], cfg["aux_channels"], cfg["layers"]
        self.plan = plan = plan_of(G, Rc, A, cfg["kernel_size"], R.dilations(cfg))
        maps = G.Maps(lens, DEV)
        pk = G.pack_weights([torch_params(w) for w in ws])
        sx, sab = plan.kept_shapes(n)
        self.xs, self.abs = [Guarded(*s) for s in sx], [Guarded(*s) for s in sab]
        self.xs[0].set(x0)
        cb, self.skips = Guarded(n, A).set(c), Guarded(n, Rc)
        with launched(*G.FWD_KERNELS):
            G.launch_forward(plan, maps, cb.t, pk, [b.t for b in self.xs], [b.t for b in self.abs], self.skips.t)
        dsb = Guarded(n, Rc).set(ds)
        self.dx0, self.dc = Guarded(n, Rc) if need_x else None, Guarded(n, A) if need_c else None
        self.dws = [[Guarded(*s) for s in plan.dweight_shapes()] for _ in range(L)] if need_w else None
        grads, dz, work = [Guarded(n, Rc), Guarded(n, Rc)], Guarded(n, 2 * Rc), Guarded(plan.workspace_floats(n))
        names = (G.DZ_KERNEL,) + ((G.DX_KERNEL,) if need_x or L > 1 else ()) + ((G.DC_KERNEL,) if need_c else ()) + (G.DW_KERNELS if need_w else ())
        with launched(*names):
            G.launch_backward(plan, maps, dsb.t, cb.t, pk, [b.t for b in self.xs], [b.t for b in self.abs], None if self.dx0 is None else self.dx0.t,
                              None if self.dc is None else self.dc.t, None if self.dws is None else [[b.t for b in row] for row in self.dws],
                              [g.t for g in grads], dz.t, work.t)
        held = self.xs + self.abs + [cb, self.skips, dsb, dz, work] + grads + [b for b in (self.dx0, self.dc) if b is not None]
        assert all(b.intact() for b in held + [b for row in (self.dws or []) for b in row])

    def grads(self, G, l):
        return grads_np(G, self.plan, self.dws[l])

    def bits(self):
        return [b.bits() for b in [self.skips, self.dx0, self.dc] + [b for row in self.dws for b in row]]


@functools.lru_cache(maxsize=None)
def stack_reference(which):
    cfg = dict(H.pwg_cfg(), upsample_scales=(2,)) if which == "v1" else R.SMALL_STACK
    sd, ws, x0, c, ds = R.stack_case(cfg, 31 if which == "small" else 37)
    dils = R.dilations(cfg)
    fw = R.stack_forward(ws, x0, c, R.LENS, dils, running=which == "small")
    bw = R.stack_backward(ws, fw, c, ds, R.LENS, dils, running=which == "small")
    return cfg, ws, x0, c, ds, dils, fw, bw


def test_small_stack_vs_float64_to_the_running_bound(G):
    """4 layers, 2 stacks, R 16: device forward then device backward against float64 forward then float64 backward"""
    cfg, ws, x0, c, ds, dils, fw, bw = stack_reference("small")
    run = Stack(G, cfg, ws, x0, c, ds)
    r = [share(run.skips.np() - fw["skips"], fw["e_s"]), share(run.dx0.np() - bw["dx0"], bw["e_dx0"]), share(run.dc.np() - bw["dc"], bw["e_dc"])]
    for l in range(cfg["layers"]):
        blk = fw["blocks"][l]
        r.append(share(run.xs[l + 1].np() - blk["x_out"], blk["e_xout"]))
        r += [share(g - wnt, e) for g, wnt, e in zip(run.grads(G, l), bw["grads"][l], bw["e_grads"][l])]
    print("small stack: worst share of the running bound %.3g" % max(r))
    assert max(r) <= 1.0


def test_v1_stack_vs_float64_by_the_error_model(G):
    """30 blocks, R 64, A 80 on the 1313 samples: every block's tap and every gradient within 4 x max(model, 2^-15 max |value|), the model being the float32
    numpy evaluation's own error against float64"""
    cfg, ws, x0, c, ds, dils, fw, bw = stack_reference("v1")
    with np.errstate(over="ignore"):
        f32 = R.stack_forward(ws, x0, c, R.LENS, dils, dt=np.float32, running=False)
        b32 = R.stack_backward(ws, f32, c, ds, R.LENS, dils, running=False, dt=np.float32)
    run = Stack(G, cfg, ws, x0, c, ds)
    worst = 0.0

    def check(what, got, model, want):
        nonlocal worst
        err, allow = np.abs(got - want).max(), 4 * max(np.abs(model.astype(np.float64) - want).max(), 2.0 ** -15 * np.abs(want).max())
        worst = max(worst, err / allow) if allow > 0 else worst
        assert np.isfinite(got).all() and err <= allow, (what, err, allow)

    check("skips", run.skips.np(), f32["skips"], fw["skips"])
    check("dx0", run.dx0.np(), b32["dx0"], bw["dx0"])
    check("dc", run.dc.np(), b32["dc"], bw["dc"])
    for l in range(cfg["layers"]):
        check("tap %d" % l, run.xs[l + 1].np(), f32["blocks"][l]["x_out"], fw["blocks"][l]["x_out"])
        for i, (g, m, wnt) in enumerate(zip(run.grads(G, l), b32["grads"][l], bw["grads"][l])):
            check("block %d %s" % (l, G.BLOCK_PARAMS[i]), g, m, wnt)
    last = run.grads(G, cfg["layers"] - 1)
    assert not last[3].any() and not last[4].any()
    print("v1 stack: worst share of 4 x max(model, 2^-15 peak) %.3g" % worst)


def stack_autograd(G, cfg, ws, x0, c, ds, lens, need=(True, True, True)):
    plan = plan_of(G, cfg["residual_channels"], cfg["aux_channels"], cfg["kernel_size"], R.dilations(cfg))
    xt, ct = t(x0).requires_grad_(need[0]), t(c).requires_grad_(need[1])
    blocks = [[p.requires_grad_(need[2]) for p in torch_params(w)] for w in ws]
    sk = G.residual_stack(plan, G.Maps(lens, DEV), xt, ct, blocks)
    sk.backward(t(ds))
    return sk.detach(), xt.grad, ct.grad, [p.grad for b in blocks for p in b]


def test_a_batch_is_its_per_utterance_runs_and_two_runs_agree_bit_for_bit(G):
    cfg, ws, x0, c, ds, dils, fw, bw = stack_reference("small")
    sk, dx, dc, dw = stack_autograd(G, cfg, ws, x0, c, ds, LENS)
    sk2, dx2, dc2, dw2 = stack_autograd(G, cfg, ws, x0, c, ds, LENS)
    assert torch.equal(sk, sk2) and torch.equal(dx, dx2) and torch.equal(dc, dc2) and all(torch.equal(a, b) for a, b in zip(dw, dw2))
    off = 0
    for n in LENS:
        s = slice(off, off + n)
        sk1, dx1, dc1, _ = stack_autograd(G, cfg, ws, x0[s], c[s], ds[s], [n])
        assert torch.equal(sk[s], sk1) and torch.equal(dx[s], dx1) and torch.equal(dc[s], dc1), n
        off += n
    # another utterance 2 leaves the others' outputs and gradients as they are
    lo, hi = sum(LENS[:2]), sum(LENS[:3])
    x0b, cb, dsb = x0.copy(), c.copy(), ds.copy()
    x0b[lo:hi], cb[lo:hi], dsb[lo:hi] = -x0[lo:hi], c[lo:hi][::-1], 2 * ds[lo:hi]
    sk3, dx3, dc3, _ = stack_autograd(G, cfg, ws, x0b, cb, dsb, LENS)
    keep = np.r_[0:lo, hi:N]
    assert not torch.equal(sk3[lo:hi], sk[lo:hi])
    assert torch.equal(sk3[keep], sk[keep]) and torch.equal(dx3[keep], dx[keep]) and torch.equal(dc3[keep], dc[keep])


def test_launch_omissions(G):
    """weight-gradient kernels only when a weight asks, aux-backward only when c asks, block 0's conv-backward only when x_0 asks"""
    cfg, ws, x0, c, ds, dils, fw, bw = stack_reference("small")
    L = cfg["layers"]
    with record() as all_:
        stack_autograd(G, cfg, ws, x0, c, ds, LENS)
    assert all_[G.DX_KERNEL]["launches"] == L and all_[G.DC_KERNEL]["launches"] == L and all_["pwt_dw_reduce_kernel"]["launches"] == 2 * L
    with record() as no_w:
        _, dx, dc, dw = stack_autograd(G, cfg, ws, x0, c, ds, LENS, (True, True, False))
    assert not any(k in no_w for k in G.DW_KERNELS) and all(g is None for g in dw) and dx is not None and dc is not None
    with record() as no_c:
        _, dx, dc, dw = stack_autograd(G, cfg, ws, x0, c, ds, LENS, (True, False, True))
    assert G.DC_KERNEL not in no_c and dc is None and no_c[G.DX_KERNEL]["launches"] == L
    with record() as no_x:
        _, dx, dc, dw = stack_autograd(G, cfg, ws, x0, c, ds, LENS, (False, True, True))
    assert no_x[G.DX_KERNEL]["launches"] == L - 1 and dx is None and no_x[G.DZ_KERNEL]["launches"] == L


# ---- the module
def module_of(G, sd, cfg, **kw):
    full = H.pwg_cfg(cfg)
    m = G.TrainableParallelWaveGANGenerator(layers=full["layers"], stacks=full["stacks"], residual_channels=full["residual_channels"],
                                            gate_channels=full["gate_channels"], skip_channels=full["skip_channels"], aux_channels=full["aux_channels"],
                                            aux_context_window=full["aux_context_window"], kernel_size=full["kernel_size"],
                                            upsample_params={"upsample_scales": list(full["upsample_scales"])}, **kw).to(DEV)
    if sd is not None:
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m, full


def padded_inputs(full, mels, noise):
    """the module's batch form: z [B, 1, T], c [B, A, frames + 2 ctx] with every utterance's replicate padding, zero behind it"""
    hop, ctx = int(np.prod(full["upsample_scales"])), full["aux_context_window"]
    F_ = max(m.shape[0] for m in mels)
    z, c = np.zeros((len(mels), 1, F_ * hop), np.float32), np.zeros((len(mels), full["aux_channels"], F_ + 2 * ctx), np.float32)
    for i, (m, nz) in enumerate(zip(mels, noise)):
        z[i, 0, : len(nz)] = nz
        c[i, :, : m.shape[0] + 2 * ctx] = m[np.clip(np.arange(-ctx, m.shape[0] + ctx), 0, m.shape[0] - 1)].T
    return t(z), t(c)


def test_module_forward_is_the_inference_generators(G):
    """hop 6, frames (1, 5, 22, 184): the module's forward against vocoder.ParallelWaveGANGenerator.synthesize on the same weights and noise, within that
    path's 1e-3 x peak; the module's state_dict goes into PWGPlan as it is"""
    from fcl_taco2_amd import vocoder

    lens = [1, 5, 22, 184]
    sd, mels, noise = H.pwg_generator_inputs(41, lens, H.PWG_SMALL_CFG)
    m, full = module_of(G, sd, H.PWG_SMALL_CFG, use_weight_norm=False)
    want = vocoder.ParallelWaveGANGenerator(vocoder.PWGPlan(m.state_dict(), DEV, H.PWG_SMALL_CFG)).synthesize(mels, noise=noise)
    z, c = padded_inputs(full, mels, noise)
    with torch.no_grad(), launched(*G.FWD_KERNELS):
        got = m(z, c, lens=lens)
    assert got.shape == z.shape
    for i, w in enumerate(want):
        n = w.numel()
        err, peak = float((got[i, 0, :n] - w.reshape(-1)).abs().max()), float(w.abs().max())
        print("module vs inference generator, %d frames: %.3g of the peak" % (lens[i], err / peak))
        assert err <= 1e-3 * peak and not got[i, 0, n:].any()


def test_padding_gets_exactly_zero_gradient_and_weight_norm_loads_bit_identically(G):
    lens = [3, 1, 7]
    cfg = dict(R.SMALL_STACK, upsample_scales=(2, 3))
    sd, mels, noise = H.pwg_generator_inputs(43, lens, cfg)
    m, full = module_of(G, sd, cfg, use_weight_norm=False)
    z, c = padded_inputs(full, mels, noise)
    z.requires_grad_(True), c.requires_grad_(True)
    y = m(z, c, lens=lens)
    (y * torch.randn_like(y)).sum().backward()
    hop, ctx = m.hop, m.ctx
    for i, n in enumerate(lens):
        assert z.grad[i, 0, : n * hop].abs().sum() > 0 and not z.grad[i, 0, n * hop :].any() and not c.grad[i, :, n + 2 * ctx :].any()
        assert not y[i, 0, n * hop :].any()
    # a weight-norm state dict into a plain module, and the module's own weight-norm form
    wn, _ = module_of(G, sd, cfg, use_weight_norm=True)
    again, _ = module_of(G, None, cfg, use_weight_norm=False)
    again.load_state_dict(wn.state_dict())
    with torch.no_grad():
        a, b = wn(z, c, lens=lens), again(z, c, lens=lens)
    assert torch.equal(a, b)


def test_one_whole_parallel_wavegan_step(G):
    """INTEGRATION.md's example: generator, discriminator, STFT loss, two Adam optimisers; every parameter but the last block's conv1x1_out gets a finite,
    non-zero gradient and changes"""
    from fcl_taco2_amd.pwg_discriminator import ParallelWaveGANDiscriminator, discriminator_adversarial_loss, generator_adversarial_loss
    from fcl_taco2_amd.stft_loss import MultiResolutionSTFTLoss

    torch.manual_seed(5)
    gen = G.TrainableParallelWaveGANGenerator(layers=4, stacks=2, residual_channels=16, gate_channels=32, skip_channels=16, aux_channels=16,
                                              upsample_params={"upsample_scales": [4, 4]}).to(DEV)
    disc = ParallelWaveGANDiscriminator(layers=4, conv_channels=16).to(DEV)
    criterion = MultiResolutionSTFTLoss(DEV)
    opt_g, opt_d = torch.optim.Adam(gen.parameters(), 1e-3), torch.optim.Adam(disc.parameters(), 1e-3)
    frames, B = 80, 2
    c = torch.randn(B, 16, frames + 2 * gen.ctx, device=DEV)
    wav = 0.3 * torch.randn(B, 1, frames * gen.hop, device=DEV)
    before = {k: v.detach().clone() for k, v in gen.named_parameters()}
    d_before = {k: v.detach().clone() for k, v in disc.named_parameters()}
    with launched(*(G.FWD_KERNELS + (G.DZ_KERNEL, G.DX_KERNEL, G.DC_KERNEL) + G.DW_KERNELS)):
        fake = gen(torch.randn_like(wav), c)
        real_loss, fake_loss = discriminator_adversarial_loss(disc(wav), disc(fake.detach()))
        opt_d.zero_grad()
        (real_loss + fake_loss).backward()
        opt_d.step()
        sc, mag = criterion(fake, wav)
        adv = generator_adversarial_loss(disc(fake))
        opt_g.zero_grad()
        (sc + mag + 4.0 * adv).backward()
        opt_g.step()
    dead = "conv_layers.3.conv1x1_out."
    for k, p in gen.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        if k.startswith(dead):
            assert not p.grad.any() and torch.equal(p.detach(), before[k]), k
        else:
            assert p.grad.abs().sum() > 0 and not torch.equal(p.detach(), before[k]), k
    assert all(not torch.equal(p.detach(), d_before[k]) for k, p in disc.named_parameters())
