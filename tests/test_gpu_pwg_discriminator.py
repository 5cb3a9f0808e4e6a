"""The pwd_* kernels of csrc/pwg_disc.hip and the autograd module on them against the float64 statement of tests/pwgd_ref.py.  Every buffer
a kernel writes sits between guard zones filled with a NaN bit pattern, which must survive; every kernel test reads the library's launch record and fails if
its kernels did not run.  The cases, their inputs, their bounds and the recorded end-to-end seeds are built and checked in pwgd_ref.py /
test_pwg_discriminator_cpu.py."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import pwgd_ref as R
from test_gpu_features import DEV, Guarded, launched

pytestmark = pytest.mark.gpu
FWD_KERNELS = ("pwd_expand_kernel<fwd>", "pwd_conv_kernel<fwd>", "pwd_reduce_kernel<fwd>")
DX_KERNELS = ("pwd_expand_kernel<dx>", "pwd_conv_kernel<dx>")
FIRST_DX = "pwd_reduce_kernel<dx>"
DW_KERNELS = ("pwd_dw_kernel", "pwd_dw_small_kernel<first>", "pwd_dw_small_kernel<last>", "pwd_dw_reduce_kernel")


@pytest.fixture(scope="module")
def P():
    assert torch.cuda.is_available()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, pwg_discriminator

    _lib.load()
    return pwg_discriminator


@functools.lru_cache(maxsize=None)
def reference(name):
    """computed once per case and shared, read-only"""
    cfg, lens = R.CONFIGS[name], dict(R.CASES)[name]
    ws, xs, ds = R.weights(cfg, 0), R.signals(lens, 0), R.given_gradient(lens, 0)
    fw = R.forward(cfg, ws, xs)
    for a in xs + ds + [v for r in fw for key in r for v in r[key]] + [w for W, b in ws for w in (W, b) if w is not None]:
        a.setflags(write=False)
    return cfg, ws, xs, ds, fw


@contextlib.contextmanager
def record():
    """-> the names of the kernels launched inside (the library's own launch record)"""
    from fcl_taco2_amd import _lib

    seen = set()
    _lib.prof_enable(True)
    try:
        yield seen
        torch.cuda.synchronize()
        seen.update(_lib.prof_collect())
    finally:
        _lib.prof_enable(False)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def split(a, lens):
    return np.split(a, np.cumsum(lens)[:-1])


def share(diff, bound):
    """the worst |diff| / bound; a bound of exactly zero (a dead ReLU channel) admits exactly zero"""
    return float(np.max(np.abs(diff) / np.maximum(bound, 1e-300)))


class Run(object):
    """one forward pass (and, given dscore, one backward pass) of a packed batch on guarded buffers"""

    def __init__(self, P, cfg, ws, xs, ds=None, need_x=True, need_w=True):
        self.lens = lens = [len(x) for x in xs]
        n = sum(lens)
        self.plan = plan = P.DiscriminatorPlan(DEV, **cfg)
        maps = P.Maps(lens, DEV)
        packed = P.pack_weights([t(W) for W, _ in ws], [None if b is None else t(b) for _, b in ws])
        x = Guarded(n).set(np.concatenate(xs))
        self.acts = [Guarded(*s) for s in plan.act_shapes(n)]
        held = [x] + self.acts
        with launched(*FWD_KERNELS):
            P.launch_forward(plan, maps, x.t, packed, [a.t for a in self.acts])
        if ds is not None:
            dscore = Guarded(n).set(np.concatenate(ds))
            self.gx = Guarded(n) if need_x else None
            self.dws = [(Guarded(*sw), Guarded(*sb) if cfg["bias"] else None) for sw, sb in plan.dweight_shapes()] if need_w else None
            grads, work = [Guarded(plan.grad_floats(n)), Guarded(plan.grad_floats(n))], Guarded(plan.workspace_floats(n))
            with launched(*(DX_KERNELS + ((FIRST_DX,) if need_x else ()) + (DW_KERNELS if need_w else ()))):
                P.launch_backward(plan, maps, dscore.t, packed, [a.t for a in self.acts], None if self.gx is None else self.gx.t,
                                  None if self.dws is None else [(dw.t, None if db is None else db.t) for dw, db in self.dws], x=x.t,
                                  grads=[g.t for g in grads], workspace=work.t)
            held += [dscore, work] + grads + ([self.gx] if need_x else []) + ([b for pair in (self.dws or []) for b in pair if b is not None])
        assert all(b.intact() for b in held)

    def h(self, u, l):
        """utterance u's activation of layer l, [T, C] float64 (the scores [T, 1])"""
        return split(self.acts[l].np().reshape(sum(self.lens), -1), self.lens)[u]

    def dw(self, l):
        """layer l's weight gradient in torch's layout [cout, cin, k], float64"""
        return self.dws[l][0].np().transpose(2, 1, 0)

    def weight_bits(self):
        return [b.bits() for pair in self.dws for b in pair if b is not None]


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_forward_vs_float64(P, name):
    """every layer's h_l and the scores of the packed batch (1, 5, 130, 257, 77 samples) within the running bounds, and every layer alone, on the
    device's own input, within the first term of its bound (a deep layer held as tightly as the first)"""
    cfg, ws, xs, _, fw = reference(name)
    run = Run(P, cfg, ws, xs)
    worst, local = 0.0, 0.0
    for u in range(len(xs)):
        for l in range(cfg["layers"]):
            got = run.h(u, l)
            assert np.isfinite(got).all()
            worst = max(worst, share(got - fw[u]["h"][l], fw[u]["e"][l]))
            want, e = R.layer_forward(cfg, ws, l, xs[u][:, None] if l == 0 else run.h(u, l - 1))
            local = max(local, share(got - want, e))
    print("discriminator %s forward: worst share of the running bound %.3g, of a layer's own bound %.3g" % (name, worst, local))
    assert worst <= 1.0 and local <= 1.0


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_backward_on_the_devices_own_activations_vs_float64(P, name):
    """on the stored activations the device's forward produced and a given dscore: the waveform gradient per utterance in norm, every dW and db per
    element, within the bounds"""
    cfg, ws, xs, ds, _ = reference(name)
    run = Run(P, cfg, ws, xs, ds)
    hs = [[run.h(u, l) for l in range(cfg["layers"] - 1)] for u in range(len(xs))]
    ref = R.backward(cfg, ws, xs, hs, ds)
    r_x = [share(np.linalg.norm(a - b), np.linalg.norm(e)) for a, b, e in zip(split(run.gx.np(), run.lens), ref["gx"], ref["gx_e"])]
    r_w = [share(run.dw(l) - ref["dw"][l], ref["dw_e"][l]) for l in range(cfg["layers"])]
    r_b = [share(run.dws[l][1].np() - ref["db"][l], ref["db_e"][l]) for l in range(cfg["layers"])] if cfg["bias"] else [0.0]
    print("discriminator %s backward: worst share of the bound: gx %s, dW %s, db %s" % (name, np.round(r_x, 4), np.round(r_w, 4), np.round(r_b, 4)))
    assert np.isfinite(run.gx.np()).all() and max(r_x) <= 1.0 and max(r_w) <= 1.0 and max(r_b) <= 1.0


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_batch_equals_per_utterance_runs_and_two_runs_give_the_same_bits(P, name):
    cfg, ws, xs, ds, _ = reference(name)
    run, again = Run(P, cfg, ws, xs, ds), Run(P, cfg, ws, xs, ds)
    assert run.weight_bits() == again.weight_bits() and run.gx.bits() == again.gx.bits()
    scores, gx = split(run.acts[-1].t.cpu().numpy(), run.lens), split(run.gx.t.cpu().numpy(), run.lens)
    for u in range(len(xs)):
        one = Run(P, cfg, ws, [xs[u]], [ds[u]], need_w=False)
        assert one.acts[-1].bits() == scores[u].tobytes() and one.gx.bits() == gx[u].tobytes(), u


def test_changing_one_utterance_leaves_the_others_bit_identical(P):
    cfg, ws, xs, ds, _ = reference("default")
    other = list(xs)
    other[2] = R.signals([len(xs[2])], 9)[0]
    a, b = Run(P, cfg, ws, xs, ds, need_w=False), Run(P, cfg, ws, other, ds, need_w=False)
    for l in range(cfg["layers"]):
        for u in range(len(xs)):
            same = a.h(u, l).tobytes() == b.h(u, l).tobytes()
            assert same == (u != 2), (l, u)
    for u, (g, h) in enumerate(zip(split(a.gx.np(), a.lens), split(b.gx.np(), b.lens))):
        assert (g.tobytes() == h.tobytes()) == (u != 2), u


# ---- the module ----------------------------------------------------------------------------------------------------------------------------------------

def module_of(P, cfg, ws=None, **kw):
    m = P.ParallelWaveGANDiscriminator(kernel_size=cfg["kernel_size"], layers=cfg["layers"], conv_channels=cfg["conv_channels"],
                                       dilation_factor=cfg["dilation_factor"], negative_slope=cfg["negative_slope"], bias=cfg["bias"], **kw).to(DEV)
    if ws is not None:
        with torch.no_grad():
            for c, (W, b) in zip(m.convs(), ws):
                if "weight" in c._parameters:
                    c.weight.copy_(t(W))
                else:
                    c.weight_v.copy_(t(W)), c.weight_g.copy_(torch.linalg.vector_norm(t(W), dim=(1, 2), keepdim=True))
                if b is not None:
                    c.bias.copy_(t(b))
    return m


def test_module_input_forms_agree_and_padding_gets_zero_gradient(P):
    cfg, ws, _, _, _ = reference("c16k5f2")
    m = module_of(P, cfg, ws, use_weight_norm=False)
    lens = [40, 64, 1]
    xs = R.signals(lens, 5)
    T = 64
    eq = t(np.stack(R.signals([T, T], 6)))
    with launched(*FWD_KERNELS):
        p2 = m(eq)
    assert p2.shape == (2, 1, T) and torch.equal(m(eq[:, None, :]), p2) and torch.equal(m(eq.reshape(-1), lens=[T, T]), p2.reshape(-1))
    x = t(np.concatenate(xs)).requires_grad_(True)
    p = m(x, lens=lens)
    assert p.shape == (sum(lens),)
    g = t(np.concatenate(R.given_gradient(lens, 5)))
    p.backward(g)
    xp = t(np.stack([np.concatenate([v, np.full(T - len(v), 0.25)]) for v in xs])).requires_grad_(True)  # the padding would matter if it were read
    pp = m(xp, lens=lens)
    assert torch.equal(pp, p)
    pp.backward(g)
    for b, n in enumerate(lens):
        assert torch.equal(xp.grad[b, :n], x.grad[sum(lens[:b]) : sum(lens[:b]) + n]) and not bool(xp.grad[b, n:].any())
    keep = m._maps
    m(x.detach(), lens=lens)
    assert m._maps is keep  # the maps are kept for the next batch of the same lengths
    with pytest.raises(ValueError, match="at least one sample"):
        m(torch.zeros(5, device=DEV), lens=[5, 0])


def test_module_omits_the_gradients_nobody_asks_for(P):
    cfg, ws, xs, _, _ = reference("c16k5f2")
    m = module_of(P, cfg, ws)
    x = t(np.concatenate(xs))
    lens = [len(v) for v in xs]
    with record() as seen:  # the generator's update: the weights are frozen
        for p in m.parameters():
            p.requires_grad_(False)
        xr = x.clone().requires_grad_(True)
        P.generator_adversarial_loss(m(xr, lens=lens)).backward()
    assert FIRST_DX in seen and set(DX_KERNELS) <= seen and not [k for k in seen if k.startswith("pwd_dw")], sorted(seen)
    assert xr.grad is not None and all(p.grad is None for p in m.parameters())
    with record() as seen:  # the discriminator's update: the fake is detached
        for p in m.parameters():
            p.requires_grad_(True)
        sum(P.discriminator_adversarial_loss(m(x, lens=lens), m(x.detach() * 0.5, lens=lens))).backward()
    assert set(DW_KERNELS) <= seen and FIRST_DX not in seen, sorted(seen)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    with record() as seen:
        with torch.no_grad():
            m(x, lens=lens)
    assert set(FWD_KERNELS) == seen


def e2e_module(P, ref):
    m = module_of(P, ref["cfg"])
    with torch.no_grad():
        for c, v, g, b in zip(m.convs(), ref["vs"], ref["gs"], ref["bs"]):
            c.weight_v.copy_(t(v)), c.weight_g.copy_(t(g).reshape(-1, 1, 1)), c.bias.copy_(t(b))
    return m


def test_end_to_end_generator_loss_gradient_vs_float64(P):
    """device forward then device backward of generator_adversarial_loss on a case whose reference finds no pre-activation within its bound of zero:
    the waveform gradient per utterance within the propagated bound"""
    ref = R.e2e_reference(R.SEEDS["generator"], "generator")
    assert ref["share"] == 1.0
    m = e2e_module(P, ref)
    for p in m.parameters():
        p.requires_grad_(False)
    lens = [len(v) for v in ref["fake"]]
    x = t(np.concatenate(ref["fake"])).requires_grad_(True)
    loss = P.generator_adversarial_loss(m(x, lens=lens))
    loss.backward()
    r = [share(np.linalg.norm(a - b), np.linalg.norm(e)) for a, b, e in zip(split(x.grad.cpu().numpy().astype(np.float64), lens), ref["gx"], ref["gx_e"])]
    print("end to end, generator: loss %.6f (float64 %.6f), gradient share of the bound %s" % (loss.item(), ref["value"], r))
    assert abs(loss.item() - ref["value"]) <= 1e-3 * abs(ref["value"]) and max(r) <= 1.0


def test_end_to_end_discriminator_loss_gradients_vs_float64(P):
    """discriminator_adversarial_loss on a real and a detached fake batch: the gradients of weight_g, weight_v and the biases within the propagated bounds"""
    ref = R.e2e_reference(R.SEEDS["discriminator"], "discriminator")
    assert ref["share"] == 1.0
    m = e2e_module(P, ref)
    lens = [len(v) for v in ref["fake"]]
    fake = t(np.concatenate(ref["fake"])).requires_grad_(True)
    r_loss, f_loss = P.discriminator_adversarial_loss(m(t(np.concatenate(ref["real"])), lens=lens), m(fake.detach(), lens=lens))
    (r_loss + f_loss).backward()
    assert fake.grad is None
    shares = []
    for l, c in enumerate(m.convs()):
        f64 = lambda p: p.grad.cpu().numpy().astype(np.float64)
        shares.append((share(f64(c.weight_g).reshape(-1) - ref["dg"][l], ref["dg_e"][l]), share(f64(c.weight_v) - ref["dv"][l], ref["dv_e"][l]),
                       share(f64(c.bias) - ref["db"][l], ref["db_e"][l])))
    print("end to end, discriminator: loss %.6f (float64 %.6f), worst share of the bound per layer (g, v, bias) %s" % (
        (r_loss + f_loss).item(), ref["value"], np.round(shares, 6).tolist()))
    assert abs((r_loss + f_loss).item() - ref["value"]) <= 1e-3 * abs(ref["value"]) and np.max(shares) <= 1.0


def test_weight_norm_state_dict_loads_into_a_plain_module_with_the_same_scores(P):
    cfg = R.CONFIGS["c16k5f2"]
    a = module_of(P, cfg)
    with torch.no_grad():
        for c in a.convs():
            c.weight_g.mul_(torch.rand_like(c.weight_g) + 0.5), c.bias.normal_(0, 0.1)
    b = module_of(P, cfg, use_weight_norm=False)
    b.load_state_dict({"model": {"discriminator": a.state_dict()}})
    x = t(np.stack(R.signals([300, 300], 3)))
    with torch.no_grad():
        pa, pb = a(x), b(x)
        assert torch.equal(pa, pb) and bool(pa.abs().sum() > 0)
        a.remove_weight_norm()
        assert torch.equal(a(x), pb)


def test_one_step_of_the_integration_example(P):
    """INTEGRATION.md "Training a generator against it", the full Parallel WaveGAN step on a two-layer torch toy generator: the discriminator's update on
    the detached fake, then the generator's update with stft + 4 adv"""
    from fcl_taco2_amd.stft_loss import MultiResolutionSTFTLoss

    torch.manual_seed(0)
    generator = torch.nn.Sequential(torch.nn.Conv1d(1, 8, 5, padding=2), torch.nn.Tanh(), torch.nn.Conv1d(8, 1, 5, padding=2)).to(DEV)
    disc = P.ParallelWaveGANDiscriminator().to(DEV)
    criterion = MultiResolutionSTFTLoss(DEV)
    opt_g, opt_d = torch.optim.Adam(generator.parameters(), 1e-4), torch.optim.Adam(disc.parameters(), 5e-5)
    before = [p.detach().clone() for p in list(generator.parameters()) + list(disc.parameters())]
    wav, z = t(np.stack(R.signals([2048, 2048], 1)))[:, None, :], torch.randn(2, 1, 2048, device=DEV)
    fake = generator(z)
    real_loss, fake_loss = P.discriminator_adversarial_loss(disc(wav), disc(fake.detach()))
    opt_d.zero_grad()
    (real_loss + fake_loss).backward()
    opt_d.step()
    sc, mag = criterion(fake, wav)
    adv = P.generator_adversarial_loss(disc(fake))
    opt_g.zero_grad()
    (sc + mag + 4.0 * adv).backward()
    opt_g.step()
    vals = [v.item() for v in (real_loss, fake_loss, sc, mag, adv)]
    print("one PWG step: real %.4f fake %.4f sc %.4f mag %.4f adv %.4f" % tuple(vals))
    assert np.isfinite(vals).all()
    after = list(generator.parameters()) + list(disc.parameters())
    assert all(bool(torch.isfinite(p).all()) and not torch.equal(p, q) for p, q in zip(after, before))
