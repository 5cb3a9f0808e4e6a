"""The pwe_* kernels of csrc/pwg_ends.hip and the module's HIP ends against the float64 statement of tests/pwge_ref.py.  Every buffer a
kernel touches sits between guard zones filled with a NaN bit pattern, which must survive; every output starts as NaN; every case reads the library's
launch record and fails if its kernels did not run.  The cases, their inputs and their bounds are built and checked in pwge_ref.py /
test_pwg_ends_cpu.py.

The gradients of the stage inputs live in the workspace, in two buffers used in turn, so after a pass the two earliest stages' (du_0, du_1) are still
there: with two scales that is every du.  With four, test_each_stage_backward_alone_at_every_depth runs every stage's backward launches on their own (a
one-scale plan at that stage's row counts, on the statement's u_k and du_{k+1}), so that every du and every dh is held to its first term and to batch =
utterances alone."""
import functools

import numpy as np
import pytest
import torch

import pwge_ref as E
from test_gpu_features import DEV, Guarded, launched
from test_gpu_pwg_discriminator import t
from test_gpu_pwg_generator import module_of, padded_inputs, record

pytestmark = pytest.mark.gpu
f8 = lambda a: np.asarray(a, np.float64)


@pytest.fixture(scope="module")
def G():
    assert torch.cuda.is_available()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, pwg_generator

    _lib.load()
    return pwg_generator


def plan_of(G, Rc, A, ctx, scales):
    return G.GeneratorPlan(DEV, layers=E.LAYERS, stacks=1, residual_channels=Rc, gate_channels=2 * Rc, skip_channels=Rc, aux_channels=A,
                           aux_context_window=ctx, upsample_params={"upsample_scales": list(scales)})


def packed(G, w):
    Rc = len(w["w0"])
    return (G.pack_in_weights(t(w["win"]), [t(h.reshape(1, 1, 1, -1)) for h in w["hs"]], t(w["w0"].reshape(Rc, 1, 1)), t(w["b0"])),
            G.pack_out_weights(t(w["W1"].reshape(Rc, Rc, 1)), t(w["b1"]), t(w["w3"].reshape(1, Rc, 1)), t(w["b3"])))


class Run(object):
    """both ends, forward and backward, of one packed batch on guarded buffers (the two ends are independent: each has its own inputs)"""

    def __init__(self, G, w, inp, frames, scales, ctx, need_w=True, need_c=True, need_z=True):
        A, Rc, hop = w["win"].shape[0], len(w["w0"]), int(np.prod(scales))
        self.plan = plan = plan_of(G, Rc, A, ctx, scales)
        self.maps = maps = G.FrameMaps(frames, hop, DEV)
        n, F, ns = maps.samples, maps.n_frames, len(scales)
        pin, pout = packed(G, w)
        new = lambda *s: Guarded(*s)
        c, z = new(F + 2 * ctx * len(frames), A).set(inp["c"]), new(n).set(inp["z"])
        self.us, self.cu, self.x0 = [new(r, A) for r in plan.stage_rows(F)], new(n, A), new(n, Rc)
        with launched(*G.IN_FWD_KERNELS):
            G.launch_in_forward(plan, maps, z.t, c.t, pin, [u.t for u in self.us], self.cu.t, self.x0.t)
        dcu, dx0 = new(n, A).set(inp["dcu"]), new(n, Rc).set(inp["dx0"])
        self.din = (new((2 * ctx + 1) * A, A), [new(2 * s + 1) for s in scales], new(Rc), new(Rc)) if need_w else None
        self.dc, self.dz = new(*c.shape) if need_c else None, new(n) if need_z else None
        self.work = work = new(plan.ends_workspace_floats(maps))
        with record() as self.seen_in:
            G.launch_in_backward(plan, maps, dcu.t, dx0.t, z.t, c.t, pin, [u.t for u in self.us], None if self.din is None else
                                 (self.din[0].t, [b.t for b in self.din[1]], self.din[2].t, self.din[3].t), None if self.dc is None else self.dc.t,
                                 None if self.dz is None else self.dz.t, work.t)
        S, dwav = new(n, Rc).set(inp["S"]), new(n).set(inp["dwav"])
        self.y1, self.wav, self.dy1, self.ds = new(n, Rc), new(n), new(n, Rc), new(n, Rc)
        with launched(G.OUT_FWD_KERNEL):
            G.launch_out_forward(plan, maps, S.t, pout, self.y1.t, self.wav.t)
        self.dout = (new(Rc, Rc), new(Rc), new(Rc), new(1)) if need_w else None
        work2 = new(plan.ends_workspace_floats(maps))
        with record() as self.seen_out:
            G.launch_out_backward(plan, maps, dwav.t, S.t, self.y1.t, pout, self.dy1.t, self.ds.t, None if self.dout is None else [b.t for b in self.dout],
                                  work2.t)
        held = [c, z, self.cu, self.x0, dcu, dx0, work, S, dwav, self.y1, self.wav, self.dy1, self.ds, work2] + self.us + [b for b in (self.dc, self.dz) if b]
        if need_w:
            held += [self.din[0], self.din[2], self.din[3]] + self.din[1] + list(self.dout)
        assert all(b.intact() for b in held)
        # the two du that are still in the workspace: du_k sits in buffer (ns - 1 - k) & 1 behind the partials
        rows, du_floats = plan.stage_rows(F), (n // scales[-1] * A + 3) // 4 * 4
        base = work.n - 2 * du_floats
        wk = work.t.cpu().numpy()
        self.dus = {k: wk[base + ((ns - 1 - k) & 1) * du_floats :][: rows[k] * A].reshape(rows[k], A).copy() for k in range(min(ns, 2))} if need_w or need_c else {}

    def grads(self):
        """(dwin [A, A, K], [dh], dw0, db0, dW1 [out, in], db1, dw3, db3) in torch's orientation, float64"""
        A = self.plan.A
        return (self.din[0].np().reshape(-1, A, A).transpose(2, 1, 0), [b.np() for b in self.din[1]], self.din[2].np(), self.din[3].np(), self.dout[0].np().T,
                self.dout[1].np(), self.dout[2].np(), self.dout[3].np())

    def bits(self):
        bufs = [self.cu, self.x0, self.wav, self.y1, self.ds, self.dc, self.dz] + self.us + [self.din[0], self.din[2], self.din[3]] + self.din[1] + list(self.dout)
        return [b.bits() for b in bufs] + [self.dus[k].tobytes() for k in sorted(self.dus)]


@functools.lru_cache(maxsize=None)
def run_of(G, shape, A, ctx, Rc):
    ref = E.reference(shape, A, ctx, Rc)
    return Run(G, ref["w"], ref["inp"], ref["frames"], ref["scales"], ctx)


@pytest.mark.parametrize("shape,A,ctx,Rc", E.CASES)
def test_every_launch_alone_and_each_end_end_to_end(G, shape, A, ctx, Rc):
    """every launch on the device's own inputs to the first term of its bound, then each end against the statement's running bounds"""
    ref, run = E.reference(shape, A, ctx, Rc), run_of(G, shape, A, ctx, Rc)
    w, inp, frames, scales = ref["w"], ref["inp"], ref["frames"], ref["scales"]
    ns, rows = len(scales), E.stage_rows(frames, scales)
    us = [u.np() for u in run.us] + [run.cu.np()]
    one, end = {}, {}
    r = E.conv_in(inp["c"], w["win"], frames, ctx)
    one["u0"] = E.share(us[0] - r["u"], r["e"])
    for i, s in enumerate(scales):
        r = E.stage(us[i], w["hs"][i], rows[i], s)
        one["u%d" % (i + 1)] = E.share(us[i + 1] - r["u"], r["e"])
    rf, rb = ref["fw"], ref["bw"]
    one["x0"] = E.share(run.x0.np() - rf["x0"], rf["e_x0"])
    end["cu"] = E.share(us[-1] - rf["cu"], rf["e_cu"])
    for i in range(ns):
        end["u%d" % i] = E.share(us[i] - rf["us"][i], rf["e_us"][i])
    # backward, input side: g_k is the gradient of stage k's output
    g_of = {ns - 1: f8(inp["dcu"])}
    for k in run.dus:
        if k >= 1:
            g_of[k - 1] = f8(run.dus[k])
    for k in sorted(run.dus):
        end["du%d" % k] = E.share(run.dus[k] - rb["dus"][k], rb["e_dus"][k])
        if k in g_of:
            r = E.stage_backward(g_of[k], w["hs"][k], rows[k], scales[k])
            one["du%d" % k] = E.share(run.dus[k] - r["d"], r["e"])
    dwin, dhs, dw0, db0, dW1, db1, dw3, db3 = run.grads()
    for k in range(ns):
        end["dh%d" % k] = E.share(dhs[k] - rb["dhs"][k], rb["e_dhs"][k])
        if k in g_of:
            r = E.filter_gradient(us[k], g_of[k], rows[k], scales[k])
            one["dh%d" % k] = E.share(dhs[k] - r["d"], r["e"])
    r = E.conv_in_backward(inp["c"], run.dus[0], w["win"], frames, ctx)
    one["dwin"], one["dc"] = E.share(dwin - r["dwin"], r["e_dwin"]), E.share(run.dc.np() - r["dc"], r["e_dc"])
    for k, got in (("dwin", dwin), ("dc", run.dc.np()), ("dw0", dw0), ("db0", db0), ("dz", run.dz.np())):
        end[k] = E.share(got - rb[k], rb["e_" + k])  # (first_conv's gradients are one launch on exact inputs: the same bound both ways)
    # output side
    qf, qb, free = ref["ofw"], ref["obw"], ref["free"]
    y1, dy1, S = run.y1.np(), run.dy1.np(), f8(inp["S"])
    one["y1"] = end["y1"] = E.share(y1 - qf["y1"], qf["e_y1"])
    wav1 = y1 @ f8(w["w3"]) + float(w["b3"][0])
    one["wav"] = E.share(run.wav.np() - wav1, (Rc + 2) * E.U * (np.abs(y1) @ np.abs(f8(w["w3"])) + abs(float(w["b3"][0]))))
    end["wav"] = E.share(run.wav.np() - qf["wav"], qf["e_wav"])
    on_s = (inp["S"] * np.float32(0.5)) > 0  # the device's own test, in float32
    a1 = E.output_backward(w, S, E.LAYERS, inp["dwav"], y1 > 0, on_s, y1=y1)
    one["dy1"] = E.share(dy1 - a1["dy1"], a1["e_dy1"])
    a2 = E.output_backward(w, S, E.LAYERS, inp["dwav"], y1 > 0, on_s, y1=y1, dy1=dy1)
    for k, got in (("ds", run.ds.np()), ("dW1", dW1), ("db1", db1), ("dw3", dw3), ("db3", db3)):
        one[k] = E.share(got - a2[k], a2["e_" + k])
    end["dy1"] = E.share(dy1 - qb["dy1"], qb["e_dy1"], free["y1"])
    end["ds"] = E.share(run.ds.np() - qb["ds"], qb["e_ds"], free["s"])
    for k, got in (("dW1", dW1), ("db1", db1), ("dw3", dw3), ("db3", db3)):
        end[k] = E.share(got - qb[k], qb["e_" + k])
    print("%s A %d ctx %d R %d: launches alone %s" % (shape, A, ctx, Rc, {k: round(v, 4) for k, v in one.items()}))
    print("   end to end %s" % {k: round(v, 4) for k, v in end.items()})
    assert free["y1"].mean() <= E.MAX_FREE
    assert max(one.values()) <= 1.0 and max(end.values()) <= 1.0, (one, end)
    # the launches of a full backward pass: one filter gradient and one transposed stage per scale, every sum reduced by a launch of its own
    si, so = run.seen_in, run.seen_out
    assert si["pwe_dh_kernel"]["launches"] == ns and si[G.IN_DU_KERNEL]["launches"] == ns and si["pwe_reduce_kernel"]["launches"] == ns + 3
    assert si["pwe_outer_kernel"]["launches"] == 1 and si["pwe_dwin_kernel"]["launches"] == 1 and si[G.IN_DC_KERNEL]["launches"] == 1
    assert si[G.IN_DZ_KERNEL]["launches"] == 1 and not any(k.startswith("pwt_") for k in list(si) + list(so))
    assert all(so[k]["launches"] == 1 for k in G.OUT_DX_KERNELS + G.OUT_DW_KERNELS[:2]) and so["pwe_reduce_kernel"]["launches"] == 4


def _stage_alone(G, w, k, rows, u, g, A):
    """pwe_dh_kernel and pwe_stage_bwd_kernel of stage k alone: a one-scale plan whose frames are the stage's input rows -> (du [rows, A], dh) float64"""
    s, n_in = int((len(w["hs"][k]) - 1) // 2), sum(rows)
    plan, maps = plan_of(G, 16, A, 0, (s,)), G.FrameMaps(rows, s, DEV)
    rng = np.random.RandomState(5)
    pin = G.pack_in_weights(t(w["win"][:, :, :1]), [t(w["hs"][k].reshape(1, 1, 1, -1))], t(rng.standard_normal((16, 1, 1))), t(rng.standard_normal(16)))
    c, z, ub = Guarded(n_in, A).set(rng.standard_normal((n_in, A))), Guarded(n_in * s).set(rng.standard_normal(n_in * s)), Guarded(n_in, A).set(u)
    dcu, dx0 = Guarded(n_in * s, A).set(g), Guarded(n_in * s, 16).set(rng.standard_normal((n_in * s, 16)))
    din, work = (Guarded(A, A), [Guarded(2 * s + 1)], Guarded(16), Guarded(16)), Guarded(plan.ends_workspace_floats(maps))
    with record() as seen:
        G.launch_in_backward(plan, maps, dcu.t, dx0.t, z.t, c.t, pin, [ub.t], (din[0].t, [din[1][0].t], din[2].t, din[3].t), None, None, work.t)
    assert seen["pwe_dh_kernel"]["launches"] == 1 and seen[G.IN_DU_KERNEL]["launches"] == 1 and G.IN_DC_KERNEL not in seen
    assert all(b.intact() for b in (c, z, ub, dcu, dx0, work, din[0], din[1][0], din[2], din[3]))
    du_floats = (n_in * A + 3) // 4 * 4
    return work.t.cpu().numpy()[work.n - 2 * du_floats :][: n_in * A].reshape(n_in, A).copy(), din[1][0].np()


@pytest.mark.parametrize("A", [16, 80])
def test_each_stage_backward_alone_at_every_depth(G, A):
    """scales (4, 4, 4, 4): du_k and dh_k of every stage, from the statement's u_k and du_{k + 1} (dcu for the last) rounded to float32, to the first
    term of their bounds; and du_k of the pack is the utterances' alone bit for bit"""
    ref = E.reference("hop256", A, 0, 16)
    w, frames, scales = ref["w"], ref["frames"], ref["scales"]
    rows_of, f4 = E.stage_rows(frames, scales), lambda a: np.asarray(a, np.float32)
    shares = {}
    for k in range(len(scales)):
        rows, s = rows_of[k], scales[k]
        u, g = f4(ref["fw"]["us"][k]), f4(ref["bw"]["dus"][k + 1] if k + 1 < len(scales) else ref["inp"]["dcu"])
        du, dh = _stage_alone(G, w, k, rows, u, g, A)
        rd, rh = E.stage_backward(g, w["hs"][k], rows, s), E.filter_gradient(u, g, rows, s)
        shares["du%d" % k], shares["dh%d" % k] = E.share(du - rd["d"], rd["e"]), E.share(dh - rh["d"], rh["e"])
        alone = []
        for (lo, hi) in E.spans(rows):
            alone.append(_stage_alone(G, w, k, [hi - lo], u[lo:hi], g[lo * s : hi * s], A)[0])
        assert du.astype(np.float32).tobytes() == b"".join(a.astype(np.float32).tobytes() for a in alone), k
    print("A %d, every stage's backward alone: %s" % (A, {k: round(v, 4) for k, v in shares.items()}))
    assert max(shares.values()) <= 1.0 and min(shares["du%d" % k] for k in range(4)) > 0, shares


CASE = ("hop6", 16, 2, 16)


def test_two_passes_are_bit_identical(G):
    ref = E.reference(*CASE)
    again = Run(G, ref["w"], ref["inp"], ref["frames"], ref["scales"], CASE[2])
    assert again.bits() == run_of(G, *CASE).bits()
    big = ("hop6", 80, 2, 64)
    ref = E.reference(*big)
    assert Run(G, ref["w"], ref["inp"], ref["frames"], ref["scales"], big[2]).bits() == run_of(G, *big).bits()


def _slices(inp, frames, hop, ctx, which):
    """the inputs of the utterances `which` of a pack, packed"""
    s, cs = E.spans(frames, hop), E.spans(frames, extra=2 * ctx)
    cat = lambda a, sp: np.concatenate([a[sp[b][0] : sp[b][1]] for b in which])
    return dict(c=cat(inp["c"], cs), **{k: cat(inp[k], s) for k in ("z", "dcu", "dx0", "S", "dwav")})


@pytest.mark.parametrize("shape,A,ctx,Rc", [CASE, ("hop256", 80, 0, 64)])
def test_batch_is_the_utterances_alone_bit_for_bit(G, shape, A, ctx, Rc):
    """cu, x0, the waveform, dS, the du still held, dc and dz of the pack are the concatenation of one run per utterance"""
    ref, run = E.reference(shape, A, ctx, Rc), run_of(G, shape, A, ctx, Rc)
    frames, scales = ref["frames"], ref["scales"]
    hop = int(np.prod(scales))
    alone = [Run(G, ref["w"], _slices(ref["inp"], frames, hop, ctx, [b]), [frames[b]], scales, ctx) for b in range(len(frames))]
    for name in ("cu", "x0", "wav", "y1", "ds", "dc", "dz"):
        assert getattr(run, name).bits() == b"".join(getattr(a, name).bits() for a in alone), name
    for k in run.dus:
        assert run.dus[k].tobytes() == b"".join(a.dus[k].tobytes() for a in alone), k


def test_another_utterance_in_the_pack_leaves_the_rest_bit_identical(G):
    ref, run = E.reference(*CASE), run_of(G, *CASE)
    frames, scales, ctx = ref["frames"], ref["scales"], CASE[2]
    hop = int(np.prod(scales))
    order = [0, 1, 3, 2, 4]  # utterance 3 (9 frames) moved in front of utterance 2: every later row shifts, the 1-frame utterance keeps its neighbours
    other = Run(G, ref["w"], _slices(ref["inp"], frames, hop, ctx, order), [frames[b] for b in order], scales, ctx)
    s_old, s_new = E.spans(frames, hop), E.spans([frames[b] for b in order], hop)
    for name, width in (("cu", 16), ("x0", 16), ("wav", 1), ("ds", 16), ("dz", 1)):
        a, b = getattr(run, name).np().reshape(-1, width), getattr(other, name).np().reshape(-1, width)
        for pos, utt in enumerate(order):
            assert np.array_equal(a[s_old[utt][0] : s_old[utt][1]], b[s_new[pos][0] : s_new[pos][1]]), (name, utt)


def test_launch_omissions(G):
    """no weight requires a gradient: no sum over samples is launched; dc and dz not asked: neither kernel runs; nothing but dz asked: no stage runs backward"""
    ref = E.reference(*CASE)
    args = (G, ref["w"], ref["inp"], ref["frames"], ref["scales"], CASE[2])
    full = run_of(G, *CASE)
    no_w = Run(*args, need_w=False)
    sums = ("pwe_outer_kernel", "pwe_dh_kernel", "pwe_dwin_kernel", "pwe_reduce_kernel", "pwe_dw_kernel<last>")
    assert not any(k in no_w.seen_in or k in no_w.seen_out for k in sums)
    assert no_w.seen_in[G.IN_DU_KERNEL]["launches"] == 2 and G.IN_DC_KERNEL in no_w.seen_in and G.IN_DZ_KERNEL in no_w.seen_in
    assert set(no_w.seen_out) == set(G.OUT_DX_KERNELS)
    assert no_w.dc.bits() == full.dc.bits() and no_w.dz.bits() == full.dz.bits() and no_w.ds.bits() == full.ds.bits()
    no_cz = Run(*args, need_c=False, need_z=False)
    assert G.IN_DC_KERNEL not in no_cz.seen_in and G.IN_DZ_KERNEL not in no_cz.seen_in and no_cz.seen_in[G.IN_DU_KERNEL]["launches"] == 2
    assert [b.bits() for b in no_cz.din[1]] == [b.bits() for b in full.din[1]] and no_cz.din[0].bits() == full.din[0].bits()
    only_z = Run(*args, need_w=False, need_c=False)
    assert set(only_z.seen_in) == {G.IN_DZ_KERNEL} and only_z.dz.bits() == full.dz.bits()


def test_autograd_functions_follow_requires_grad(G):
    """the same omissions through input_end / output_end: what does not require a gradient gets None and its kernels are not launched"""
    ref = E.reference(*CASE)
    w, inp, frames, scales, ctx = ref["w"], ref["inp"], ref["frames"], ref["scales"], CASE[2]
    plan, maps = plan_of(G, 16, 16, ctx, scales), G.FrameMaps(frames, 6, DEV)
    tw = dict(win=t(w["win"]), hs=[t(h.reshape(1, 1, 1, -1)) for h in w["hs"]], w0=t(w["w0"].reshape(16, 1, 1)), b0=t(w["b0"]), W1=t(w["W1"].reshape(16, 16, 1)),
              b1=t(w["b1"]), w3=t(w["w3"].reshape(1, 16, 1)), b3=t(w["b3"]))

    def go(weights, inputs):
        ps = [tw["win"], tw["w0"], tw["b0"], tw["W1"], tw["b1"], tw["w3"], tw["b3"]] + tw["hs"]
        for p in ps:
            p.requires_grad_(weights)
            p.grad = None
        z, c, S = t(inp["z"]).requires_grad_(inputs), t(inp["c"]).requires_grad_(inputs), t(inp["S"]).requires_grad_(True)
        with record() as seen:
            cu, x0 = G.input_end(plan, maps, z, c, tw["win"], tw["hs"], tw["w0"], tw["b0"])
            wav = G.output_end(plan, maps, S, tw["W1"], tw["b1"], tw["w3"], tw["b3"])
            if weights or inputs:
                ((cu * t(inp["dcu"])).sum() + (x0 * t(inp["dx0"])).sum()).backward()
            (wav * t(inp["dwav"])).sum().backward()
        return seen, ps, z, c, S

    full = run_of(G, *CASE)
    seen, ps, z, c, S = go(True, True)
    dwin, dhs, dw0, db0, dW1, db1, dw3, db3 = full.grads()
    same = lambda p, want: np.array_equal(p.grad.cpu().numpy().reshape(want.shape), want.astype(np.float32))
    assert same(ps[0], dwin) and same(ps[1], dw0) and same(ps[2], db0) and same(ps[3], dW1) and same(ps[4], db1) and same(ps[5], dw3) and same(ps[6], db3)
    assert all(same(p, d) for p, d in zip(ps[7:], dhs)) and same(z, full.dz.np()) and same(c, full.dc.np()) and same(S, full.ds.np())
    seen, ps, z, c, S = go(False, True)
    assert all(p.grad is None for p in ps) and "pwe_reduce_kernel" not in seen and same(c, full.dc.np()) and same(S, full.ds.np())
    seen, ps, z, c, S = go(True, False)
    assert z.grad is None and c.grad is None and G.IN_DC_KERNEL not in seen and G.IN_DZ_KERNEL not in seen and same(ps[0], dwin)


@pytest.mark.parametrize("with_lens", [False, True])
def test_module_hip_ends_against_torch_ends(G, with_lens):
    """(1, 5, 22) frames at hop 6 (pwge_ref.module_case): forward(ends="hip") and forward(ends="torch") each within the whole generator's running float32
    bound of the float64 statement (pwge_ref.generator), for the waveform and every parameter's gradient -- so the two agree within the sum of the two
    evaluations' bounds, which is asserted as well.  With lens: one padded batch, whose padding is zero with exactly zero gradient; without: the same
    three utterances as three batches of one, their gradients accumulated."""
    frames, hop = list(E.MODULE_FRAMES), 6
    cfg, sd, mels, noise, dwav = E.module_case()
    _, _, wav, e_wav, grads, bounds = E.module_reference()
    m, full = module_of(G, sd, cfg, use_weight_norm=False)
    ctx = m.ctx
    z, c = padded_inputs(full, mels, noise)
    z.requires_grad_(True), c.requires_grad_(True)
    dw = torch.zeros_like(z)
    for i, (lo, hi) in enumerate(E.spans(frames, hop)):
        dw[i, 0, : hi - lo] = t(dwav[lo:hi])
    dw[:, 0, :][dw[:, 0, :] == 0] = 1.0  # (a gradient arrives at the padding too, and must not get through)

    def leg(ends):
        for p in m.parameters():
            p.grad = None
        z.grad, c.grad = None, None
        with record() as seen:
            if with_lens:
                y = m(z, c, lens=frames, ends=ends)
                (y * dw).sum().backward()
                ys = [y[i, 0, : n * hop] for i, n in enumerate(frames)]
                for i, n in enumerate(frames):
                    assert not y[i, 0, n * hop :].any() and not z.grad[i, 0, n * hop :].any() and not c.grad[i, :, n + 2 * ctx :].any()
                    assert z.grad[i, 0, : n * hop].abs().sum() > 0 and c.grad[i, :, : n + 2 * ctx].abs().sum() > 0
            else:
                ys = []
                for i, n in enumerate(frames):
                    y = m(z[i : i + 1, :, : n * hop], c[i : i + 1, :, : n + 2 * ctx], ends=ends)
                    (y * dw[i : i + 1, :, : n * hop]).sum().backward()
                    ys.append(y[0, 0])
        got = torch.cat(ys).detach().cpu().numpy().astype(np.float64)
        return seen, got, {k: p.grad.cpu().numpy().astype(np.float64) for k, p in m.named_parameters()}

    seen_h, wav_h, g_h = leg("hip")
    seen_t, wav_t, g_t = leg("torch")
    ours = G.IN_FWD_KERNELS + (G.OUT_FWD_KERNEL,) + G.OUT_DX_KERNELS + G.IN_DW_KERNELS + G.OUT_DW_KERNELS + (G.IN_DU_KERNEL, G.IN_DC_KERNEL, G.IN_DZ_KERNEL)
    assert all(k in seen_h for k in ours) and not any(k.startswith("pwe_") for k in seen_t) and G.FWD_KERNELS[0] in seen_t
    assert set(g_h) == set(grads)
    sh = dict(wav=E.share(wav_h - wav, e_wav), **{k: E.share(g_h[k] - grads[k], bounds[k]) for k in grads})
    st = dict(wav=E.share(wav_t - wav, e_wav), **{k: E.share(g_t[k] - grads[k], bounds[k]) for k in grads})
    both = dict(wav=E.share(wav_h - wav_t, 2 * e_wav), **{k: E.share(g_h[k] - g_t[k], 2 * bounds[k]) for k in grads})
    print("lens %s: worst share of the bound, hip ends %.3g (%s), torch ends %.3g (%s), hip against torch %.3g; waveform hip - torch %.3g of the peak" % (
        with_lens, max(sh.values()), max(sh, key=sh.get), max(st.values()), max(st, key=st.get), max(both.values()),
        np.abs(wav_h - wav_t).max() / np.abs(wav).max()))
    assert max(sh.values()) <= 1.0 and max(st.values()) <= 1.0 and max(both.values()) <= 1.0, (sh, st)
