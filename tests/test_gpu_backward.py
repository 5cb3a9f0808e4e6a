"""-m gpu: gradient primitives (H13) vs torch autograd on CPU, each in isolation; exact-fp32 kernels."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import max_abs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, ops as _ops

    _lib.load()
    return _ops


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return t.to(DEV).contiguous()


def close(a, ref, atol=2e-4, rtol=3e-5):
    """max-abs within atol + rtol * max|ref|: the weight-gradient GEMM runs bf16x3-split operands by default (2^-16 relative per product,
    fp32 accumulation; exact fp32 MFMA under FCL_PRECISION=0), so sums over hundreds of O(1) products are compared relative to their size."""
    ref_t = ref.detach().cpu() if hasattr(ref, "detach") else torch.as_tensor(ref)
    return max_abs(a, ref_t) < atol + rtol * float(ref_t.abs().max())


def rnd(rng, *shape):
    return rng.standard_normal(shape).astype(np.float32)


@pytest.mark.parametrize("m,n,k", [(1, 4, 4), (33, 8, 12), (700, 80, 128), (2501, 256, 256), (5000, 384, 768), (64, 1024, 512)])
def test_gemm_tn_linear_weight_grad(ops, m, n, k):
    rng = np.random.RandomState(m + n)
    dy, x = rnd(rng, m, n), rnd(rng, m, k)
    out = torch.zeros(n, k, device=DEV)
    ops.gemm_tn(dev(dy), dev(x), out)
    ref = dy.astype(np.float64).T @ x.astype(np.float64)
    assert max_abs(out.cpu().double(), ref) < 2e-4 * max(1.0, np.sqrt(m))
    ops.gemm_tn(dev(dy), dev(x), out)  # accumulates
    assert max_abs(out.cpu().double(), 2 * ref) < 4e-4 * max(1.0, np.sqrt(m))


@pytest.mark.parametrize("cin,cout,ksz", [(16, 8, 5), (80, 128, 5), (256, 384, 3)])
def test_conv1d_backward_vs_autograd(ops, cin, cout, ksz):
    """dW per tap by gemm_tn with shifted, segment-bounded rows; dX by the forward conv on transposed, tap-reversed weights."""
    rng = np.random.RandomState(cin)
    seg_lens = [3, 1, 50, 17, 129]
    M = sum(seg_lens)
    lo = np.repeat(np.cumsum([0] + seg_lens[:-1]), seg_lens).astype(np.int32)
    hi = (lo + np.repeat(seg_lens, seg_lens)).astype(np.int32)
    x = torch.from_numpy(rnd(rng, M, cin)).requires_grad_(True)
    w = torch.from_numpy((rnd(rng, cout, cin, ksz) / np.sqrt(cin * ksz)).astype(np.float32)).requires_grad_(True)
    dy = torch.from_numpy(rnd(rng, M, cout))
    y = torch.cat([F.conv1d(x[s:e].t().unsqueeze(0), w, None, 1, (ksz - 1) // 2)[0].t() for s, e in zip(np.cumsum([0] + seg_lens[:-1]), np.cumsum(seg_lens))])
    (y * dy).sum().backward()
    pad = (ksz - 1) // 2
    dwp = torch.zeros(ksz, cout, cin, device=DEV)
    for j in range(ksz):
        ops.gemm_tn(dev(dy), dev(x.detach()), dwp[j], shift=j - pad, seg_lo=dev(lo), seg_hi=dev(hi))
    assert close(dwp.cpu().permute(1, 2, 0), w.grad)
    # dX: y[m] = sum_j x[m + j - pad] W_j  =>  dx[m] = sum_j dy[m - (j - pad)] W_j^T : a conv of dy with taps reversed, weights transposed
    wp = ops.pack_conv1d_weight(dev(w.detach()))  # [k, Cout, Cin]
    wt = torch.stack([ops.transpose2d(wp[ksz - 1 - j]) for j in range(ksz)])  # [k, Cin, Cout], tap order reversed
    dx = ops.conv1d(dev(dy), wt.contiguous(), None, dev(lo), dev(hi))
    assert max_abs(dx.cpu(), x.grad) < 2e-4


def test_act_bwd_colsum_transpose(ops):
    rng = np.random.RandomState(0)
    y, dy = rnd(rng, 301, 40), rnd(rng, 301, 40)
    keep = (rng.rand(301, 40) < 0.5).astype(np.uint8)
    for act, fn in ((0, lambda v: v), (1, torch.relu), (2, torch.tanh)):
        pre = torch.from_numpy(y).requires_grad_(True)
        out = fn(pre) * torch.from_numpy(keep).float() * 2.0
        out.backward(torch.from_numpy(dy))
        act_out = fn(torch.from_numpy(y))
        dz = ops.act_bwd(dev(dy), dev(act_out.numpy()), act, dev(keep), 2.0)
        assert max_abs(dz.cpu(), pre.grad) < 1e-6
    out = torch.zeros(40, device=DEV)
    ops.colsum(dev(dy), out)
    assert max_abs(out.cpu(), dy.sum(0)) < 1e-4
    g, b = 1 + 0.1 * rnd(rng, 40), rnd(rng, 40)
    out2 = torch.zeros(40, device=DEV)
    ops.colsum(dev(dy), out2, y=dev(y), gamma=dev(g), beta=dev(b), mode=2)
    assert max_abs(out2.cpu(), (dy * (y - b) / g).sum(0)) < 2e-3
    t = ops.transpose2d(dev(y))
    assert torch.equal(t.cpu(), torch.from_numpy(y).t().contiguous())


def test_l1_mse_grad(ops):
    rng = np.random.RandomState(1)
    a0, b = rnd(rng, 100, 8), np.abs(rnd(rng, 100, 8))
    valid = (rng.rand(100) < 0.6).astype(np.uint8)
    for blog in (None, 1.0):
        a = torch.from_numpy(a0).requires_grad_(True)
        bt = torch.from_numpy(b) if blog is None else torch.log(torch.from_numpy(b) + blog)
        mask = torch.from_numpy(valid).bool().unsqueeze(1).expand_as(a)
        d = (a - bt).masked_select(mask)
        (0.7 * d.abs().mean() + 1.3 * (d ** 2).mean()).backward()
        da = ops.l1_mse_grad(dev(a0), dev(b), dev(valid), float(mask.sum()), 0.7, 1.3, b_log_offset=blog)
        assert max_abs(da.cpu(), a.grad) < 1e-6


@pytest.mark.parametrize("c", [20, 384])
def test_layernorm_bwd_with_scalar_head(ops, c):
    """Against torch autograd at M = 97 (one row per wave), no dropout.  The keep mask, M = 1029 (a wave's second row) and C = 65 / 257 / 513 (the
    first channel count of each wider arm) are in tests/test_gpu_train_pointwise_f64.py, against the float64 statement."""
    rng = np.random.RandomState(c)
    m = 97
    x0, g0, b0, lw0, lb0 = 2 * rnd(rng, m, c) + 0.5, 1 + 0.1 * rnd(rng, c), rnd(rng, c), (rnd(rng, c) / np.sqrt(c)).astype(np.float32), rnd(rng, 1)
    dy, ds = rnd(rng, m, c), rnd(rng, m)
    pad = (rng.rand(m) < 0.2).astype(np.uint8)
    x, g, b, lw, lb = [torch.from_numpy(v).requires_grad_(True) for v in (x0, g0, b0, lw0, lb0)]
    y = F.layer_norm(x, (c,), g, b, 1e-12)
    s = (y @ lw + lb).masked_fill(torch.from_numpy(pad).bool(), 0.0)
    ((y * torch.from_numpy(dy)).sum() + (s * torch.from_numpy(ds)).sum()).backward()
    dg, db, dlw, dlb = (torch.zeros(c, device=DEV), torch.zeros(c, device=DEV), torch.zeros(c, device=DEV), torch.zeros(1, device=DEV))
    dx = ops.layernorm_bwd(dev(x0), dev(g0), dev(b0), 1e-12, dg, db, dy=dev(dy), lin_w=dev(lw0), ds=dev(ds), pad_mask=dev(pad), dlin_w=dlw, dlin_b=dlb)
    assert max_abs(dx.cpu(), x.grad) < 2e-4
    assert max_abs(dg.cpu(), g.grad) < 2e-4 and max_abs(db.cpu(), b.grad) < 2e-4
    assert max_abs(dlw.cpu(), lw.grad) < 2e-4 and max_abs(dlb.cpu(), lb.grad) < 2e-4


@pytest.mark.parametrize("masks", [False, True])
def test_lstm_cell_bwd_vs_autograd(ops, masks):
    rng = np.random.RandomState(5)
    m, u, zr = 37, 24, 0.1
    pre0, h0, c0 = rnd(rng, m, 4 * u), rnd(rng, m, u), rnd(rng, m, u)
    dh, dc = rnd(rng, m, u), rnd(rng, m, u)
    zh = (rng.rand(m, u) < 0.3).astype(np.uint8) if masks else None
    zc = (rng.rand(m, u) < 0.3).astype(np.uint8) if masks else None
    pre, h_old, c_old = [torch.from_numpy(v).requires_grad_(True) for v in (pre0, h0, c0)]
    i, f, g, o = pre.chunk(4, 1)
    i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
    c_new = f * c_old + i * g
    h_new = o * torch.tanh(c_new)
    if masks:
        mh, mc = torch.from_numpy(zh).float(), torch.from_numpy(zc).float()
        h_out, c_out = mh * h_old + (1 - mh) * h_new, mc * c_old + (1 - mc) * c_new
    else:
        h_out, c_out = zr * h_old + (1 - zr) * h_new, zr * c_old + (1 - zr) * c_new
    ((h_out * torch.from_numpy(dh)).sum() + (c_out * torch.from_numpy(dc)).sum()).backward()
    gates = torch.cat([i, f, g, o], 1).detach()
    dgates, dh_old, dc_old = ops.lstm_cell_bwd(dev(gates), dev(c0), dev(c_new.detach()), dev(dh), dev(dc), zr,
                                                dev(zh) if masks else None, dev(zc) if masks else None)
    assert max_abs(dgates.cpu(), pre.grad) < 1e-5
    assert max_abs(dh_old.cpu(), h_old.grad) < 1e-6 and max_abs(dc_old.cpu(), c_old.grad) < 1e-5


def test_scatter_add_and_adam_step(ops):
    rng = np.random.RandomState(2)
    src, idx = rnd(rng, 500, 32), rng.randint(0, 12, size=500).astype(np.int64)
    dst = torch.zeros(12, 32, device=DEV)
    ops.scatter_add_rows(dev(src), dev(idx), dst, skip=0)
    ref = np.zeros((12, 32), np.float64)
    for r, i in zip(src, idx):
        if i != 0:
            ref[i] += r
    assert max_abs(dst.cpu().double(), ref) < 1e-4
    # Adam with clip_grad_norm_(1.0): two steps vs torch.optim.Adam on CPU
    p0, grads = rnd(rng, 1000), [5 * rnd(rng, 1000), rnd(rng, 1000)]
    pt = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([pt], lr=1e-3, eps=1e-6, weight_decay=0.0)
    p, m, v = dev(p0.copy()), torch.zeros(1000, device=DEV), torch.zeros(1000, device=DEV)
    step_dev = torch.zeros(1, dtype=torch.int32, device=DEV)  # applied updates, advanced on the device
    for step, gnp in enumerate(grads, 1):
        pt.grad = torch.from_numpy(gnp.copy())
        torch.nn.utils.clip_grad_norm_([pt], 1.0)
        opt.step()
        nsq = torch.zeros(1, dtype=torch.float64, device=DEV)
        ops.sumsq_accum(dev(gnp), nsq)
        ops.adam_step(p, dev(gnp), m, v, nsq, 1.0, 1e-3, 0.9, 0.999, 1e-6, step_dev)
        assert max_abs(p.cpu(), pt.detach()) < 2e-6 and int(step_dev.item()) == step
    nan = torch.full((1,), float("nan"), dtype=torch.float64, device=DEV)
    before = p.clone()
    ops.adam_step(p, dev(grads[0]), m, v, nan, 1.0, 1e-3, 0.9, 0.999, 1e-6, step_dev)  # NaN grad norm -> the step is skipped (tts.py:175-178)
    assert torch.equal(p, before) and int(step_dev.item()) == 2  # ... and does not count (torch's per-parameter `step` would not advance either)
    status = torch.ones(1, dtype=torch.int32, device=DEV)
    nsq = torch.ones(1, dtype=torch.float64, device=DEV)
    ops.adam_step(p, dev(grads[0]), m, v, nsq, 1.0, 1e-3, 0.9, 0.999, 1e-6, step_dev, status)  # non-zero device status word -> skipped as well
    assert torch.equal(p, before) and int(step_dev.item()) == 2


@pytest.mark.parametrize("wd", [0.01, 0.3])
def test_adam_step_weight_decay_matches_torch(ops, wd):
    """`--weight-decay` (tts.py:397-399, tts_distill.py:418-420: torch.optim.Adam(weight_decay=...)): the L2 term joins the CLIPPED gradient inside
    the step.  Three steps vs torch.optim.Adam on CPU, with clip_grad_norm_(1.0) in between as the reference's update has it."""
    rng = np.random.RandomState(11)
    p0, grads = rnd(rng, 1500), [5 * rnd(rng, 1500), rnd(rng, 1500), 0.1 * rnd(rng, 1500)]
    pt = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([pt], lr=1e-3, eps=1e-6, weight_decay=wd)
    p, m, v = dev(p0.copy()), torch.zeros(1500, device=DEV), torch.zeros(1500, device=DEV)
    step_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    for step, gnp in enumerate(grads, 1):
        pt.grad = torch.from_numpy(gnp.copy())
        torch.nn.utils.clip_grad_norm_([pt], 1.0)
        opt.step()
        nsq = torch.zeros(1, dtype=torch.float64, device=DEV)
        ops.sumsq_accum(dev(gnp), nsq)
        ops.adam_step(p, dev(gnp), m, v, nsq, 1.0, 1e-3, 0.9, 0.999, 1e-6, step_dev, weight_decay=wd)
        assert max_abs(p.cpu(), pt.detach()) < 3e-6 and int(step_dev.item()) == step
    st = opt.state[pt]
    assert max_abs(m.cpu(), st["exp_avg"]) < 1e-6 and max_abs(v.cpu(), st["exp_avg_sq"]) < 1e-6
    # without the decay term the trajectories differ visibly: the flag is not a no-op
    p2, m2, v2 = dev(p0.copy()), torch.zeros(1500, device=DEV), torch.zeros(1500, device=DEV)
    s2 = torch.zeros(1, dtype=torch.int32, device=DEV)
    nsq = torch.zeros(1, dtype=torch.float64, device=DEV)
    ops.sumsq_accum(dev(grads[0]), nsq)
    ops.adam_step(p2, dev(grads[0]), m2, v2, nsq, 1.0, 1e-3, 0.9, 0.999, 1e-6, s2)
    ops.adam_step(p2, dev(grads[1]), m2, v2, nsq, 1.0, 1e-3, 0.9, 0.999, 1e-6, s2)
    assert float((m2 - m).abs().max()) > 1e-4


@pytest.mark.parametrize("m,n,k", [(1, 16, 256), (7, 100, 260), (16, 256, 1024), (33, 256, 1024), (64, 1024, 512),
                                   (100, 2048, 1024), (129, 2040, 4096), (200, 2048, 4096), (256, 2048, 4096), (256, 512, 1024), (250, 1000, 268), (17, 8200, 256)])
def test_small_m_split_k_gemm(ops, m, n, k):
    """The split-K kernel launch_gemm picks for M <= 256, K >= 256 (the per-step GEMMs of the BPTT recurrences; their residual epilogue is covered by
    the full-size training-step tests of test_gpu_training_fullsize.py, whose decoder BPTT runs the steps with at most 128 live rows -- the carry GEMMs
    with the carry as residual -- on this kernel).  Round 5: 32 x 32 and 16 x 32 output tiles per workgroup while they give a
    workgroup per CU (the second row of shapes: FCL-taco2-T sizes, ragged M / N against every tile form)."""
    rng = np.random.RandomState(m + k)
    x, w, b = rnd(rng, m, k), rnd(rng, n, k) / np.sqrt(k), rnd(rng, n)
    ref = x.astype(np.float64) @ w.astype(np.float64).T + b
    y = ops.linear(dev(x), dev(w.astype(np.float32)), dev(b))
    assert max_abs(y.cpu().double(), ref) < 2e-5
    y2 = ops.linear(dev(x), dev(w.astype(np.float32)))  # no bias
    assert max_abs(y2.cpu().double(), ref - b) < 2e-5


@pytest.mark.parametrize("H,lens", [(16, [19, 19, 12, 5, 1]), (128, [19, 19, 12, 5, 1]), (256, [19, 19, 12, 5, 1]), (24, [19, 19, 12, 5, 1]),
                                    (256, sorted(np.random.RandomState(9).randint(40, 81, 32).tolist(), reverse=True)),
                                    # round 5 (lane-split kernels: steps unrolled by 4 / 2 with operands prefetched 4 steps ahead): every residue of the
                                    # sequence length, a long sequence
                                    (128, [131, 64, 7, 6, 4, 3, 2, 1]), (256, [67, 66, 5, 4, 3, 2, 1, 1])])
def test_bilstm_train_forward_and_bptt_vs_torch_lstm(ops, H, lens):
    """fcl_bilstm_train_fwd / fcl_bilstm_bptt (persistent kernels for H <= 128, the 4-workgroup group kernels for H = 256, the per-step fallback for
    any other H) against torch.nn.LSTM over packed sequences: outputs, and — through the saved gates — the gradients of W_hh, W_ih and x.
    The inference entry (ops.bilstm, algo 0) takes the same kernels without saving and must agree too."""
    rng = np.random.RandomState(H)
    B, T, C = len(lens), max(lens), 32  # the last case fills all 256 CUs with 32 x 2 groups of 4 workgroups
    lstm = torch.nn.LSTM(C, H, 1, batch_first=True, bidirectional=True)
    x = torch.from_numpy(rnd(rng, B, T, C)).requires_grad_(True)
    packed = torch.nn.utils.rnn.pack_padded_sequence(x, lens, batch_first=True)
    ref, _ = torch.nn.utils.rnn.pad_packed_sequence(lstm(packed)[0], batch_first=True, total_length=T)
    d_out = rnd(rng, B, T, 2 * H)
    for b, l in enumerate(lens):
        d_out[b, l:] = 0.0
    (ref * torch.from_numpy(d_out)).sum().backward()
    sd = {k: v.detach() for k, v in lstm.named_parameters()}
    lens_dev = dev(np.array(lens, np.int32))
    xd = dev(x.detach().reshape(B * T, C))
    sfxs = ("", "_reverse")
    gx = [ops.linear(xd, dev(sd["weight_ih_l0" + s]), dev(sd["bias_ih_l0" + s] + sd["bias_hh_l0" + s])) for s in sfxs]
    whh = [dev(sd["weight_hh_l0" + s]) for s in sfxs]
    sv = [[torch.zeros(T, B, 4 * H, device=DEV)] + [torch.zeros(T, B, H, device=DEV) for _ in range(3)] for _ in sfxs]
    out = torch.empty(B * T, 2 * H, device=DEV)
    ops.bilstm_train_fwd(gx, whh, lens_dev, B, T, out, sv)
    assert max_abs(out.cpu().reshape(B, T, 2 * H), ref.detach()) < 2e-5
    inf = ops.bilstm(xd, lens_dev, dev(sd["weight_ih_l0"]), whh[0], dev(sd["bias_ih_l0"] + sd["bias_hh_l0"]), dev(sd["weight_ih_l0_reverse"]), whh[1],
                     dev(sd["bias_ih_l0_reverse"] + sd["bias_hh_l0_reverse"]), B, T)
    assert max_abs(inf.cpu().reshape(B, T, 2 * H), ref.detach()) < 2e-5
    dgs = [torch.empty(T, B, 4 * H, device=DEV) for _ in sfxs]
    ops.bilstm_bptt(sv, lens_dev, B, T, dev(d_out.reshape(B * T, 2 * H)), [ops.transpose2d(w) for w in whh], dgs)
    perm = dev(((np.arange(B * T) % T) * B + np.arange(B * T) // T).astype(np.int32))
    dx = torch.zeros(B * T, C, device=DEV)
    for d, s in enumerate(sfxs):
        dg2 = dgs[d].reshape(T * B, 4 * H)
        g_hh = torch.zeros(4 * H, H, device=DEV)
        ops.gemm_tn(dg2, sv[d][3].reshape(T * B, H), g_hh)
        assert close(g_hh.cpu(), dict(lstm.named_parameters())["weight_hh_l0" + s].grad), s
        dgx = ops.gather_rows(dg2, perm)
        g_ih = torch.zeros(4 * H, C, device=DEV)
        ops.gemm_tn(dgx, xd, g_ih)
        assert close(g_ih.cpu(), dict(lstm.named_parameters())["weight_ih_l0" + s].grad), s
        ops.add2d(dx, ops.linear(dgx, ops.transpose2d(dev(sd["weight_ih_l0" + s]))))
    assert max_abs(dx.cpu().reshape(B, T, C), x.grad) < 2e-4 * max(1.0, float(x.grad.abs().max()))


def test_bilstm_group_kernel_more_workgroups_than_cus(ops):
    """H = 256 group kernel with 8 B = 768 workgroups on a 256-CU part: groups are dispatched in id order, partially resident groups wait for running
    ones to retire (bounded spins), results equal the per-step algorithm."""
    B, T, C, H = 96, 40, 64, 256
    rng = np.random.RandomState(0)
    x = dev(rnd(rng, B * T, C))
    lens_np = np.sort(rng.randint(5, T + 1, B))[::-1].astype(np.int32).copy()
    lens_np[0] = T
    lens = dev(lens_np)
    w = lambda *s: dev((rnd(rng, *s) / np.sqrt(s[-1])).astype(np.float32))
    a = [w(4 * H, C), w(4 * H, H), w(4 * H), w(4 * H, C), w(4 * H, H), w(4 * H)]
    ref = ops.bilstm(x, lens, *a, B, T, 1)
    out = ops.bilstm(x, lens, *a, B, T, 3)
    assert max_abs(out.cpu(), ref.cpu()) < 1e-5


def test_bilstm_group_kernel_beside_another_streams_work(ops):
    """Rounds 5 - 6.  With the device to itself the lane-split BiLSTM kernels are exact; beside another stream's GEMMs they returned 1e-2 errors in lanes 48 - 63 of
    single waves in 299 of 300 launches (`tools/stress_bilstm_concurrent.py`).  Round 5 kept foreign waves off their SIMDs; round 6 found the cause -- packed-FP32
    VALU results go stale in the wave's last quarter while another wave of the SIMD issues MFMAs (`tools/hazard_trigger_scan.py`, `profiles/r6_packed_fp32_hazard_ab.log`) --
    and builds the library without packed-FP32 instructions (csrc/Makefile NOPK; tests/test_cabi_cpu.py disassembles it), so the kernels share their SIMDs again and THIS
    test is the functional guard: every launch of the H = 256 forward and reverse pass beside a stream of H = 128 recurrences (each with its two input-projection
    GEMMs), in both orders of submission, must equal the serial result bit for bit, and the status word stays clear; then the same for the H = 128 TRAINING pair
    (forward + BPTT) beside H = 256 work."""
    g = torch.Generator().manual_seed(3)

    def case(B, T, C, H):
        lens = torch.randint(30, T + 1, (B,), generator=g).to(torch.int32)
        lens[0] = T
        w = [(torch.randn(4 * H, d, generator=g) * 0.05).to(DEV) for d in (C, H, C, H)]
        bs = [(torch.randn(4 * H, generator=g) * 0.1).to(DEV) for _ in range(2)]
        return dict(B=B, T=T, H=H, x=torch.randn(B * T, C, generator=g).to(DEV), w=w, bs=bs, ld=lens.to(DEV))

    st = ops.status_word(DEV)

    def fwd(c):
        return ops.bilstm(c["x"], c["ld"], c["w"][0], c["w"][1], c["bs"][0], c["w"][2], c["w"][3], c["bs"][1], c["B"], c["T"], 3 if c["H"] == 256 else 2, status=st)

    big, small = case(8, 60, 512, 256), case(8, 60, 256, 128)
    B, T, H = big["B"], big["T"], 256
    gx = [torch.randn(B * T, 4 * H, generator=g).to(DEV) for _ in range(2)]
    sv = [[torch.zeros(T * B, 4 * H, device=DEV)] + [torch.zeros(T * B, H, device=DEV) for _ in range(3)] for _ in range(2)]
    o2 = torch.empty(B * T, 2 * H, device=DEV)
    ops.bilstm_train_fwd(gx, (big["w"][1], big["w"][3]), big["ld"], B, T, o2, sv, status=st)
    d_out = torch.randn(B * T, 2 * H, generator=g).to(DEV)
    wt = [big["w"][1].t().contiguous(), big["w"][3].t().contiguous()]

    def bptt():
        dg = [torch.empty(T * B, 4 * H, device=DEV) for _ in range(2)]
        ops.bilstm_bptt(sv, big["ld"], B, T, d_out, wt, dg, status=st)
        return dg

    ref_f, ref_b, ref_s = fwd(big).clone(), [d.clone() for d in bptt()], fwd(small).clone()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for it in range(60):
        if it % 2:  # (both orders of submission: either kernel family can be the one whose waves fall out of step)
            with torch.cuda.stream(s2):
                outs = [fwd(small) for _ in range(8)]
            with torch.cuda.stream(s1):
                o1 = fwd(big)
                dg = bptt()
        else:
            with torch.cuda.stream(s1):
                o1 = fwd(big)
                dg = bptt()
            with torch.cuda.stream(s2):
                outs = [fwd(small) for _ in range(4)]
        torch.cuda.synchronize()
        assert torch.equal(o1, ref_f), (it, float((o1 - ref_f).abs().max()))
        assert all(torch.equal(a, b) for a, b in zip(dg, ref_b)), it
        assert all(torch.equal(o, ref_s) for o in outs), it
    assert int(st.item()) == 0
    # round 6: the H = 128 training kernels (bilstm_ksplit_kernel<true> / bilstm_bptt_ksplit_kernel) beside a foreign stream of H = 256 recurrences
    Bs, Ts, Hs = small["B"], small["T"], 128
    gxs = [torch.randn(Bs * Ts, 4 * Hs, generator=g).to(DEV) for _ in range(2)]
    svs = [[torch.zeros(Ts * Bs, 4 * Hs, device=DEV)] + [torch.zeros(Ts * Bs, Hs, device=DEV) for _ in range(3)] for _ in range(2)]
    d_out_s = torch.randn(Bs * Ts, 2 * Hs, generator=g).to(DEV)
    wts = [small["w"][1].t().contiguous(), small["w"][3].t().contiguous()]

    def train_small():
        o = torch.empty(Bs * Ts, 2 * Hs, device=DEV)
        ops.bilstm_train_fwd(gxs, (small["w"][1], small["w"][3]), small["ld"], Bs, Ts, o, svs, status=st)
        dgs = [torch.empty(Ts * Bs, 4 * Hs, device=DEV) for _ in range(2)]
        ops.bilstm_bptt(svs, small["ld"], Bs, Ts, d_out_s, wts, dgs, status=st)
        return [o] + dgs

    ref_t = [t.clone() for t in train_small()]
    torch.cuda.synchronize()
    for it in range(40):
        first, second = (s1, s2) if it % 2 else (s2, s1)
        with torch.cuda.stream(first):
            got = [train_small() for _ in range(3)] if it % 2 else None
            if not it % 2:
                o1 = fwd(big)
        with torch.cuda.stream(second):
            if it % 2:
                o1 = fwd(big)
            else:
                got = [train_small() for _ in range(3)]
        torch.cuda.synchronize()
        assert torch.equal(o1, ref_f), it
        # (the three repetitions overwrite the same saved tensors with the same values; each result list is compared)
        assert all(torch.equal(a, b) for res in got for a, b in zip(res, ref_t)), it
    assert int(st.item()) == 0


# ---- round 5: the weight-gradient GEMM with the transposition fused into its LDS reads (csrc/dw_gemm.hip, `ds_read_b64_tr_b16`) -----------------
def _dw_on_path(ops_mod):
    """True when fcl_gemm_tn_* dispatches to dw_mfma_kernel (bf16x3 / bf16 arithmetic; FCL_PRECISION=0 keeps the exact-fp32 kernel)."""
    return ops_mod.planes_enabled()


@pytest.mark.parametrize("m,n,k", [(256, 32, 32), (300, 128, 128), (2501, 256, 256), (4999, 80, 256), (3333, 256, 80), (1030, 384, 36), (20000, 1024, 256),
                                   (513, 132, 260)])
def test_dw_mfma_linear_weight_grad(ops, m, n, k):
    """dW = dY^T X against float64: ragged N / K (not multiples of the 128-wide tile, of 16, of 32), contraction lengths that are not multiples of
    the 32-row chunk or of the slice, a strided output block whose neighbours must stay untouched, accumulation into a non-zero gradient."""
    from fcl_taco2_amd import _lib

    rng = np.random.RandomState(m + n + k)
    dy, x = rnd(rng, m, n), rnd(rng, m, k)
    ref = dy.astype(np.float64).T @ x.astype(np.float64)
    base = dev(rnd(rng, n, k + 8))
    out = base.clone()
    _lib.prof_enable(True)
    ops.gemm_tn(dev(dy), dev(x), out[:, 4 : 4 + k])
    torch.cuda.synchronize()
    prof = _lib.prof_collect()
    _lib.prof_enable(False)
    if _dw_on_path(ops):
        assert any(name.startswith("dw_mfma_kernel") for name in prof), sorted(prof)
    scale = float(np.abs(ref).max())
    assert max_abs((out[:, 4 : 4 + k] - base[:, 4 : 4 + k]).cpu().double(), ref) < 3e-5 * scale
    assert torch.equal(out[:, :4], base[:, :4]) and torch.equal(out[:, 4 + k :], base[:, 4 + k :])
    ops.gemm_tn(dev(dy), dev(x), out[:, 4 : 4 + k])  # accumulates
    assert max_abs((out[:, 4 : 4 + k] - base[:, 4 : 4 + k]).cpu().double(), 2 * ref) < 6e-5 * scale


@pytest.mark.parametrize("cin,cout,ksz", [(80, 128, 5), (256, 384, 3), (128, 80, 5)])
def test_dw_mfma_conv_taps_vs_autograd(ops, cin, cout, ksz):
    """All taps of a Conv1d weight gradient in one launch (fcl_gemm_tn_taps_fwd): shifted rows, zero outside each utterance's segment --
    segments of 1, 3, 31, 32, 33 and a few hundred rows, so chunk and slice boundaries fall inside and between segments."""
    rng = np.random.RandomState(cin + ksz)
    seg_lens = [3, 1, 350, 31, 32, 33, 129, 500, 2]
    M = sum(seg_lens)
    starts = np.cumsum([0] + seg_lens[:-1])
    lo = np.repeat(starts, seg_lens).astype(np.int32)
    hi = (lo + np.repeat(seg_lens, seg_lens)).astype(np.int32)
    x = torch.from_numpy(rnd(rng, M, cin)).requires_grad_(True)
    w = torch.from_numpy((rnd(rng, cout, cin, ksz) / np.sqrt(cin * ksz)).astype(np.float32)).requires_grad_(True)
    dy = torch.from_numpy(rnd(rng, M, cout))
    y = torch.cat([F.conv1d(x[s : s + n].t().unsqueeze(0).double(), w.double(), None, 1, (ksz - 1) // 2)[0].t() for s, n in zip(starts, seg_lens)])
    (y * dy.double()).sum().backward()
    dwp = torch.zeros(ksz, cout, cin, device=DEV)
    ops.gemm_tn_taps(dev(dy), dev(x.detach()), dwp, -((ksz - 1) // 2), seg_lo=dev(lo), seg_hi=dev(hi))
    ref = w.grad.permute(2, 0, 1)
    assert max_abs(dwp.cpu(), ref) < 3e-5 * float(ref.abs().max())


def test_dw_mfma_bf16_mode_rounds_operands_once(ops):
    """fcl_set_gemm_mode(BF16) (the --use-amp recipe): the product of the bf16-ROUNDED operands, accumulated in fp32."""
    if not _dw_on_path(ops):
        pytest.skip("FCL_PRECISION=0: no bf16 mode")
    rng = np.random.RandomState(5)
    m, n, k = 3000, 256, 128
    dy, x = dev(rnd(rng, m, n)), dev(rnd(rng, m, k))
    out = torch.zeros(n, k, device=DEV)
    with ops.gemm_mode("bf16"):
        ops.gemm_tn(dy, x, out)
    ref = dy.bfloat16().double().t() @ x.bfloat16().double()
    assert max_abs(out.double(), ref) < 3e-5 * float(ref.abs().max())
    exact = dy.double().t() @ x.double()
    assert float((out.double() - exact).abs().max()) > 1e-3  # the rounding is visible
