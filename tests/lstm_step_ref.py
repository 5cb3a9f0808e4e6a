"""float64 statement of one LSTM step as include/fcl_hip.h documents fcl_lstm_step_t, its per-element error bound, and the seeded inputs of the
tests built on it (tests/test_lstm_step_ref_cpu.py without a GPU, tests/test_gpu_lstm_step_f64.py on one).  Plain numpy; nothing here calls, or is
derived from, a kernel of the library.

The cell (gate order i, f, g, o; row m, unit u, gate column n = gate * U + u):
    pre[m, n]  = sum_t A_t[m, :] . W_t[n, :] + bias[n] + G[m * g_row_mul + g_row_add, n] + (step / dur[m]) * rank1_w[n]
    i, f, o    = sigmoid(pre), g = tanh(pre);   c_new = f * c_old + i * g;   h_new = o * tanh(c_new)
The position quotient step / dur[m] is formed in float32 (as the header states); everything else in float64.  h_in == None is the ZERO-STATE form:
old h and c are 0.  Zoneout: with masks, a mask value of 1 keeps the OLD state (h and c independently); without, rate * old + (1 - rate) * new.
row_len: row m is live iff step < row_len[m]; a dead row passes h and c through.  m_dev: rows >= min(M, m_dev) are untouched everywhere (the
caller compares them with what its buffers held before: `rows` of the result).  Side outputs: gates = the activated i, f, g, o; c_new raw (before
zoneout); c_old / h_old the incoming state; out2 (out2_scatter) receives the zoned h of a live row and 0 for a dead row.

The bound (lstm_step_bound): the contraction is the only inexact input of the cell, so its error is carried through the float64 cell to first
order.  delta = 3e-5 * max(1, rms of the contraction part of pre): 3e-5 is the project's bound for a pre-split GEMM at unit output scale
(test_gpu_planes.py::test_linear_on_planes_vs_fp64_and_plane_output).  Per element, with F the absolute floor of one gate-function evaluation:
    e_i, e_f, e_o = delta * s (1 - s) + F,   e_g = delta * (1 - g^2) + F
    d c_new = e_f |c_old| + e_i |g| + e_g i                       (= delta (|c_old| f (1 - f) + |g| i (1 - i) + i (1 - g^2)) at F = 0)
    d h_new = e_o |tanh c_new| + o ((1 - tanh^2 c_new) d c_new + F)
    d h, d c = (1 - rate) * (d h_new, d c_new), or (1 - mask) * ... under sampled zoneout; 0 for a dead row (a copy); out2 as h.
Every output is computed and stored in float32: each bound above also carries 2^-21 (four roundings, each bounded by one float32 ulp: 1 - rate, the two
products of the blend, their sum) of the reference value -- for the expectation blend of rate |old| + (1 - rate) |new|, the magnitudes it sums
(where the gates are saturated the terms above fall below these roundings).  A kept or dead element is a copy: bound 0.
F = GATE_FLOOR = 1e-6: the smallest power of ten under which the float32 numpy restatement of the cell (lstm_step_f32: float32 matmul, exp,
division, tanh -- the precision of the device's v_exp_f32 / v_rcp_f32 gates, which csrc/lstm_epilogue.h puts at ~1e-7 each) stays within a quarter
of the bound at every element of the input families below (test_lstm_step_ref_cpu.py::test_gate_floor_is_the_smallest_power_of_ten; at 1e-7 it
does not: a saturated gate has delta * s (1 - s) -> 0 while float32 still rounds it by up to 6e-8)."""
import numpy as np

GATE_FLOOR = 1e-6
GEMM_BOUND = 3e-5
SENTINEL = 7.0


def f64(x):
    return None if x is None else np.asarray(x, dtype=np.float64)


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def contraction_f64(terms):
    """sum_t A_t . W_t^T in float64; terms = [(A [M, K], W [4U, K]), ...]"""
    return sum(f64(a) @ f64(w).T for a, w in terms)


def lstm_step_f64(mm, u, h_in, c_in, g=None, g_row_mul=0, g_row_add=0, bias=None, rank1_w=None, dur=None, step=0, zoneout=0.0, zone_keep_h=None,
                  zone_keep_c=None, row_len=None, m_dev=None):
    """One step on the contraction mm [M, 4U] (contraction_f64).  h_in None = the zero-state form (c_in is then ignored).  Returns a dict: rows
    (= min(M, m_dev): what lies beyond is untouched), live [M] bool, mm, pre, gates [M, 4U], c_new / h_new (raw), h / c (what the step stores),
    h_old / c_old, and rate / keep_h / keep_c for the bound."""
    mm = f64(mm)
    m = mm.shape[0]
    assert mm.shape == (m, 4 * u)
    pre = mm.copy()
    if bias is not None:
        pre += f64(bias)[None, :]
    if g is not None:
        pre += f64(g)[np.arange(m, dtype=np.int64) * g_row_mul + g_row_add]
    if rank1_w is not None:
        pos = np.float32(step) / np.asarray(dur, dtype=np.int32).astype(np.float32)  # the one float32 operation of the statement
        assert pos.dtype == np.float32
        pre += pos.astype(np.float64)[:, None] * f64(rank1_w)[None, :]
    zero_state = h_in is None
    h_old = np.zeros((m, u)) if zero_state else f64(h_in)
    c_old = np.zeros((m, u)) if zero_state else f64(c_in)
    ig, fg, og = sigmoid(pre[:, :u]), sigmoid(pre[:, u: 2 * u]), sigmoid(pre[:, 3 * u:])
    gg = np.tanh(pre[:, 2 * u: 3 * u])
    c_new = fg * c_old + ig * gg
    h_new = og * np.tanh(c_new)
    if zone_keep_h is not None:
        kh, kc = np.asarray(zone_keep_h) != 0, np.asarray(zone_keep_c) != 0
        h_z, c_z = np.where(kh, h_old, h_new), np.where(kc, c_old, c_new)
    else:
        kh = kc = None
        rate = float(np.float32(zoneout))
        h_z, c_z = rate * h_old + (1.0 - rate) * h_new, rate * c_old + (1.0 - rate) * c_new
    live = np.ones(m, bool) if row_len is None else step < np.asarray(row_len)
    h = np.where(live[:, None], h_z, h_old)
    c = np.where(live[:, None], c_z, c_old)
    rows = m if m_dev is None else min(m, int(m_dev))
    return dict(rows=rows, live=live, u=u, mm=mm, pre=pre, gates=np.concatenate([ig, fg, gg, og], axis=1), c_new=c_new, h_new=h_new, h=h, c=c, h_zoned=h_z,
                h_old=h_old, c_old=c_old, rate=float(np.float32(zoneout)), keep_h=kh, keep_c=kc)


def out2_scatter(prev, ref, out2_row_base=None, out2_row_mul=0, out2_row_add=0, out2_col_off=0, values=None):
    """The out2 buffer [R, ld2] after the step: `prev` with, for every row m < rows, the zoned h of a live row (0 for a dead one) at row
    (out2_row_base ? out2_row_base[m] : m * out2_row_mul) + out2_row_add, columns out2_col_off ... + U.  Returns (buffer, bool mask of what was
    written).  values: what to scatter instead of the reference's h (the per-element bound, to lay it out the same way)."""
    out = np.array(prev, dtype=np.float64)
    written = np.zeros(out.shape, bool)
    u, rows = ref["u"], ref["rows"]
    v = np.where(ref["live"][:, None], ref["h_zoned"], 0.0) if values is None else values
    ms = np.arange(rows, dtype=np.int64)
    r = (np.asarray(out2_row_base, dtype=np.int64)[:rows] if out2_row_base is not None else ms * out2_row_mul) + out2_row_add
    assert len(np.unique(r)) == rows, "two rows of the step write the same out2 row"
    out[r, out2_col_off: out2_col_off + u] = v[:rows]
    written[r, out2_col_off: out2_col_off + u] = True
    return out, written


def lstm_step_bound(ref, floor=GATE_FLOOR):
    """Per-element bounds of gates, c_new, h, c (and out2's values: the bound of h, 0 for a dead row) -- see the module docstring."""
    u = ref["u"]
    delta = GEMM_BOUND * max(1.0, float(np.sqrt(np.mean(ref["mm"] ** 2))))
    gt = ref["gates"]
    ig, fg, gg, og = gt[:, :u], gt[:, u: 2 * u], gt[:, 2 * u: 3 * u], gt[:, 3 * u:]
    e_i, e_f, e_o = (delta * s * (1.0 - s) + floor for s in (ig, fg, og))
    e_g = delta * (1.0 - gg ** 2) + floor
    d_c_new = e_f * np.abs(ref["c_old"]) + e_i * np.abs(gg) + e_g * ig
    tc = np.tanh(ref["c_new"])
    d_h_new = e_o * np.abs(tc) + og * ((1.0 - tc ** 2) * d_c_new + floor)
    ulp = lambda v: 2.0 ** -21 * np.abs(v)  # noqa: E731  (four roundings, each bounded by one float32 ulp)
    lv = ref["live"][:, None].astype(np.float64)
    if ref["keep_h"] is not None:  # an element either is a copy of the old state or the new value
        d_h = lv * (1.0 - ref["keep_h"]) * (d_h_new + ulp(ref["h_new"]))
        d_c = lv * (1.0 - ref["keep_c"]) * (d_c_new + ulp(ref["c_new"]))
    else:
        r = ref["rate"]
        d_h = lv * ((1.0 - r) * d_h_new + ulp(r * np.abs(ref["h_old"]) + (1.0 - r) * np.abs(ref["h_new"])))
        d_c = lv * ((1.0 - r) * d_c_new + ulp(r * np.abs(ref["c_old"]) + (1.0 - r) * np.abs(ref["c_new"])))
    return dict(delta=delta, gates=np.concatenate([e_i, e_f, e_g, e_o], axis=1) + ulp(gt), c_new=d_c_new + ulp(ref["c_new"]), h=d_h, c=d_c, out2=d_h)


def lstm_step_f32(terms, u, h_in, c_in, **kw):
    """The same statement evaluated in float32 numpy throughout (matmul, sums, exp, division, tanh): the arithmetic-precision model of the bound.
    Returns gates, c_new, h, c (float32)."""
    f = np.float32
    m = terms[0][0].shape[0]
    pre = np.zeros((m, 4 * u), f)
    for a, w in terms:
        pre += np.asarray(a, f) @ np.asarray(w, f).T
    if kw.get("bias") is not None:
        pre += np.asarray(kw["bias"], f)[None, :]
    if kw.get("g") is not None:
        pre += np.asarray(kw["g"], f)[np.arange(m, dtype=np.int64) * kw.get("g_row_mul", 0) + kw.get("g_row_add", 0)]
    if kw.get("rank1_w") is not None:
        pos = f(kw.get("step", 0)) / np.asarray(kw["dur"], np.int32).astype(f)
        pre += pos[:, None] * np.asarray(kw["rank1_w"], f)[None, :]
    h_old = np.zeros((m, u), f) if h_in is None else np.asarray(h_in, f)
    c_old = np.zeros((m, u), f) if h_in is None else np.asarray(c_in, f)
    sg = lambda x: f(1.0) / (f(1.0) + np.exp(-x))  # noqa: E731
    ig, fg, og, gg = sg(pre[:, :u]), sg(pre[:, u: 2 * u]), sg(pre[:, 3 * u:]), np.tanh(pre[:, 2 * u: 3 * u])
    c_new = fg * c_old + ig * gg
    h_new = og * np.tanh(c_new)
    if kw.get("zone_keep_h") is not None:
        h_z, c_z = np.where(np.asarray(kw["zone_keep_h"]) != 0, h_old, h_new), np.where(np.asarray(kw["zone_keep_c"]) != 0, c_old, c_new)
    else:
        rate = f(kw.get("zoneout", 0.0))
        h_z, c_z = rate * h_old + (f(1.0) - rate) * h_new, rate * c_old + (f(1.0) - rate) * c_new
    live = np.ones(m, bool) if kw.get("row_len") is None else kw.get("step", 0) < np.asarray(kw["row_len"])
    out = dict(gates=np.concatenate([ig, fg, gg, og], axis=1), c_new=c_new, h=np.where(live[:, None], h_z, h_old), c=np.where(live[:, None], c_z, c_old))
    assert all(v.dtype == f for v in out.values())
    return out


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------------------------
# One input FAMILY per (M, U, term widths): everything any option set reads, drawn once from RandomState(seed).  Scales: activations N(0,1) (the
# recurrent term's, = h_in, 0.5 N(0,1)), weights 0.5 N(0,1) / sqrt(sum K) -- a contraction part of rms ~0.45, so that what the P32 planes
# lose of the operands (2^-17 relative each: ~2e-5 of a unit-rms sum of 500 products at its worst element) stays within half of the 3e-5 bound --
# and additive operands wide enough to saturate the gates: G 1.5 N(0,1), bias 1.5 N(0,1), position weights N(0,1), c_old N(0,1).
# What the families must provide is asserted in test_lstm_step_ref_cpu.py::test_input_conditions.
T_BILSTM, T_STEP = 3, 1  # the BiLSTM form: G and out2 hold T_BILSTM time steps per row, the step runs t = T_STEP
STEP = 3                 # the decoder step of the position term
ZONEOUT = 0.1


def step_inputs(m, u, ks, seed=None):
    """dict of float32 / integer numpy arrays.  terms: [(A, W)], the LAST one being the recurrent term (its A is h_in) when there are two or
    more; a single-term family has an h_in of its own (the BiLSTM form: the input projection is in G)."""
    rng = np.random.RandomState(1000 * u + m + sum(ks) if seed is None else seed)
    f = np.float32
    rnd = lambda *s: rng.standard_normal(s).astype(f)  # noqa: E731
    ksum = float(sum(ks))
    h_in = rnd(m, u) * f(0.5)
    terms = []
    for i, k in enumerate(ks):
        rec = i == len(ks) - 1 and k == u
        terms.append((h_in if rec else rnd(m, k), rnd(4 * u, k) * f(0.5 / np.sqrt(ksum))))
    row_len = rng.randint(0, T_BILSTM + 1, size=m).astype(np.int32)  # 0 .. T: dead rows at t = T_STEP include length 0
    row_len[: min(m, 3)] = [T_BILSTM, 0, 1][: min(m, 3)]
    dur = rng.randint(1, 30, size=m).astype(np.int32)
    return dict(m=m, u=u, terms=terms, h_in=h_in, c_in=rnd(m, u), g=rnd(m, 4 * u) * f(1.5), g_t=rnd(m * T_BILSTM, 4 * u) * f(1.5), bias=rnd(4 * u) * f(1.5),
                wpos=rnd(4 * u), dur=dur, row_len=row_len, keep_h=(rng.random_sample((m, u)) < 0.5).astype(np.uint8),
                keep_c=(rng.random_sample((m, u)) < 0.5).astype(np.uint8), frame_off=(np.cumsum(dur) - dur).astype(np.int32))


# option sets (issue order): name -> (what the step reads and writes).  "zero": the zero-state form (only the non-recurrent terms are passed).
OPTIONS = {
    "l0": dict(g=True, pos=True, zoneout=ZONEOUT),                                  # decoder layer 0: G + position, no bias (fixed MODE 0)
    "l1": dict(bias=True, zoneout=ZONEOUT),                                         # decoder layer 1: bias (MODE 1)
    "l0z": dict(g=True, pos=True, zoneout=ZONEOUT, zero=True),                      # their zero-state forms (MODE 2 / 3)
    "l1z": dict(bias=True, zoneout=ZONEOUT, zero=True),
    "gen": dict(g=True, bias=True, pos=True, zoneout=ZONEOUT),                      # generic: G + bias + position together
    "genz": dict(g=True, bias=True, pos=True, zoneout=ZONEOUT, zero=True),
    "bilstm": dict(g_t=True, row_len=True, out2="bilstm"),                          # G row m * T + t, dead rows, out2 [M * T, 2U] at column U
    "train0": dict(g=True, pos=True, masks=True, save=True, out2="rows"),           # training forms: sampled zoneout, all four save_*, out2 row m
    "train1": dict(bias=True, masks=True, save=True, out2="rows"),
    "kd": dict(bias=True, zoneout=ZONEOUT, out2="frames"),                          # KD tap: out2 row frame_off[m] + step
}


def option_kwargs(inp, opt, m_dev=None):
    """(terms, h_in, c_in, keyword arguments of lstm_step_f64 / lstm_step_f32) of option set `opt` on the family `inp`"""
    o = OPTIONS[opt]
    zero = o.get("zero", False)
    terms = inp["terms"][:-1] if zero and len(inp["terms"]) > 1 else inp["terms"]
    kw = dict(zoneout=o.get("zoneout", 0.0), m_dev=m_dev)
    if o.get("g"):
        kw.update(g=inp["g"], g_row_mul=1, g_row_add=0)
    if o.get("g_t"):
        kw.update(g=inp["g_t"], g_row_mul=T_BILSTM, g_row_add=T_STEP, step=T_STEP)
    if o.get("bias"):
        kw.update(bias=inp["bias"])
    if o.get("pos"):
        kw.update(rank1_w=inp["wpos"], dur=inp["dur"], step=STEP)
    if o.get("out2") == "frames":
        kw.update(step=STEP)
    if o.get("masks"):
        kw.update(zone_keep_h=inp["keep_h"], zone_keep_c=inp["keep_c"])
    if o.get("row_len"):
        kw.update(row_len=inp["row_len"])
    return terms, (None if zero else inp["h_in"]), (None if zero else inp["c_in"]), kw


def out2_layout(inp, opt):
    """(shape, keyword arguments of out2_scatter, ld2) of the option set's out2 buffer, or None"""
    kind = OPTIONS[opt].get("out2")
    m, u = inp["m"], inp["u"]
    if kind == "bilstm":
        return (m * T_BILSTM, 2 * u), dict(out2_row_mul=T_BILSTM, out2_row_add=T_STEP, out2_col_off=u)
    if kind == "rows":
        return (m, u), dict(out2_row_mul=1, out2_row_add=0, out2_col_off=0)
    if kind == "frames":
        return (int(inp["dur"].sum()) + STEP, u), dict(out2_row_base=inp["frame_off"], out2_row_add=STEP, out2_col_off=0)
    return None


# the input families of the GPU cases: name -> (M, U, term widths).  M: the smallest row count at which the library's dispatch selects each kernel
# form (tests/test_gpu_lstm_step_f64.py asserts the launched kernel), plus rows that leave the last tile ragged.
FAMILIES = {
    "m1": (1, 256, (256, 256)), "m17": (17, 256, (256, 256)), "u24_m17": (17, 24, (36,)), "t3_m17": (17, 256, (32, 64, 256)),
    "m513": (513, 256, (256, 256)), "m737": (737, 256, (256, 256)), "u24_m513": (513, 24, (36,)), "u16_m513": (513, 16, (32, 16)),
    "m961": (961, 256, (256, 256)), "wide_m65": (65, 1024, (256, 1024)), "u32_m70": (70, 32, (32, 64)), "t3_m513": (513, 256, (32, 64, 256)),
    "m520": (520, 256, (256, 256)), "m600": (600, 256, (256, 256)), "m1930": (1930, 256, (256, 256)), "m1200": (1200, 256, (256, 256)),
    "m2310": (2310, 256, (256, 256)), "k260_m520": (520, 256, (260, 256)),
}


def family_inputs(name):
    m, u, ks = FAMILIES[name]
    return step_inputs(m, u, ks, seed=1 + sorted(FAMILIES).index(name))
