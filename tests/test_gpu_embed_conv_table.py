"""-m gpu: fcl_embed_conv_table_fwd (embedding + first encoder Conv1d as k table rows summed per output row) against the float64 statement of
tests/embed_conv_ref.py inside its rounding-count bound, the plane output against the documented split of the fp32 output bit for bit, the device
row count (rows at or beyond it untouched, guard lines around both outputs), out-of-range ids, and against the two launches it replaces
(fcl_embedding_fwd, then fcl_conv1d_planes_fwd) at the tolerance tests/test_gpu_planes.py holds that convolution to."""
import numpy as np
import pytest
import torch

import embed_conv_ref as R
from helpers import split_planes_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 128  # elements in front of and behind each output (512 bytes of fp32, 256 bytes of planes: both keep the alignment the entry asks for)
SENT_F, SENT_P = np.float32(-7777.25), np.int16(0x5A5A)
PLANES_CONV_TOL = 3e-5  # tests/test_gpu_planes.py::test_conv1d_on_planes_vs_the_fp32_operand_kernel: max_abs(y, y_ref) < 3e-5


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib

    return _lib.load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).contiguous()


def launch(lib, c, tab32, ids, m_dev, residual, want_y=True, want_p=True):
    """One launch into guarded, sentinel-filled buffers: (y [m, Cout] float32, planes int16 [m, Cout / 32 * 64]) as numpy; the guards are checked here."""
    from fcl_taco2_amd import _lib

    m, cout = c["m"], c["cout"]
    yb = torch.full((2 * GUARD + m * cout,), float(SENT_F), dtype=torch.float32, device=DEV)
    pb = torch.full((2 * GUARD + m * cout * 2,), int(SENT_P), dtype=torch.int16, device=DEV)
    assert (pb.data_ptr() + 2 * GUARD) % 128 == 0 and (yb.data_ptr() + 4 * GUARD) % 16 == 0
    md = dev(np.array([m_dev], dtype=np.int32)) if m_dev is not None else None
    keep = [dev(ids), dev(tab32), dev(c["bias"]), dev(c["seg_lo"]), dev(c["seg_hi"]), dev(c["embed"])]
    rc = lib.fcl_embed_conv_table_fwd(keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr(), keep[4].data_ptr(),
                                      keep[5].data_ptr() if residual else None, yb.data_ptr() + 4 * GUARD if want_y else None,
                                      pb.data_ptr() + 2 * GUARD if want_p else None, m, c["v"], cout, c["k"], c["act"],
                                      md.data_ptr() if md is not None else None, None)
    _lib.check(rc)
    torch.cuda.synchronize()
    y, p = yb.cpu().numpy(), pb.cpu().numpy()
    for g in (y[:GUARD], y[-GUARD:]):
        assert (g == SENT_F).all()
    for g in (p[:GUARD], p[-GUARD:]):
        assert (g == SENT_P).all()
    return y[GUARD:-GUARD].reshape(m, cout), p[GUARD:-GUARD].reshape(m, -1)


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "c%d_v%d_k%d" % s)
def test_kernel_against_the_float64_statement(lib, shape):
    cout, v, k = shape
    for name, lens in R.ROW_SETS.items():
        for residual in (False, True):
            c = R.make_case(cout, v, k, lens, residual)
            emb = c["embed"] if residual else None
            tab = R.tables_f64(c["wfold"], c["embed"])
            ref = R.ref_embed_conv(tab, c["bias"], c["ids"], c["seg_lo"], c["seg_hi"], c["act"], emb)
            bound = R.bound_embed_conv(tab, c["bias"], c["ids"], c["seg_lo"], c["seg_hi"], c["act"], emb)
            tab32 = tab.astype(np.float32)
            assert (c["ids"] == 0).any() or (c["ids"] == v - 1).any()
            full = None
            for m_dev in (None, 0, 11):
                rows = c["m"] if m_dev is None else min(m_dev, c["m"])
                y, p = launch(lib, c, tab32, c["ids"], m_dev, residual)
                err = np.abs(y[:rows].astype(np.float64) - ref[:rows])
                assert (err <= bound[:rows]).all(), (name, residual, m_dev, float((err / np.maximum(bound[:rows], 1e-300)).max()))
                assert (y[rows:] == SENT_F).all() and (p[rows:] == SENT_P).all()  # rows at or beyond *m_dev are not written
                assert np.array_equal(p[:rows].view(np.uint16).reshape(rows, cout // 32, 2, 32), split_planes_np(y[:rows]))  # y_p == split(y), bit for bit
                if m_dev is None:
                    full = (y, p)
                else:
                    assert np.array_equal(y[:rows], full[0][:rows])
            # either output alone: the same bits, the other buffer untouched
            y_only, p_none = launch(lib, c, tab32, c["ids"], None, residual, want_p=False)
            y_none, p_only = launch(lib, c, tab32, c["ids"], None, residual, want_y=False)
            assert np.array_equal(y_only, full[0]) and np.array_equal(p_only, full[1])
            assert (p_none == SENT_P).all() and (y_none == SENT_F).all()


def test_out_of_range_ids_contribute_nothing(lib):
    """fcl_embedding_fwd gives an id outside [0, V) a zero row; here it adds nothing to the sum and to the residual."""
    c = R.make_case(32, 3, 3, (5, 12), True)
    ids = c["ids"].copy()
    ids[3], ids[9] = -1, 3
    tab = R.tables_f64(c["wfold"], c["embed"])
    args = (c["bias"], ids, c["seg_lo"], c["seg_hi"], c["act"], c["embed"])
    y, _ = launch(lib, c, tab.astype(np.float32), ids, None, True)
    assert (np.abs(y.astype(np.float64) - R.ref_embed_conv(tab, *args)) <= R.bound_embed_conv(tab, *args)).all()


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("cout,v,k", [(256, 80, 5), (32, 3, 3)])
def test_against_the_launches_it_replaces(lib, cout, v, k, residual):
    from fcl_taco2_amd import ops

    if not ops.planes_enabled():
        pytest.skip("FCL_PRECISION=0 / FCL_PLANES=0: the pre-split operand path is off")
    c = R.make_case(cout, v, k, R.ROW_SETS["three_utts"], True)  # (Cin = Cout = a multiple of 32: the plane convolution's operand width)

    class CV(object):
        pass

    cv = CV()
    wp = ops.pack_conv1d_weight(dev(c["wfold"]))
    cv.wpp, cv.bias, cv.cin, cv.cout, cv.k = ops.pack_planes(wp.reshape(k * cout, c["cin"])), dev(c["bias"]), c["cin"], cout, k
    x, xp = ops.embedding(dev(c["ids"]), dev(c["embed"]), want_f32=True, want_planes=True)
    y_old, _ = ops.conv1d_planes(xp, cv, dev(c["seg_lo"]), dev(c["seg_hi"]), ops.ACT_RELU, residual=x if residual else None, want_f32=True)
    from fcl_taco2_amd.plan import embed_conv_tables_f64

    tabs = dev(embed_conv_tables_f64(wp.cpu().numpy(), c["embed"]).astype(np.float32))
    y_new, yp_new = ops.embed_conv_table(dev(c["ids"]), tabs, dev(c["bias"]), dev(c["seg_lo"]), dev(c["seg_hi"]), ops.ACT_RELU,
                                         residual_table=dev(c["embed"]) if residual else None, want_f32=True, want_planes=True)
    torch.cuda.synchronize()
    assert float((y_new - y_old).abs().max()) < PLANES_CONV_TOL
    assert np.array_equal(yp_new.cpu().numpy().view(np.uint16).reshape(c["m"], -1, 2, 32), split_planes_np(y_new.cpu().numpy()))
