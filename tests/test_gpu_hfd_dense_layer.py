"""A dense C -> C' layer computes the same bits through the scale discriminator's entries (fcl_hsd_layer_fwd / _dx / _dw with groups = 1) as through the
period discriminator's (fcl_hpd_layer_*): the grouped kernels with one group are the dense ones in another form, which is what lets the two files share
code (csrc/hfd_rows.h) and what any later merge of their C -> C' kernels rests on.
The bound is exact equality (torch.equal): with one group the grouped contraction index kk = j cin + c walks the taps and the channels in the dense
kernels' order, 16 per step, so every output is the same k-ordered fmaf chain on the same operands -- there is nothing to measure a tolerance from.
Every output buffer starts as a NaN pattern between guard zones, so a row that either path leaves unwritten fails the comparison too."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_features import DEV, Guarded, launched

pytestmark = pytest.mark.gpu
SEGMENTS = (1, 2, 40, 41, 130, 7, 300)  # utterances shorter than the kernel among them; the edges inside 128-row tiles
HPD = ("hpd_conv_kernel", "hpd_conv_dx_kernel", "hpd_dw_kernel", "hpd_dw_reduce_kernel")
HSD = ("hsd_conv_kernel", "hsd_conv_dx_kernel", "hsd_dw_kernel", "hsd_dw_reduce_kernel")


def heights(s):
    """SEGMENTS and one more utterance that brings the output rows to 1 061: a second weight-gradient chunk, and no multiple of a 128-row tile"""
    base = sum((h - 1) // s + 1 for h in SEGMENTS)
    return list(SEGMENTS) + [s * (1061 - base)]


# one, two and four column tiles on each side (tiles per workgroup of the forward / of the input gradient): 4 / 2, 1 / 1 (48 = 3 x 16), 2 / 4
@pytest.mark.parametrize("ci,co,k,s", [(32, 64, 5, 3), (16, 48, 3, 1), (64, 32, 5, 2)])
def test_a_dense_layer_is_bit_identical_through_the_grouped_and_the_dense_entries(ci, co, k, s):
    assert torch.cuda.is_available()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, hfd_common, hifigan_discriminator as PD, hifigan_scale_discriminator as SD, ops

    pad, hs = (k - 1) // 2, heights(s)
    maps = hfd_common.LayerMaps(hs, k, s, pad, DEV)
    n_in, n_out = maps.rows
    assert n_in == sum(hs) and n_out == 1061
    dense = PD.LayerPlan(DEV, ci, co, k, s, pad, 0.1)
    grouped = SD.LayerPlan(DEV, ci, co, k, s, pad, 1, 0.1)
    grouped.kinds = [SD.GROUPED]  # (LayerPlan sends a one-group layer of up to 5 taps to the dense entries: here it goes to the grouped ones)
    assert grouped.hsd(0) and not dense.hsd(0)
    gen = torch.Generator(device="cpu").manual_seed(1000 * ci + 10 * co + k + s)
    rnd = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float32)
    W, b = rnd(co, ci, k) * float(np.sqrt(2.0 / (ci * k))), rnd(co) * 0.1
    x = torch.nn.functional.leaky_relu(rnd(n_in, ci), 0.1)
    x[::5, ::3] = 0.0  # stored activations that are exactly zero take the slope
    g, ex = rnd(n_out, co), rnd(n_in, ci) * 0.3
    put = lambda a: Guarded(*a.shape).set(a.numpy())
    xd, gd, exd = put(x), put(g), put(ex)
    got = {}
    for plan, names, w in ((dense, HPD, W[..., None]), (grouped, HSD, W)):
        wf, wb, bias = hfd_common.pack_weights(plan, [w.to(DEV)], [b.to(DEV)])[0]
        y = Guarded(n_out, co)
        with launched(names[0]):
            hfd_common.launch_forward(plan, maps, xd.t, [(wf, wb, bias)], [y.t])
        dxs = []
        for extra in (None, exd):
            dx = Guarded(n_in, ci)
            args = hfd_common._args(plan, maps, 0, g=gd.t, w=wb, y=dx.t, h=xd.t, extra=None if extra is None else extra.t)
            with launched(names[1]):
                _lib.check(hfd_common._entry(plan, 0, "dx")(C.byref(args), ops._stream()))
            dxs.append(dx)
        dw, db, work = Guarded(k, ci, co), Guarded(co), Guarded(plan.workspace_floats(maps.rows))
        with launched(names[2], names[3]):
            hfd_common.launch_backward(plan, maps, gd.t, [], [(wf, wb, bias)], [], None, [(dw.t, db.t)], x=xd.t, grads=[], workspace=work.t)
        outs = dict(wf=wf, wb=wb, y=y, dx=dxs[0], dx_extra=dxs[1], dw=dw, db=db)
        assert all(buf.intact() for buf in (xd, gd, exd, y, dw, db, work) + tuple(dxs))
        got[names] = {key: (v.t.clone() if isinstance(v, Guarded) else v) for key, v in outs.items()}
    for key, a in got[HPD].items():
        assert bool(torch.isfinite(a).all()), key
        assert torch.equal(a, got[HSD][key]), (key, float((a - got[HSD][key]).abs().max()))
