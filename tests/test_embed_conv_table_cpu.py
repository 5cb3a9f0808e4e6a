"""The float64 statement of the table form of the first encoder stage (tests/embed_conv_ref.py) without a GPU: it IS embedding -> Conv1d -> eval
BatchNorm -> ReLU (-> + residual) per utterance (torch float64), a float32 evaluation in the kernel's order stays inside half of the rounding-count
bound, every wrong restatement leaves the bound, and the plan's table builder states the same tables."""
import numpy as np
import pytest
import torch

import embed_conv_ref as R

CASES = [(cout, v, k, name, res) for (cout, v, k) in R.SHAPES for name in R.ROW_SETS for res in (False, True)]


def _ids(c):
    return "c%d_v%d_k%d_%s_%s" % (c[0], c[1], c[2], c[3], "res" if c[4] else "nores")


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_statement_is_the_convolution_and_float32_uses_half_the_bound(case):
    cout, v, k, name, res = case
    c = R.make_case(cout, v, k, R.ROW_SETS[name], res)
    emb = c["embed"] if res else None
    # 1. folding: Conv1d -> BatchNorm(eval) == Conv1d with (w * scale, shift), in float64
    gamma, beta, mean, var = (torch.from_numpy(np.asarray(a, dtype=np.float64)) for a in c["bn"])
    wf64, bf64 = R.fold_bn_f64(c["w"], *c["bn"])
    x_all = torch.from_numpy(c["embed"].astype(np.float64))[torch.from_numpy(c["ids"])]  # gathered embeddings [m, Cin]
    s = 0
    for n in c["lens"]:
        x = x_all[s : s + n].t()[None]  # [1, Cin, n]
        z = torch.nn.functional.conv1d(x, torch.from_numpy(np.asarray(c["w"], dtype=np.float64)), padding=k // 2)
        bn = torch.nn.functional.batch_norm(z, mean, var, gamma, beta, False, 0.0, R.BN_EPS)
        folded = torch.nn.functional.conv1d(x, torch.from_numpy(wf64), torch.from_numpy(bf64), padding=k // 2)
        assert (bn - folded).abs().max().item() <= 1e-12 * max(1.0, bn.abs().max().item())
        s += n
    # 2. the statement on the plan's float32 folded weights == torch's convolution of each utterance on its own
    tab = R.tables_f64(c["wfold"], c["embed"])
    ref = R.ref_embed_conv(tab, c["bias"], c["ids"], c["seg_lo"], c["seg_hi"], c["act"], emb)
    s = 0
    for n in c["lens"]:
        x = x_all[s : s + n].t()[None]
        y = torch.relu(torch.nn.functional.conv1d(x, torch.from_numpy(c["wfold"].astype(np.float64)), torch.from_numpy(c["bias"].astype(np.float64)),
                                                  padding=k // 2))
        if res:
            y = y + x
        assert np.abs(y[0].t().numpy() - ref[s : s + n]).max() <= 1e-12 * max(1.0, np.abs(ref).max())
        s += n
    # 3. float32 in the kernel's order: at most half of the bound
    bound = R.bound_embed_conv(tab, c["bias"], c["ids"], c["seg_lo"], c["seg_hi"], c["act"], emb)
    err = np.abs(R.f32_embed_conv(tab, c["bias"], c["ids"], c["seg_lo"], c["seg_hi"], c["act"], emb).astype(np.float64) - ref)
    assert (err <= 0.5 * bound).all(), (err / bound).max()
    assert (c["ids"] == 0).any() or (c["ids"] == v - 1).any()


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "c%d_v%d_k%d" % s)
def test_wrong_restatements_leave_the_bound(shape):
    cout, v, k = shape
    c = R.make_case(cout, v, k, R.ROW_SETS["three_utts"], True)
    tab = R.tables_f64(c["wfold"], c["embed"])
    args = (c["bias"], c["ids"], c["seg_lo"], c["seg_hi"], c["act"], c["embed"])
    ref, bound = R.ref_embed_conv(tab, *args), R.bound_embed_conv(tab, *args)
    wrong = R.wrong_restatements(tab, *args)
    assert len(wrong) >= 8
    for name, y in wrong.items():
        assert (np.abs(y - ref) > bound).any(), name
    # the activations other than ReLU: the float32 model stays inside half of their bound as well
    for act in (R.ACT_NONE, R.ACT_TANH):
        a = (c["bias"], c["ids"], c["seg_lo"], c["seg_hi"], act, c["embed"])
        err = np.abs(R.f32_embed_conv(tab, *a).astype(np.float64) - R.ref_embed_conv(tab, *a))
        assert (err <= 0.5 * R.bound_embed_conv(tab, *a)).all()


def test_out_of_range_ids_are_zero_rows():
    c = R.make_case(32, 3, 3, (5, 12), True)
    ids = c["ids"].copy()
    ids[3], ids[9] = -1, 3
    tab = R.tables_f64(c["wfold"], c["embed"])
    ext = np.concatenate([c["embed"], np.zeros((1, c["cin"]), dtype=np.float32)])  # id 3 = a zero row
    ids_ext = np.where((ids < 0) | (ids >= 3), 3, ids)
    a = R.ref_embed_conv(tab, c["bias"], ids, c["seg_lo"], c["seg_hi"], c["act"], c["embed"])
    b = R.ref_embed_conv(R.tables_f64(c["wfold"], ext), c["bias"], ids_ext, c["seg_lo"], c["seg_hi"], c["act"], ext)
    assert np.array_equal(a, b)


def test_the_plan_builds_the_same_tables():
    from fcl_taco2_amd.plan import embed_conv_tables_f64

    c = R.make_case(256, 80, 5, (5, 12), True)
    wp = np.ascontiguousarray(c["wfold"].transpose(2, 0, 1))  # the plan's tap-major packing [k, Cout, Cin]
    mine, theirs = embed_conv_tables_f64(wp, c["embed"]), R.tables_f64(c["wfold"], c["embed"])
    assert mine.dtype == np.float64 and mine.shape == theirs.shape == (5, 80, 256)
    assert np.abs(mine - theirs).max() <= 1e-13 * np.abs(theirs).max()  # (float64 summation order only)
    assert np.mean(mine.astype(np.float32) != theirs.astype(np.float32)) < 2e-5  # rounded once: the same float32 tables but for double-rounding ties
