"""-m gpu: fcl_bilstm_rows_fwd, the synthesis BiLSTM (C = 256, H = 128) over COMPACT rows -- utterance b at rows [utt_row0[b], utt_row0[b] + len_b) of
an [n_rows, .] input and output -- against the padded entry (fcl_bilstm_fwd, utterance b at row b * T) on the same utterances: the real rows must be
bit-identical in the fp32 output and in its planes, the rows in [total, n_rows) zero, the lines behind n_rows untouched, and row maps that ride in
the launch must equal engine.build_row_maps (src_rows in compact row numbers)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C, H = 256, 128
SENTINEL = -7.25
TAIL = 5  # sentinel lines behind n_rows


@pytest.fixture(scope="module")
def weights():
    g = torch.Generator().manual_seed(128)
    return [(0.2 * torch.randn(sh, generator=g)).to(DEV) for sh in [(4 * H, C), (4 * H, H), (4 * H,), (4 * H, C), (4 * H, H), (4 * H,)]]


@pytest.fixture(scope="module")
def padded(weights):
    """Per (lens, T, planes): the inputs and the padded entry's outputs, computed once."""
    from fcl_taco2_amd import ops

    cache = {}

    def get(lens, T, planes):
        key = (lens, T, planes)
        if key not in cache:
            B = len(lens)
            g = torch.Generator().manual_seed(sum(lens) + T)
            x = torch.randn(B * T, C, generator=g).to(DEV)
            lens_dev = torch.tensor(lens, dtype=torch.int32, device=DEV)
            if planes:
                wp = (ops.pack_planes(weights[0]), ops.pack_planes(weights[3]))
                ref, ref_p = ops.bilstm(None, lens_dev, *weights, B, T, x_p=ops.pack_planes(x), w_ih_p=wp, want_planes=True)
            else:
                wp, ref_p = None, None
                ref = ops.bilstm(x, lens_dev, *weights, B, T)
            torch.cuda.synchronize()
            cache[key] = (x, lens_dev, wp, ref, ref_p)
        return cache[key]

    return get


@pytest.mark.parametrize("planes", [False, True], ids=["fp32", "planes"])
@pytest.mark.parametrize("with_maps", [False, True], ids=["alone", "maps"])
@pytest.mark.parametrize("slack", [0, 64 + 13], ids=["exact", "slack"])
@pytest.mark.parametrize("lens,T", [((1, 8, 3), 8), ((61, 5, 70), 70)], ids=["1-8-3", "61-5-70"])
def test_rows_form_against_the_padded_entry(lens, T, slack, with_maps, planes, weights, padded):
    from fcl_taco2_amd import engine, ops

    B, total = len(lens), sum(lens)
    n_rows = total + slack
    x, lens_dev, wp, ref, ref_p = padded(lens, T, planes)
    row0 = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    keep = np.concatenate([b * T + np.arange(n) for b, n in enumerate(lens)])  # padded row of every compact row
    keep_dev = torch.from_numpy(keep).to(DEV)
    xc = torch.randn(n_rows, C, generator=torch.Generator().manual_seed(3)).to(DEV)  # (the rows behind the total hold anything)
    xc[:total] = x[keep_dev]
    row0_dev = torch.from_numpy(row0).to(DEV)
    out = torch.full((n_rows + TAIL, 2 * H), SENTINEL, device=DEV)
    out_p = torch.full((n_rows + TAIL, 2 * H // 32 * 64), 0x5A5A, dtype=torch.int16, device=DEV) if planes else None
    req = None
    if with_maps:
        rng = np.random.RandomState(total)
        durs = [rng.randint(1, 9, size=n) for n in lens]
        dur = np.zeros(n_rows, dtype=np.int32)
        dur[:total] = np.concatenate(durs)
        pad = np.ones(n_rows, dtype=np.uint8)
        pad[:total] = 0
        m = engine.build_row_maps(list(lens), durs, T)
        st = torch.zeros(1, dtype=torch.int32, device=DEV)
        req = ops.row_maps_request(n_rows, B, m.lmax + 2, m.n_frames + 30, dur_i32=torch.from_numpy(dur).to(DEV), utt_row0=row0_dev,
                                   pad=torch.from_numpy(pad).to(DEV), want_order=True, status=st)
        for v in req.maps.values():
            v.fill_(-7)
    ops.bilstm_rows(None if planes else xc, lens_dev, row0_dev, *weights, B, n_rows, x_p=ops.pack_planes(xc) if planes else None, w_ih_p=wp,
                    row_maps=req, out=out[:n_rows], out_p=out_p[:n_rows] if planes else None)
    torch.cuda.synchronize()
    assert torch.equal(out[:total], ref[keep_dev])  # the real rows, bit for bit
    assert not out[total:n_rows].any() and (out[n_rows:] == SENTINEL).all()
    if planes:
        assert torch.equal(out_p[:total], ref_p[keep_dev])
        assert not out_p[total:n_rows].any() and (out_p[n_rows:] == 0x5A5A).all()
    if with_maps:
        d = {k: v.cpu().numpy() for k, v in req.maps.items()}
        assert int(st.item()) == 0
        assert np.array_equal(d["src_rows"][:total], m.order) and np.array_equal(d["order"][:total], m.order)
        assert np.array_equal(d["dur"][:total], m.dur_sorted) and np.array_equal(d["frame_off"][:total], m.frame_off_sorted)
        assert not d["dur"][total:].any() and sorted(d["src_rows"][total:]) == list(range(total, n_rows))  # the slack rows sort last
        assert np.array_equal(d["live_rows"][: m.lmax], m.live_rows) and not d["live_rows"][m.lmax :].any()
        assert np.array_equal(d["frame_lo"][: m.n_frames], m.frame_lo) and np.array_equal(d["frame_hi"][: m.n_frames], m.frame_hi)
        assert not d["frame_lo"][m.n_frames :].any() and not d["frame_hi"][m.n_frames :].any()
        assert list(np.diff(d["utt_frame0"])) == m.utt_frames and tuple(d["totals"][:3]) == (m.n_frames, m.lmax, 0)


def test_other_widths_are_refused(weights):
    """H = 64 has no rows form: an error, never another route."""
    from fcl_taco2_amd import _lib, ops

    g = torch.Generator().manual_seed(1)
    w = [(0.2 * torch.randn(sh, generator=g)).to(DEV) for sh in [(256, 32), (256, 64), (256,), (256, 32), (256, 64), (256,)]]
    with pytest.raises(_lib.FclError, match="H = 128"):
        ops.bilstm_rows(torch.zeros(8, 32, device=DEV), torch.tensor([3, 5], dtype=torch.int32, device=DEV),
                        torch.tensor([0, 3, 8], dtype=torch.int32, device=DEV), *w, 2, 8)
