"""Objective evaluation on the HIP path: mel-cepstral distortion, F0 RMSE and voicing error of a synthesised utterance against a reference one, over
the dynamic-time-warping path between their mel cepstra (csrc/evaluate.hip).

A student that predicts its own durations gives T' != T frames, so a frame-by-frame error against the recording is not defined; the usual figures
align the two first.  Everything is computed on this package's own analysis: log10 mels on the frame grid of features.py (or the mels `decode`
writes), F0 from pitch.py on the same grid.  The cepstra are the DCT-II of the log-mel vector in natural-log units without c_0, the local distance is
Euclidean, the warping has symmetric unit steps, MCD_dB = (10 sqrt 2 / ln 10) cost / path length.  The contract is stated in include/fcl_hip.h
"Evaluation" and restated in float64 numpy in tests/evaluate_ref.py.  Comparability with the mel-cepstra of SPTK / WORLD (the MCD other toolkits
print) stays unpinned: those libraries are not available here, and their cepstra come from another spectral envelope, warping and order.

No CPU fallback."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib, features, ops

ORDER, ORDER_MAX, FRAMES_MAX, PAIRS_MAX, N_MELS_MAX = 13, 40, 4096, 65535, 256
BATCH_CELLS = 16 << 20
MCD_SCALE = 10.0 * math.sqrt(2.0) / math.log(10.0)


def check_order(n_mels, order):
    """1 <= D <= min(n_mels - 1, 40), 2 <= n_mels <= 256; anything else is refused naming the flag"""
    if not 2 <= int(n_mels) <= N_MELS_MAX:
        raise NotImplementedError("fcl-taco2_amd: metrics: --n-mels %r is not supported (2 .. %d)" % (n_mels, N_MELS_MAX))
    if not 1 <= int(order) <= min(int(n_mels) - 1, ORDER_MAX):
        raise ValueError("fcl-taco2_amd: metrics: --order %r must lie in 1 .. min(n_mels - 1, %d) = %d" % (order, ORDER_MAX, min(int(n_mels) - 1, ORDER_MAX)))


def dct_table(n_mels, order):
    """W [D][N] float64: W[k - 1][m] = sqrt(2 / N) cos(pi k (m + 1/2) / N), k = 1 .. D (orthonormal rows; c_0 is left out)"""
    k = np.arange(1, int(order) + 1, dtype=np.float64)[:, None]
    m = np.arange(int(n_mels), dtype=np.float64)[None, :]
    return math.sqrt(2.0 / n_mels) * np.cos(np.pi * k * (m + 0.5) / n_mels)


def cepstra_table(n_mels, order, mel_stats=None):
    """(table [D][N], bias [D]) float64: c = table x + bias is ln10 W applied to the log10 mels.  mel_stats ([2, N]: mean, std) folds the
    de-normalisation x (std + 1e-8) + mean (the formula GriffinLimPlan applies) into a column scale and the bias."""
    check_order(n_mels, order)
    raw = math.log(10.0) * dct_table(n_mels, order)
    if mel_stats is None:
        return raw, np.zeros(int(order))
    st = np.asarray(mel_stats, dtype=np.float64)
    if st.shape != (2, int(n_mels)):
        raise ValueError("fcl-taco2_amd: metrics: mel_stats must be [2, %d] (mean, std), got %r" % (n_mels, st.shape))
    return raw * (st[1] + 1e-8)[None, :], raw @ st[0]


class CepstraPlan(object):
    """The cepstral transform of one side: `table` [D][N] and `bias` [D] in float64, and their float32 copies on the device."""

    def __init__(self, device, n_mels, order=ORDER, mel_stats=None):
        self.n_mels, self.order = int(n_mels), int(order)
        self.table, self.bias = cepstra_table(self.n_mels, self.order, mel_stats)
        if not str(device).startswith("cuda"):
            raise _lib.FclError("fcl-taco2_amd: CepstraPlan needs a GPU device (no CPU fallback)")
        self.device = torch.device(device)
        with torch.cuda.device(self.device):
            self.table_d = torch.from_numpy(np.ascontiguousarray(self.table, dtype=np.float32)).to(self.device)
            self.bias_d = torch.from_numpy(np.ascontiguousarray(self.bias, dtype=np.float32)).to(self.device)


class PairMaps(object):
    """The offset tables of a packed batch of pairs on the device: a_off / b_off [n + 1] int32, cell_off [n + 1] int64 (cumulative Ta Tb) and
    path_off [n + 1] int32 (cumulative Ta + Tb - 1), with their totals on the host"""

    def __init__(self, a_lens, b_lens, dev):
        self.a_lens, self.b_lens = [int(n) for n in a_lens], [int(n) for n in b_lens]
        assert len(self.a_lens) == len(self.b_lens)
        self.n_pairs = len(self.a_lens)
        cum = lambda v: np.concatenate([[0], np.cumsum(np.asarray(v, dtype=np.int64))]).astype(np.int64)
        self.a_offs, self.b_offs = cum(self.a_lens), cum(self.b_lens)
        self.cell_offs = cum([ta * tb for ta, tb in zip(self.a_lens, self.b_lens)])
        self.path_offs = cum([ta + tb - 1 for ta, tb in zip(self.a_lens, self.b_lens)])
        self.frames_a, self.frames_b, self.cells, self.path_rows = (int(v[-1]) for v in (self.a_offs, self.b_offs, self.cell_offs, self.path_offs))
        self.max_ta, self.max_tb = max(self.a_lens + [0]), max(self.b_lens + [0])
        t = lambda a, dt: torch.from_numpy(a.astype(dt)).to(dev)
        self.a_off, self.b_off, self.path_off = t(self.a_offs, np.int32), t(self.b_offs, np.int32), t(self.path_offs, np.int32)
        self.cell_off = t(self.cell_offs, np.int64)

    def workspace_bytes(self):
        return int(_lib.load().fcl_ev_dtw_workspace_bytes(self.cells, self.n_pairs))


# one launch each, on caller-owned buffers (the tests surround them with guard zones)
def launch_cepstra(pl, x, c, frames):
    """x [frames][n_mels] float32 -> c [frames][order] float32"""
    _lib.check(_lib.load().fcl_ev_cepstra_fwd(x.data_ptr(), pl.table_d.data_ptr(), pl.bias_d.data_ptr(), c.data_ptr(), int(frames), pl.n_mels, pl.order,
                                              ops._stream()))


def _args(mp, order, **ptr):
    a = _lib.Evaluate()
    a.frames_a, a.frames_b, a.cells, a.path_rows = mp.frames_a, mp.frames_b, mp.cells, mp.path_rows
    a.n_pairs, a.d, a.max_ta, a.max_tb = mp.n_pairs, int(order), mp.max_ta, mp.max_tb
    a.a_off, a.b_off, a.cell_off, a.path_off = mp.a_off.data_ptr(), mp.b_off.data_ptr(), mp.cell_off.data_ptr(), mp.path_off.data_ptr()
    for k, v in ptr.items():
        setattr(a, k, None if v is None else v.data_ptr())
    return a


def launch_dtw(mp, order, a, b, workspace, path, path_len, cost):
    """a [frames_a][order], b [frames_b][order] float32 -> path [path_rows][2] int32 (each pair's cells in forward order, -1 past its length),
    path_len [n_pairs] int32, cost [n_pairs] float32 = C(Ta - 1, Tb - 1); workspace: uint8, PairMaps.workspace_bytes() of it"""
    args = _args(mp, order, a=a, b=b, workspace=workspace, path=path, path_len=path_len, cost=cost)
    args.workspace_bytes = int(workspace.numel() * workspace.element_size())
    _lib.check(_lib.load().fcl_ev_dtw_fwd(C.byref(args), ops._stream()))


def launch_path_pitch(mp, path, path_len, pitch_a, pitch_b, counts, sums):
    """pitch_a [frames_a], pitch_b [frames_b] float32 cents (0 = unvoiced) over the paths -> counts [n_pairs][2] int32 (n_vv, n_vuv), sums [n_pairs]"""
    _lib.check(_lib.load().fcl_ev_path_pitch_fwd(C.byref(_args(mp, 1, path=path, path_len=path_len, pitch_a=pitch_a, pitch_b=pitch_b, counts=counts,
                                                               sums=sums)), ops._stream()))


def cents(f0):
    """F0 in Hz (device tensor, 0 = unvoiced) -> cents above 1 Hz, 1200 log2 f0, 0 where unvoiced"""
    f0 = f0.to(torch.float32)
    return torch.where(f0 > 0, 1200.0 * torch.log2(torch.clamp(f0, min=1e-30)), torch.zeros_like(f0))


def check_pairs(ref_lens, syn_lens, ids=None):
    """Every utterance needs 1 .. 4096 frames on either side; the first other one is refused by id (its position without ids)."""
    if len(ref_lens) != len(syn_lens):
        raise _lib.FclError("fcl-taco2_amd: metrics: %d reference and %d synthesised utterances" % (len(ref_lens), len(syn_lens)))
    for i, (ta, tb) in enumerate(zip(ref_lens, syn_lens)):
        if not (1 <= int(ta) <= FRAMES_MAX and 1 <= int(tb) <= FRAMES_MAX):
            raise ValueError("fcl-taco2_amd: metrics: utterance %s has %d reference and %d synthesised frames; the alignment covers 1 .. %d frames on "
                             "either side" % (ids[i] if ids is not None else "#%d" % i, int(ta), int(tb), FRAMES_MAX))


def pair_batches(ref_lens, syn_lens, batch_cells):
    """consecutive runs of pairs whose cells sum to at most batch_cells (a larger single pair goes alone), at most 65535 pairs each"""
    out, cur, cells = [], [], 0
    for i, (ta, tb) in enumerate(zip(ref_lens, syn_lens)):
        c = int(ta) * int(tb)
        if cur and (cells + c > batch_cells or len(cur) >= PAIRS_MAX):
            out.append(cur)
            cur, cells = [], 0
        cur.append(i)
        cells += c
    return out + ([cur] if cur else [])


def figures(cost, path_len, counts=None, sums=None):
    """the per-pair figures from what the kernels return, in float64 on the host"""
    n = np.asarray(path_len, dtype=np.float64)
    out = dict(path_len=np.asarray(path_len, dtype=np.int64), cost=np.asarray(cost, dtype=np.float64))
    out["mcd_db"] = MCD_SCALE * out["cost"] / n
    if counts is not None:
        counts = np.asarray(counts, dtype=np.int64).reshape(-1, 2)
        vv = counts[:, 0].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            out["f0_rmse_cents"] = np.where(vv > 0, np.sqrt(np.asarray(sums, dtype=np.float64) / vv), np.nan)
        out["vuv_error"] = counts[:, 1] / n
        out["n_vv"], out["n_vuv"] = counts[:, 0], counts[:, 1]
    return out


def _track(f0, lens, dev, ids, side):
    """per-utterance F0 tracks (or one packed tensor) -> packed float32 on the device; a track whose length is not its mel's frame count is refused by id"""
    if isinstance(f0, (list, tuple)):
        if len(f0) != len(lens):
            raise _lib.FclError("fcl-taco2_amd: metrics: %d %s F0 tracks for %d utterances" % (len(f0), side, len(lens)))
        for i, (v, n) in enumerate(zip(f0, lens)):
            if int(np.prod(tuple(v.shape))) != int(n):
                raise ValueError("fcl-taco2_amd: metrics: utterance %s: the %s F0 track has %d frames, its mel has %d"
                                 % (ids[i] if ids is not None else "#%d" % i, side, int(np.prod(tuple(v.shape))), int(n)))
        f0 = torch.cat([torch.as_tensor(v).reshape(-1).to(device=dev, dtype=torch.float32) for v in f0])
    f0 = torch.as_tensor(f0).to(device=dev, dtype=torch.float32).contiguous().reshape(-1)
    if f0.numel() != sum(lens):
        raise _lib.FclError("fcl-taco2_amd: metrics: the packed %s F0 has %d frames, lens sum to %d" % (side, f0.numel(), sum(lens)))
    return f0


class Evaluator(object):
    """MCD / F0 RMSE / voicing error of synthesised against reference utterances.  ref_stats / syn_stats ([2, n_mels]: mean, std) say that that
    side's mels are normalised with them.  extractor (features.FeatureExtractor), tracker (pitch.PitchTracker, optional) and resampler_for (input rate
    -> resample.Resampler, e.g. a ResamplerCache) serve compare_waves."""

    def __init__(self, device, n_mels=80, order=ORDER, ref_stats=None, syn_stats=None, extractor=None, tracker=None, resampler_for=None,
                 batch_cells=BATCH_CELLS):
        if not str(device).startswith("cuda"):
            raise _lib.FclError("fcl-taco2_amd: Evaluator needs a GPU device (no CPU fallback)")
        if batch_cells < 1:
            raise ValueError("fcl-taco2_amd: metrics: --batch-cells must be positive (got %r)" % (batch_cells,))
        if extractor is not None and extractor.plan.A != int(n_mels):
            raise ValueError("fcl-taco2_amd: metrics: the feature extractor gives %d mels, the evaluation is set up for %d" % (extractor.plan.A, int(n_mels)))
        if extractor is not None and extractor.plan.mel_stats is not None:
            raise ValueError("fcl-taco2_amd: metrics: the feature extractor must give raw log10 mels (no mel_stats)")
        self.device, self.n_mels, self.order, self.batch_cells = torch.device(device), int(n_mels), int(order), int(batch_cells)
        self.raw_plan = CepstraPlan(device, n_mels, order)
        self.ref_plan = self.raw_plan if ref_stats is None else CepstraPlan(device, n_mels, order, ref_stats)
        self.syn_plan = self.raw_plan if syn_stats is None else CepstraPlan(device, n_mels, order, syn_stats)
        self.extractor, self.tracker, self.resampler_for = extractor, tracker, resampler_for

    def _rows(self, rows, lens, side, ids):
        rows = torch.as_tensor(rows)
        if rows.dim() != 2 or rows.shape[1] != self.n_mels:
            raise ValueError("fcl-taco2_amd: metrics: the %s mels%s are %r; [frames, n_mels = %d] expected (mismatched n_mels)"
                             % (side, "" if ids is None else " of %s .. %s" % (ids[0], ids[-1]), tuple(rows.shape), self.n_mels))
        if rows.shape[0] != sum(lens):
            raise _lib.FclError("fcl-taco2_amd: metrics: the packed %s mels have %d rows, lens sum to %d" % (side, rows.shape[0], sum(lens)))
        return rows.to(device=self.device, dtype=torch.float32).contiguous()

    def cepstra(self, plan, rows):
        """mel rows [frames, n_mels] on the device -> cepstra [frames, order]: ONE launch"""
        c = torch.empty(rows.shape[0], plan.order, device=self.device, dtype=torch.float32)
        launch_cepstra(plan, rows, c, rows.shape[0])
        return c

    def compare_mels(self, ref_rows, ref_lens, syn_rows, syn_lens, ref_f0=None, syn_f0=None, ids=None, return_paths=False, raw=False,
                     return_cepstra=False):
        """ref_rows [sum Ta, n_mels] / syn_rows [sum Tb, n_mels]: the utterances' mel rows back to back (device tensors or arrays) with their frame
        counts; ref_f0 / syn_f0: frame-level F0 in Hz, 0 = unvoiced (per-utterance tracks or one packed vector; both or neither).  raw (one flag, or
        one per side): the rows are raw log10 mels whatever statistics the evaluator holds (compare_waves).  -> dict of per-pair arrays: mcd_db, path_len, cost (+ f0_rmse_cents,
        vuv_error, n_vv, n_vuv with F0; + paths, a list of [n, 2] int arrays, with return_paths; + ref_cepstra / syn_cepstra / ref_cents / syn_cents
        with return_cepstra).  Per batch of at most batch_cells cells: two cepstra launches, one DTW launch, one pitch launch."""
        dev = self.device
        ref_lens, syn_lens = [int(n) for n in ref_lens], [int(n) for n in syn_lens]
        check_pairs(ref_lens, syn_lens, ids)
        if (ref_f0 is None) != (syn_f0 is None):
            raise _lib.FclError("fcl-taco2_amd: metrics: F0 on one side only")
        with torch.cuda.device(dev):
            ref_rows, syn_rows = self._rows(ref_rows, ref_lens, "reference", ids), self._rows(syn_rows, syn_lens, "synthesised", ids)
            pa = pb = None
            if ref_f0 is not None:
                pa, pb = cents(_track(ref_f0, ref_lens, dev, ids, "reference")), cents(_track(syn_f0, syn_lens, dev, ids, "synthesised"))
            raw_a, raw_b = (raw, raw) if isinstance(raw, bool) else raw
            ca = self.cepstra(self.raw_plan if raw_a else self.ref_plan, ref_rows) if ref_rows.shape[0] else None
            cb = self.cepstra(self.raw_plan if raw_b else self.syn_plan, syn_rows) if syn_rows.shape[0] else None
            ao, bo = np.concatenate([[0], np.cumsum(ref_lens)]).astype(np.int64), np.concatenate([[0], np.cumsum(syn_lens)]).astype(np.int64)
            parts, paths = [], []
            for idx in pair_batches(ref_lens, syn_lens, self.batch_cells):  # consecutive pairs: slices of the packed cepstra
                i0, i1 = idx[0], idx[-1] + 1
                mp = PairMaps(ref_lens[i0:i1], syn_lens[i0:i1], dev)
                ws = torch.empty(mp.workspace_bytes(), device=dev, dtype=torch.uint8)
                path = torch.empty(mp.path_rows, 2, device=dev, dtype=torch.int32)
                path_len = torch.empty(mp.n_pairs, device=dev, dtype=torch.int32)
                cost = torch.empty(mp.n_pairs, device=dev, dtype=torch.float32)
                launch_dtw(mp, self.order, ca[ao[i0] : ao[i1]], cb[bo[i0] : bo[i1]], ws, path, path_len, cost)
                counts = sums = None
                if pa is not None:
                    counts = torch.empty(mp.n_pairs, 2, device=dev, dtype=torch.int32)
                    sums = torch.empty(mp.n_pairs, device=dev, dtype=torch.float32)
                    launch_path_pitch(mp, path, path_len, pa[ao[i0] : ao[i1]], pb[bo[i0] : bo[i1]], counts, sums)
                n = path_len.cpu().numpy()
                parts.append(figures(cost.cpu().numpy(), n, None if counts is None else counts.cpu().numpy(), None if sums is None else sums.cpu().numpy()))
                if return_paths:
                    host = path.cpu().numpy()
                    paths += [host[mp.path_offs[k] : mp.path_offs[k] + n[k]].copy() for k in range(mp.n_pairs)]
        out = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]} if parts else figures(np.zeros(0), np.zeros(0, np.int64))
        if return_paths:
            out["paths"] = paths
        if return_cepstra:
            out.update(ref_cepstra=ca, syn_cepstra=cb, ref_cents=pa, syn_cents=pb)
        return out

    def at_analysis_rate(self, waves, rates=None, ids=None):
        """list of 1-D float waveforms -> (the same as float32 device tensors at the analysis rate, their sample counts): those whose rate (rates)
        is another one go through resampler_for, one packed launch per rate"""
        fx, dev = self.extractor, self.device
        if fx is None:
            raise _lib.FclError("fcl-taco2_amd: metrics: compare_waves needs a feature extractor")
        xs = [torch.as_tensor(np.asarray(w, dtype=np.float32).reshape(-1)).to(dev) for w in waves]
        lens = [int(x.numel()) for x in xs]
        if rates is not None:
            groups = {}
            for i, r in enumerate(rates):
                if int(r) != fx.plan.fs:
                    groups.setdefault(int(r), []).append(i)
            if groups and self.resampler_for is None:
                raise ValueError("fcl-taco2_amd: metrics: utterance %s is sampled at %d Hz, the analysis at %d Hz (--resample resamples on the device)"
                                 % (ids[min(min(g) for g in groups.values())] if ids is not None else "#?", sorted(groups)[0], fx.plan.fs))
            for r, g in groups.items():
                y, out_lens = self.resampler_for(r).resample_packed(torch.cat([xs[i] for i in g]), [lens[i] for i in g])
                o = np.concatenate([[0], np.cumsum(out_lens)])
                for k, i in enumerate(g):
                    xs[i], lens[i] = y[int(o[k]) : int(o[k + 1])], int(out_lens[k])
        return xs, lens

    def analyse(self, waves, rates=None, ids=None):
        """list of 1-D float waveforms (rates: their sampling rates where they are not the analysis rate; needs resampler_for) -> (mel rows
        [sum T, n_mels] raw log10, frame counts, F0 [sum T] Hz or None without a tracker): the mel launch and the tracker's two on shared Maps"""
        fx, dev = self.extractor, self.device
        xs, lens = self.at_analysis_rate(waves, rates, ids)
        fx.check_lens(lens, ids)
        if self.tracker is not None:
            self.tracker.check_lens(lens, ids)
        with torch.cuda.device(dev):
            x = torch.cat(xs)
            mp = features.Maps(lens, fx.plan.hop, dev)
            mel, _, T = fx.extract_packed(x, lens, ids=ids, maps=mp)
            f0 = None if self.tracker is None else self.tracker.track_packed(x, lens, ids=ids, maps=mp)[0]
        return mel, list(T), f0

    def compare_waves(self, ref_waves, syn_waves, ids=None, ref_rates=None, syn_rates=None, return_paths=False, return_cepstra=False):
        """Waveforms in [-1, 1] on either side -> compare_mels on this package's own log10 mels and, with a tracker, its own F0 tracks."""
        if len(ref_waves) != len(syn_waves):
            raise _lib.FclError("fcl-taco2_amd: metrics: %d reference and %d synthesised waveforms" % (len(ref_waves), len(syn_waves)))
        ra, la, fa = self.analyse(ref_waves, ref_rates, ids)
        rb, lb, fb = self.analyse(syn_waves, syn_rates, ids)
        return self.compare_mels(ra, la, rb, lb, fa, fb, ids=ids, return_paths=return_paths, raw=True, return_cepstra=return_cepstra)
