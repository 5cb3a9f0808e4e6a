"""Objective evaluation driver on MI355X: synthesised utterances against reference ones, on fcl_taco2_amd/metrics.py.

    python -m fcl_taco2_amd.evaluate --ref-wav-dir wavs --syn-wav-dir tts_out --out metrics.json
    python -m fcl_taco2_amd.evaluate --ref-mel-dir feats/mels-ori --syn-feats-scp decode_out/feats.scp --mel-stats feats/mel_stats.npy --syn-normalised

Each side takes one source: a directory of 16-bit PCM mono wavs (`<utt>.wav`, or `<utt>_gen.wav` as `tts` writes them), a directory of mels
(`<utt>.npy`, [T, n_mels] log10 mels as `extract_features` writes them) or the ark / scp `decode` writes.  `--mel-stats` with `--ref-normalised` /
`--syn-normalised` says which side's mels are normalised with those statistics; wavs go through this package's own analysis (features.py, and pitch.py
when both sides are wavs; `--resample` for files at another rate).  Utterances are paired by id; an id present on one side only is refused before the
first device call, as is a pair longer than 4096 frames.  Pairs are batched by their cells Ta Tb (`--batch-cells`).

Per utterance: mel-cepstral distortion in dB over the DTW path of the order-`--order` mel cepstra and the path length; with wavs on both sides also
the F0 RMSE in cents over the cells voiced on both sides, the share of cells voiced on one side only and the count of the former.  `--out` holds
these records, the corpus figures (MCD and V/UV error: the mean of the per-utterance values; F0 RMSE: the mean over the utterances with n_vv > 0),
n_utt and the settings; one summary line goes to stdout.  The MCD is this package's own: comparability with SPTK / WORLD mel-cepstra is unpinned.

`--aligned` (wavs on both sides) adds the figure for time-aligned pairs -- copy-synthesis: a vocoder run on a recording's own mel -- where a DTW
path is the wrong tool: the multi-resolution STFT distance of stft_loss.py, spectral convergence and log-magnitude distance over the
`--stft-*` resolutions (Parallel WaveGAN's by default).  Each pair is cut to its shorter side; a pair whose lengths differ by more than
`--aligned-max-diff` samples (default: two hops of the analysis) is refused by id before the first device call.  Every record gains `stft_sc`,
`stft_log_mag` (the means over the resolutions), `stft` (per resolution) and `aligned_samples`; the document gains the corpus means of the first two.  `--aligned-mel` (with `--aligned`) adds `mel_l1`, the
mel-spectrogram L1 distance of mel_loss.py on the log10 mels of the analysis flags -- the distance in the acoustic model's own output
space -- to the records, its corpus mean to the document and one clause to the summary line.
"""
import argparse
import json
import logging
import math
import os
import struct

import numpy as np
import torch

from . import extract_features as X, features, griffinlim, kaldi_io, mel_loss, metrics, pitch, resample, stft_loss

SIDES = ("ref", "syn")


def _mat_shape(ark_path, offset):
    """(rows, cols) of a Kaldi binary float matrix from its header alone"""
    with open(ark_path, "rb") as f:
        f.seek(offset)
        head = f.read(15)
    if len(head) != 15 or head[:5] != b"\0BFM " or head[5:6] != b"\x04" or head[10:11] != b"\x04":
        raise ValueError("%s:%d: not a binary float matrix" % (ark_path, offset))
    return struct.unpack("<i", head[6:10])[0], struct.unpack("<i", head[11:15])[0]


class Source(object):
    """One side's utterances: kind "wav" / "mel" / "scp", {id: where}"""

    def __init__(self, kind, where, items):
        self.kind, self.where, self.items = kind, where, items

    def ids(self):
        return set(self.items)

    def mel_shape(self, u):
        if self.kind == "mel":
            return tuple(np.load(self.items[u], mmap_mode="r").shape)
        return _mat_shape(*self.items[u])

    def mel(self, u):
        return np.asarray(np.load(self.items[u]) if self.kind == "mel" else kaldi_io.read_mat(*self.items[u]), dtype=np.float32)


def read_source(wav_dir=None, mel_dir=None, feats_scp=None):
    if wav_dir is not None:
        items = {}
        for n in sorted(os.listdir(wav_dir)):
            if n.lower().endswith(".wav"):
                u = n[:-4]
                u = u[:-4] if u.endswith("_gen") else u
                if u in items:
                    raise ValueError("%s: both %s.wav and %s_gen.wav" % (wav_dir, u, u))
                items[u] = os.path.join(wav_dir, n)
        src = Source("wav", wav_dir, items)
    elif mel_dir is not None:
        src = Source("mel", mel_dir, {n[:-4]: os.path.join(mel_dir, n) for n in sorted(os.listdir(mel_dir)) if n.endswith(".npy")})
    else:
        items = {}
        with open(feats_scp) as f:
            for ln in f:
                if ln.strip():
                    key, loc = ln.strip().split(None, 1)
                    path, off = loc.rsplit(":", 1)
                    items[key] = (path, int(off))
        src = Source("scp", feats_scp, items)
    if not src.items:
        raise ValueError("no utterances in %s" % src.where)
    return src


def pair_ids(ref, syn):
    """the ids of both sides, sorted; an id on one side only is refused by name"""
    only_ref, only_syn = sorted(ref.ids() - syn.ids()), sorted(syn.ids() - ref.ids())
    if only_ref or only_syn:
        raise ValueError("unpaired utterances: %d only in %s (first: %s), %d only in %s (first: %s)"
                         % (len(only_ref), ref.where, only_ref[0] if only_ref else "-", len(only_syn), syn.where, only_syn[0] if only_syn else "-"))
    return sorted(ref.ids())


def frame_counts(src, ids, fs, hop, n_mels, resampling):
    """frames per utterance from the headers alone (wavs: after resampling, in integers) -> (frames, rates or None); a mel of another width is
    refused by id"""
    frames, rates = [], [] if src.kind == "wav" else None
    for u in ids:
        if src.kind == "wav":
            rate, n = X.wav_rate_and_samples(src.items[u])
            if rate != fs:
                if not resampling:
                    raise ValueError("%s: sampling rate %d, --fs is %d (--resample resamples on the device)" % (src.items[u], rate, fs))
                L, M, _ = resample.check_rates(rate, fs)
                n = resample.out_samples(n, L, M)
            rates.append(rate)
            frames.append(features.frames_of(n, hop))
        else:
            shape = src.mel_shape(u)
            if len(shape) != 2 or shape[1] != n_mels:
                raise ValueError("utterance %s: the mel in %s is %r; [T, n_mels = %d] expected (mismatched n_mels)" % (u, src.where, tuple(shape), n_mels))
            frames.append(int(shape[0]))
    return frames, rates


def sample_counts(src, ids, fs, resampling):
    """samples per utterance of a wav source at the analysis rate, from the headers alone (after resampling, in integers)"""
    out = []
    for u in ids:
        rate, n = X.wav_rate_and_samples(src.items[u])
        if rate != fs and resampling:
            L, M, _ = resample.check_rates(rate, fs)
            n = resample.out_samples(n, L, M)
        out.append(int(n))
    return out


def check_aligned(ids, ref_samples, syn_samples, max_diff, n_fft):
    """-> the pairs' common lengths (the shorter side).  A pair whose lengths differ by more than max_diff samples is no time-aligned pair, and one
    shorter than n_fft / 2 + 1 (n_fft: the largest resolution) has no single reflection: the first such pair is refused by id."""
    out = []
    for u, a, b in zip(ids, ref_samples, syn_samples):
        if abs(int(a) - int(b)) > max_diff:
            raise ValueError("fcl-taco2_amd: evaluate: utterance %s has %d reference and %d synthesised samples; --aligned compares time-aligned pairs "
                             "and allows a difference of %d samples (--aligned-max-diff)" % (u, int(a), int(b), max_diff))
        out.append(min(int(a), int(b)))
    features.check_lens(out, n_fft, ids)
    return out


def sample_batches(lens, batch_samples):
    """consecutive runs of pairs whose samples sum to at most batch_samples (a longer single pair goes alone)"""
    out, cur, tot = [], [], 0
    for i, n in enumerate(lens):
        if cur and tot + n > batch_samples:
            out.append(cur)
            cur, tot = [], 0
        cur.append(i)
        tot += n
    return out + ([cur] if cur else [])


def add_aligned(records, sc, mag, lens, configs):
    """the per-utterance records gain the multi-resolution STFT figures (sc, mag [n_utt, R])"""
    for r, s, m, n in zip(records, sc, mag, lens):
        r.update(stft_sc=float(np.mean(s)), stft_log_mag=float(np.mean(m)), aligned_samples=int(n),
                 stft=[dict(n_fft=c[0], hop=c[1], win_length=c[2], sc=float(a), log_mag=float(b)) for c, a, b in zip(configs, s, m)])


def add_aligned_mel(records, d):
    """the per-utterance records gain the mel-spectrogram L1 distance (d [n_utt, 1]: the analysis flags' single resolution)"""
    for r, v in zip(records, d):
        r["mel_l1"] = float(np.mean(v))


def summarise(records, settings):
    """The --out document from the per-utterance records (dicts with id, ref_frames, syn_frames, path_len, mcd_db and, with F0, f0_rmse_cents (None
    for n_vv = 0), vuv_error, n_vv): corpus MCD and V/UV error are the means of the per-utterance values, the F0 RMSE the mean over the utterances
    with n_vv > 0 (None when there is none)."""
    mean = lambda v: float(np.mean(v)) if len(v) else None
    doc = dict(n_utt=len(records), mcd_db=mean([r["mcd_db"] for r in records]))
    if records and "vuv_error" in records[0]:
        doc["vuv_error"] = mean([r["vuv_error"] for r in records])
        voiced = [r["f0_rmse_cents"] for r in records if r["n_vv"] > 0]
        doc["f0_rmse_cents"], doc["n_utt_voiced"] = mean(voiced), len(voiced)
    if records and "stft_sc" in records[0]:
        doc["stft_sc"], doc["stft_log_mag"] = mean([r["stft_sc"] for r in records]), mean([r["stft_log_mag"] for r in records])
    if records and "mel_l1" in records[0]:
        doc["mel_l1"] = mean([r["mel_l1"] for r in records])
    doc["settings"], doc["utterances"] = settings, records
    return doc


def records_of(ids, ref_frames, syn_frames, res):
    out = []
    for k, u in enumerate(ids):
        r = dict(id=u, ref_frames=int(ref_frames[k]), syn_frames=int(syn_frames[k]), path_len=int(res["path_len"][k]), mcd_db=float(res["mcd_db"][k]))
        if "vuv_error" in res:
            v = float(res["f0_rmse_cents"][k])
            r.update(f0_rmse_cents=None if math.isnan(v) else v, vuv_error=float(res["vuv_error"][k]), n_vv=int(res["n_vv"][k]))
        out.append(r)
    return out


def summary_line(doc):
    s = "evaluate: %d utterances, MCD %.3f dB" % (doc["n_utt"], doc["mcd_db"])
    if "vuv_error" in doc:
        s += ", F0 RMSE %s cents over %d utterances, V/UV error %.2f %%" % ("%.1f" % doc["f0_rmse_cents"] if doc["f0_rmse_cents"] is not None else "n/a",
                                                                             doc["n_utt_voiced"], 100.0 * doc["vuv_error"])
    if "stft_sc" in doc:
        s += ", STFT spectral convergence %.4f, log-magnitude %.4f" % (doc["stft_sc"], doc["stft_log_mag"])
    if "mel_l1" in doc:
        s += ", mel L1 %.4f" % doc["mel_l1"]
    return s


def build_parser():
    ap = argparse.ArgumentParser(prog="fcl_taco2_amd.evaluate", description="DTW-aligned mel-cepstral distortion and F0 error of synthesised against reference utterances on MI355X")
    for side, what in zip(SIDES, ("reference", "synthesised")):
        g = ap.add_mutually_exclusive_group(required=True)
        g.add_argument("--%s-wav-dir" % side, default=None, metavar="DIR", help="the %s utterances as <utt>.wav or <utt>_gen.wav (16-bit PCM mono)" % what)
        g.add_argument("--%s-mel-dir" % side, default=None, metavar="DIR", help="the %s utterances as <utt>.npy [T, n_mels] log10 mels" % what)
        g.add_argument("--%s-feats-scp" % side, default=None, metavar="FILE", help="the %s utterances as the scp `decode` writes" % what)
        ap.add_argument("--%s-normalised" % side, action="store_true", help="the %s mels are normalised with --mel-stats" % what)
    ap.add_argument("--mel-stats", default=None, metavar="FILE.npy", help="mel_stats.npy of the preprocessing ([2, n_mels]: mean, std)")
    ap.add_argument("--order", type=int, default=metrics.ORDER, help="cepstral coefficients c_1 .. c_order (at most min(n_mels - 1, %d))" % metrics.ORDER_MAX)
    ap.add_argument("--batch-cells", type=int, default=metrics.BATCH_CELLS, help="cells Ta x Tb per GPU batch")
    ap.add_argument("--out", default=None, metavar="FILE.json", help="per-utterance records, corpus figures and settings")
    ap.add_argument("--resample", action="store_true", help="resample wavs whose rate is not --fs on the GPU instead of refusing them")
    ap.add_argument("--n-mels", type=int, default=griffinlim.DEFAULTS["n_mels"])
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--verbose", type=int, default=1)
    g = ap.add_argument_group("analysis of the wav sources (the defaults are the reference's preprocessing)")
    g.add_argument("--mel-basis", default=None, metavar="FILE.npy", help="[n_mels, n_fft / 2 + 1] mel filterbank replacing the built Slaney one")
    griffinlim.add_analysis_arguments(g)
    pitch.add_pitch_arguments(ap.add_argument_group("F0 tracking (both sides wavs)"))
    g = ap.add_argument_group("time-aligned pairs (both sides wavs): the multi-resolution STFT distance")
    g.add_argument("--aligned", action="store_true", help="the pairs are time-aligned (copy-synthesis): add spectral convergence and log-magnitude distance")
    g.add_argument("--aligned-max-diff", type=int, default=None, metavar="SAMPLES", help="largest length difference of a pair (default: 2 x --hop)")
    g.add_argument("--aligned-batch-samples", type=int, default=1 << 22, metavar="SAMPLES", help="samples per GPU batch of the STFT distance")
    stft_loss.add_arguments(g)
    g.add_argument("--aligned-mel", action="store_true", help="with --aligned: add the mel-spectrogram L1 distance (log10 mels of the analysis flags above)")
    return ap


def parse_args(argv=None):
    """Parses and checks what can be checked before the first device call; flag errors end in ap.error (SystemExit 2)."""
    ap = build_parser()
    args = ap.parse_args(argv)
    for side in SIDES:
        d = vars(args)
        if d["%s_normalised" % side] and d["%s_wav_dir" % side] is not None:
            ap.error("--%s-normalised applies to mels, not to --%s-wav-dir" % (side, side))
        if d["%s_normalised" % side] and args.mel_stats is None:
            ap.error("--%s-normalised needs --mel-stats" % side)
        for flag in ("wav_dir", "mel_dir"):
            v = d["%s_%s" % (side, flag)]
            if v is not None and not os.path.isdir(v):
                ap.error("--%s-%s %s is not a directory" % (side, flag.replace("_", "-"), v))
        if d["%s_feats_scp" % side] is not None and not os.path.isfile(d["%s_feats_scp" % side]):
            ap.error("--%s-feats-scp %s is not a file" % (side, d["%s_feats_scp" % side]))
    if args.mel_stats is not None and not (args.ref_normalised or args.syn_normalised):
        ap.error("--mel-stats needs --ref-normalised and / or --syn-normalised: which side it applies to")
    for flag, p in (("--mel-stats", args.mel_stats), ("--mel-basis", args.mel_basis)):
        if p is not None and not os.path.isfile(p):
            ap.error("%s %s is not a file" % (flag, p))
    if args.batch_cells < 1:
        ap.error("--batch-cells must be positive")
    try:
        metrics.check_order(args.n_mels, args.order)
        griffinlim.check_config(args.n_fft, args.hop, args.n_fft if args.win_length is None else args.win_length, args.n_mels, args.fs, args.fmin, args.fmax)
    except (NotImplementedError, ValueError) as e:
        ap.error(str(e))
    if args.ref_wav_dir is not None and args.syn_wav_dir is not None:
        pitch.check_arguments(ap, args)
    if args.aligned and (args.ref_wav_dir is None or args.syn_wav_dir is None):
        ap.error("--aligned compares waveforms: it needs --ref-wav-dir and --syn-wav-dir")
    if args.aligned_mel and not args.aligned:
        ap.error("--aligned-mel is a figure of time-aligned pairs: it needs --aligned")
    try:
        stft_loss.check_resolutions(args.stft_fft_sizes, args.stft_hops, args.stft_win_lengths)
    except (NotImplementedError, ValueError) as e:
        ap.error("--stft-fft-sizes / --stft-hops / --stft-win-lengths: %s" % e)
    if args.aligned_max_diff is None:
        args.aligned_max_diff = 2 * args.hop
    if args.aligned_max_diff < 0 or args.aligned_batch_samples < 1:
        ap.error("--aligned-max-diff must not be negative and --aligned-batch-samples must be positive")
    return args


def evaluate(args):
    """-> the --out document"""
    ref = read_source(args.ref_wav_dir, args.ref_mel_dir, args.ref_feats_scp)
    syn = read_source(args.syn_wav_dir, args.syn_mel_dir, args.syn_feats_scp)
    ids = pair_ids(ref, syn)
    fa, ra = frame_counts(ref, ids, args.fs, args.hop, args.n_mels, args.resample)
    fb, rb = frame_counts(syn, ids, args.fs, args.hop, args.n_mels, args.resample)
    metrics.check_pairs(fa, fb, ids)  # refused by id before the first device call
    aligned_lens = None
    if args.aligned:
        configs = stft_loss.check_resolutions(args.stft_fft_sizes, args.stft_hops, args.stft_win_lengths)
        aligned_lens = check_aligned(ids, sample_counts(ref, ids, args.fs, args.resample), sample_counts(syn, ids, args.fs, args.resample),
                                     args.aligned_max_diff, max(c[0] for c in configs))
    stats = None if args.mel_stats is None else np.load(args.mel_stats)
    any_wav, both_wav = "wav" in (ref.kind, syn.kind), ref.kind == syn.kind == "wav"
    fx = features.from_args(args, args.device) if any_wav else None
    ev = metrics.Evaluator(args.device, args.n_mels, args.order, ref_stats=stats if args.ref_normalised else None,
                           syn_stats=stats if args.syn_normalised else None, extractor=fx, tracker=pitch.from_args(args, args.device) if both_wav else None,
                           resampler_for=resample.ResamplerCache(args.device, args.fs) if args.resample and any_wav else None, batch_cells=args.batch_cells)

    def side(src, rates, idx, bid):
        """-> (mel rows, frame counts, F0 or None, raw)"""
        if src.kind == "wav":
            waves = [X.read_wav(src.items[u], rates[i]) for u, i in zip(bid, idx)]
            return ev.analyse(waves, [rates[i] for i in idx], bid) + (True,)
        mels = [src.mel(u) for u in bid]
        return np.concatenate(mels), [len(m) for m in mels], None, False

    records = []
    for idx in metrics.pair_batches(fa, fb, args.batch_cells):
        bid = [ids[i] for i in idx]
        rows_a, la, f0_a, raw_a = side(ref, ra, idx, bid)
        rows_b, lb, f0_b, raw_b = side(syn, rb, idx, bid)
        if la != [fa[i] for i in idx] or lb != [fb[i] for i in idx]:
            raise RuntimeError("evaluate: the frame counts read do not match the headers' (%r)" % (bid,))
        res = ev.compare_mels(rows_a, la, rows_b, lb, f0_a if both_wav else None, f0_b if both_wav else None, ids=bid, raw=(raw_a, raw_b))
        records += records_of(bid, la, lb, res)
    settings = dict(order=args.order, n_mels=args.n_mels, ref=dict(kind=ref.kind, source=ref.where, normalised=bool(args.ref_normalised)),
                    syn=dict(kind=syn.kind, source=syn.where, normalised=bool(args.syn_normalised)), mel_stats=args.mel_stats, batch_cells=args.batch_cells,
                    analysis=dict(fs=args.fs, n_fft=args.n_fft, hop=args.hop, win_length=args.win_length, fmin=args.fmin, fmax=args.fmax, resample=bool(args.resample)))
    if args.aligned:
        loss = stft_loss.MultiResolutionSTFTLoss(args.device, args.stft_fft_sizes, args.stft_hops, args.stft_win_lengths)
        mel = mel_loss.from_args(args, args.device) if args.aligned_mel else None
        for idx in sample_batches(aligned_lens, args.aligned_batch_samples):
            bid, n = [ids[i] for i in idx], [aligned_lens[i] for i in idx]
            xa, la = ev.at_analysis_rate([X.read_wav(ref.items[u], ra[i]) for u, i in zip(bid, idx)], [ra[i] for i in idx], bid)
            xb, lb = ev.at_analysis_rate([X.read_wav(syn.items[u], rb[i]) for u, i in zip(bid, idx)], [rb[i] for i in idx], bid)
            if [min(a, b) for a, b in zip(la, lb)] != n:
                raise RuntimeError("evaluate: the sample counts read do not match the headers' (%r)" % (bid,))
            sc, mag = loss.distances(torch.cat([v[:k] for v, k in zip(xb, n)]), n, torch.cat([v[:k] for v, k in zip(xa, n)]), ids=bid)
            add_aligned([records[i] for i in idx], sc, mag, n, configs)
            if mel is not None:
                add_aligned_mel([records[i] for i in idx], mel.distances(torch.cat([v[:k] for v, k in zip(xb, n)]), n, torch.cat([v[:k] for v, k in zip(xa, n)]),
                                                                         ids=bid))
        settings["aligned"] = dict(max_diff=args.aligned_max_diff, fft_sizes=[c[0] for c in configs], hops=[c[1] for c in configs],
                                   win_lengths=[c[2] for c in configs])
        if args.aligned_mel:
            settings["aligned"]["mel"] = dict(n_mels=args.n_mels, mel_basis=args.mel_basis)
    if both_wav:
        settings["f0"] = dict(floor=args.f0_floor, ceil=args.f0_ceil, threshold=args.f0_threshold, min_voiced=args.f0_min_voiced, frame_length=args.f0_frame_length)
        if args.f0_method != "yin":  # the default's document stays as it was
            settings["f0"].update(method=args.f0_method, bins_per_semitone=args.f0_bins_per_semitone, max_rate=args.f0_max_rate)
    return summarise(records, settings)


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO if args.verbose else logging.WARN, format="%(asctime)s %(levelname)s: %(message)s")
    doc = evaluate(args)
    torch.cuda.synchronize()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    print(summary_line(doc))
    return doc


if __name__ == "__main__":
    main()
