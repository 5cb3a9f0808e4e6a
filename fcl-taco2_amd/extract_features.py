"""wav -> training features driver on MI355X: the acoustic half of the reference's preprocessing step (log10 mel, frame energy, phoneme-level
means, mean / std normalisation), written from the contract in include/fcl_hip.h "Feature extraction" and DESIGN.md §6e on fcl_taco2_amd/features.py.

    python -m fcl_taco2_amd.extract_features --wav-dir wavs --feature-root feats --durations-dir durations --track-f0 --train-list train.txt

Reads 16-bit PCM mono wavs at `--fs` (standard library `wave`; samples / 32768), batches them by frame count, and writes under `--feature-root`.  A wav
at another rate is refused unless `--resample` is given; it is then uploaded at its own rate and resampled on the device (fcl_taco2_amd/resample.py,
DESIGN.md §6g) in front of the mel launch and the tracker:
    mels-ori/<utt>.npy  [T, n_mels] float32 log10 mel, T = samples // hop + 1
    en-ori/<utt>.npy    [T] frame energy ||S||_2; with --durations-dir [P] phoneme-level means, and
    durations_MFA/<utt>.npy  [P] the durations with the last entry adjusted so that they sum to T
    f0-ori/<utt>.npy    [P] with --track-f0 (the YIN tracker of fcl_taco2_amd/pitch.py, DESIGN.md §6f, on the batch's samples already on the device;
                        --f0-floor / --f0-ceil / --f0-threshold / --f0-min-voiced / --f0-frame-length) or --f0-dir (frame-level F0 tracks in Hz
                        from any other tracker, 0 = unvoiced, truncated to T, zero-padded when shorter): phoneme-level means of log F0 over
                        voiced frames, 0 for a phoneme without one.  --f0-frames-out DIR also writes the tracker's frame-level tracks, <utt>.npy
                        [T] float32 Hz: fed back through --f0-dir they reproduce f0-ori/ bit for bit
With `--train-list` (utterance ids, one per line) the mean and population standard deviation over the listed utterances are accumulated in float64
(F0: non-zero entries only) and written as mel_stats.npy [2, n_mels] and f0_en_stats.npy [f0_mean, f0_std, en_mean, en_std] (en_stats.npy
[en_mean, en_std] without F0), and every utterance is normalised with them, (v - mean) / (std + 1e-8), into mels/ [T, n_mels], en/ [P, 1]
([T, 1] without --durations-dir) and f0/ [P, 1] (unvoiced phonemes stay 0): with durations_MFA/, the files a training manifest's input1 / input4 /
input3 / input2 point at.
TextGrid parsing, the symbol table, the split and the json manifests are fcl_taco2_amd/preprocess.py, which calls extract() and normalise_all() here.
Out of scope: parity with the reference's third-party F0 tracker (DIO + StoneMask) and resampler, tracking across frames.
"""
import argparse
import logging
import os
import time
import wave

import numpy as np
import torch

from . import features, griffinlim, pitch, resample
from .batching import Writer, make_batches


def _check_header(f, path, fs):
    if f.getsampwidth() != 2:
        raise ValueError("%s: %d-byte samples; only 16-bit PCM is read" % (path, f.getsampwidth()))
    if f.getnchannels() != 1:
        raise ValueError("%s: %d channels; only mono is read" % (path, f.getnchannels()))
    if fs is not None and f.getframerate() != fs:
        raise ValueError("%s: sampling rate %d, --fs is %d (there is no resampler)" % (path, f.getframerate(), fs))


def wav_samples(path, fs):
    """the sample count from the header alone (the same refusals as read_wav)"""
    with wave.open(path, "rb") as f:
        _check_header(f, path, fs)
        return f.getnframes()


def wav_rate_and_samples(path):
    """(sampling rate, sample count) from the header alone, for a driver that resamples (the other refusals of read_wav)"""
    with wave.open(path, "rb") as f:
        _check_header(f, path, None)
        return f.getframerate(), f.getnframes()


def read_wav(path, fs):
    """16-bit PCM mono at `fs` -> float32 samples / 32768; anything else is refused naming the file"""
    with wave.open(path, "rb") as f:
        _check_header(f, path, fs)
        pcm = np.frombuffer(f.readframes(f.getnframes()), dtype="<i2")
    return pcm.astype(np.float32) / np.float32(32768.0)


def read_wav_list(wav_scp=None, wav_dir=None):
    """[(utt_id, path)] sorted by id, from a Kaldi-style `utt path` list or every *.wav of a directory"""
    if wav_scp is not None:
        out = []
        with open(wav_scp) as f:
            for ln in f:
                if ln.strip():
                    uid, path = ln.strip().split(None, 1)
                    out.append((uid, path))
    else:
        out = [(n[:-4], os.path.join(wav_dir, n)) for n in os.listdir(wav_dir) if n.lower().endswith(".wav")]
    if not out:
        raise ValueError("no wav files in %s" % (wav_scp or wav_dir))
    ids = [u for u, _ in out]
    if len(set(ids)) != len(ids):
        raise ValueError("duplicate utterance ids in %s" % (wav_scp or wav_dir))
    return sorted(out)


class Moments(object):
    """mean and population standard deviation accumulated in float64 (per column for 2-D input)"""

    def __init__(self):
        self.n, self.s, self.ss = 0, 0.0, 0.0

    def add(self, a):
        a = np.asarray(a, dtype=np.float64)
        self.n += a.shape[0]
        self.s = self.s + a.sum(axis=0)
        self.ss = self.ss + (a * a).sum(axis=0)

    def result(self, what):
        if self.n == 0:
            raise ValueError("no %s entries in the --train-list utterances: no statistics" % what)
        mean = self.s / self.n
        return mean, np.sqrt(np.maximum(self.ss / self.n - mean * mean, 0.0))


def normalise(a, mean, std, nonzero_only=False):
    """(a - mean) / (std + 1e-8) in float64 -> float32; nonzero_only: zeros stay zero (unvoiced phonemes)"""
    a = np.asarray(a, dtype=np.float64)
    out = (a - mean) / (std + 1e-8)
    return (np.where(a != 0.0, out, 0.0) if nonzero_only else out).astype(np.float32)


def log_f0(f0):
    """frame-level F0 in Hz -> log F0 where voiced, 0 elsewhere"""
    f0 = np.asarray(f0, dtype=np.float64).reshape(-1)
    return np.where(f0 > 0.0, np.log(np.maximum(f0, 1e-300)), 0.0).astype(np.float32)


def fit_track(f0, T):
    """an external tracker's frame count rarely equals T exactly: truncated to T, zero-padded (unvoiced) when shorter"""
    f0 = np.asarray(f0, dtype=np.float32).reshape(-1)[:T]
    return np.concatenate([f0, np.zeros(T - len(f0), np.float32)])


def _by_rate(idx, rates):
    """a batch's indices split into runs of one sampling rate, in first-seen order (files of different rates cannot share a packed launch)"""
    if rates is None:
        return [(idx, None)]
    groups = {}
    for i in idx:
        groups.setdefault(rates[i], []).append(i)
    return [(g, r) for r, g in groups.items()]


def extract(fx, utts, root, batch_frames=51200, durations_dir=None, f0_dir=None, tracker=None, f0_frames_out=None, resampler_for=None):
    """utts: [(utt_id, path)].  Writes the -ori files under root; returns the ids in input order.  tracker (a pitch.PitchTracker on fx's hop and
    sampling rate) takes the place of f0_dir's tracks; f0_frames_out: a directory for its frame-level tracks.  resampler_for (input rate -> a
    resample.Resampler to fx's rate, e.g. a resample.ResamplerCache): wavs at another rate are resampled on the device instead of refused."""
    pl = fx.plan
    sub = lambda d: os.path.join(root, d)
    for d in ["mels-ori", "en-ori"] + (["durations_MFA"] if durations_dir else []) + (["f0-ori"] if f0_dir or tracker else []):
        os.makedirs(sub(d), exist_ok=True)
    if f0_frames_out:
        os.makedirs(f0_frames_out, exist_ok=True)
    ids, paths = [u for u, _ in utts], dict(utts)
    rates = None
    if resampler_for is None:
        n_samples = [wav_samples(paths[u], pl.fs) for u in ids]  # headers only: the samples are read batch by batch
    else:  # the sample counts after resampling, in integers from the header's
        rates, n_samples = [], []
        for u in ids:
            rate, n = wav_rate_and_samples(paths[u])
            try:
                L, M, _ = resample.check_rates(rate, pl.fs)
            except (NotImplementedError, ValueError) as e:
                raise type(e)("%s: %s" % (paths[u], e))
            rates.append(rate)
            n_samples.append(resample.out_samples(n, L, M))
    fx.check_lens(n_samples, ids)  # refused by id before the first device call
    if tracker is not None:
        tracker.check_lens(n_samples, ids)
    frame_lens = [fx.frames_of(n) for n in n_samples]

    def write(items):
        for path, arr in items:
            np.save(path, arr)

    wr = Writer(write, 4)
    try:
        for idx, rate in (g for b in make_batches(frame_lens, batch_frames) for g in _by_rate(b, rates)):
            bid = [ids[i] for i in idx]
            waves = [read_wav(paths[u], pl.fs if rate is None else rate) for u in bid]
            lens = [len(w) for w in waves]
            if rate is not None and rate != pl.fs:  # uploaded at its own rate, resampled on the device
                x, lens = resampler_for(rate).resample_packed(torch.from_numpy(np.concatenate(waves)).to(pl.device), lens, ids=bid)
            elif tracker is None:
                x = np.concatenate(waves)
            else:
                x = torch.from_numpy(np.concatenate(waves)).to(pl.device)
            if tracker is None:
                mel, energy, T = fx.extract_packed(x, lens, ids=bid)
            else:  # one upload and one set of maps for the mel launch and the tracker's two
                mp = features.Maps(lens, pl.hop, pl.device)
                mel, energy, T = fx.extract_packed(x, lens, ids=bid, maps=mp)
                f0 = tracker.track_packed(x, lens, ids=bid, maps=mp)[0].cpu().numpy()
            if durations_dir:
                durs = [np.load(os.path.join(durations_dir, u + ".npy")) for u in bid]
                en, durs = fx.phoneme_means(energy, T, durs, ids=bid)
                en = en.cpu().numpy()
                ph = np.concatenate([[0], np.cumsum([len(d) for d in durs])])
                if f0_dir or tracker is not None:
                    if tracker is None:
                        f0 = np.concatenate([fit_track(np.load(os.path.join(f0_dir, u + ".npy")), t) for u, t in zip(bid, T)])
                    lf0, _ = fx.phoneme_means(log_f0(f0), T, durs, mask=f0, ids=bid)
                    lf0 = lf0.cpu().numpy()
            mel, energy = mel.cpu().numpy(), energy.cpu().numpy()
            fo = np.concatenate([[0], np.cumsum(T)])
            items = []
            for j, u in enumerate(bid):
                items.append((os.path.join(sub("mels-ori"), u + ".npy"), mel[fo[j] : fo[j + 1]].copy()))
                if durations_dir:
                    items.append((os.path.join(sub("en-ori"), u + ".npy"), en[ph[j] : ph[j + 1]].copy()))
                    items.append((os.path.join(sub("durations_MFA"), u + ".npy"), durs[j]))
                    if f0_dir or tracker is not None:
                        items.append((os.path.join(sub("f0-ori"), u + ".npy"), lf0[ph[j] : ph[j + 1]].copy()))
                else:
                    items.append((os.path.join(sub("en-ori"), u + ".npy"), energy[fo[j] : fo[j + 1]].copy()))
                if f0_frames_out:
                    items.append((os.path.join(f0_frames_out, u + ".npy"), f0[fo[j] : fo[j + 1]].copy()))
            wr.put(items)
    finally:
        wr.join()
    wr.close()
    return ids


def normalise_all(root, ids, train_ids, have_durations, have_f0):
    """statistics over train_ids from the -ori files, then the normalised files of every utterance; returns the statistics"""
    sub = lambda d, u: os.path.join(root, d, u + ".npy")
    have = set(ids)
    missing = [u for u in train_ids if u not in have]
    if missing:
        raise ValueError("--train-list names %d utterances without a wav (first: %s)" % (len(missing), missing[0]))
    m_mel, m_en, m_f0 = Moments(), Moments(), Moments()
    for u in train_ids:
        m_mel.add(np.load(sub("mels-ori", u)))
        m_en.add(np.load(sub("en-ori", u)).reshape(-1))
        if have_f0:
            f0 = np.load(sub("f0-ori", u)).reshape(-1)
            m_f0.add(f0[f0 != 0.0])
    mel_mean, mel_std = m_mel.result("mel")
    en_mean, en_std = m_en.result("energy")
    np.save(os.path.join(root, "mel_stats.npy"), np.stack([mel_mean, mel_std]))
    stats = dict(mel=(mel_mean, mel_std), en=(en_mean, en_std))
    if have_f0:
        stats["f0"] = m_f0.result("voiced F0")
        np.save(os.path.join(root, "f0_en_stats.npy"), np.array([stats["f0"][0], stats["f0"][1], en_mean, en_std]))
    else:
        np.save(os.path.join(root, "en_stats.npy"), np.array([en_mean, en_std]))
    for d in ["mels", "en"] + (["f0"] if have_f0 else []):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    for u in ids:
        np.save(sub("mels", u), normalise(np.load(sub("mels-ori", u)), mel_mean, mel_std))
        np.save(sub("en", u), normalise(np.load(sub("en-ori", u)).reshape(-1, 1), en_mean, en_std))
        if have_f0:
            np.save(sub("f0", u), normalise(np.load(sub("f0-ori", u)).reshape(-1, 1), stats["f0"][0], stats["f0"][1], nonzero_only=True))
    return stats


def build_parser():
    ap = argparse.ArgumentParser(prog="fcl_taco2_amd.extract_features", description="wav -> log-mel / energy / phoneme-level training features on MI355X")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--wav-scp", default=None, metavar="FILE", help="`utt_id path` per line")
    src.add_argument("--wav-dir", default=None, metavar="DIR", help="every *.wav of the directory (utt_id = the file name without .wav)")
    ap.add_argument("--feature-root", required=True, metavar="DIR")
    ap.add_argument("--durations-dir", default=None, metavar="DIR", help="<utt>.npy integer phoneme durations in frames: energy (and F0) become phoneme-level")
    ap.add_argument("--f0-dir", default=None, metavar="DIR", help="<utt>.npy frame-level F0 in Hz (0 = unvoiced) from an external tracker; needs --durations-dir")
    ap.add_argument("--track-f0", action="store_true", help="track F0 on the GPU (YIN) in place of --f0-dir; needs --durations-dir")
    ap.add_argument("--f0-frames-out", default=None, metavar="DIR", help="with --track-f0: also write the frame-level tracks <utt>.npy [T] float32 Hz")
    ap.add_argument("--train-list", default=None, metavar="FILE", help="utterance ids (one per line) the statistics are taken over; writes the normalised files")
    ap.add_argument("--resample", action="store_true", help="resample wavs whose rate is not --fs on the GPU instead of refusing them")
    ap.add_argument("--batch-frames", type=int, default=51200, help="frames per GPU batch")
    ap.add_argument("--n-mels", type=int, default=griffinlim.DEFAULTS["n_mels"])
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--verbose", type=int, default=1)
    g = ap.add_argument_group("analysis (the defaults are the reference's preprocessing)")
    g.add_argument("--mel-basis", default=None, metavar="FILE.npy", help="[n_mels, n_fft / 2 + 1] mel filterbank replacing the built Slaney one")
    griffinlim.add_analysis_arguments(g)
    pitch.add_pitch_arguments(ap.add_argument_group("F0 tracking (--track-f0; the defaults are the range of the reference's tracker)"))
    return ap


def parse_args(argv=None):
    """Parses and checks what can be checked before the first device call; flag errors end in ap.error (SystemExit 2)."""
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.f0_dir and not args.durations_dir:
        ap.error("--f0-dir needs --durations-dir (F0 is written as phoneme-level means)")
    if args.track_f0 and args.f0_dir:
        ap.error("--track-f0 and --f0-dir are mutually exclusive (one source of F0)")
    if args.track_f0 and not args.durations_dir:
        ap.error("--track-f0 needs --durations-dir (F0 is written as phoneme-level means)")
    if args.f0_frames_out and not args.track_f0:
        ap.error("--f0-frames-out needs --track-f0 (it writes the tracker's frame-level tracks)")
    if args.batch_frames < 1:
        ap.error("--batch-frames must be positive")
    for flag, d in (("--wav-dir", args.wav_dir), ("--durations-dir", args.durations_dir), ("--f0-dir", args.f0_dir)):
        if d is not None and not os.path.isdir(d):
            ap.error("%s %s is not a directory" % (flag, d))
    for flag, p in (("--wav-scp", args.wav_scp), ("--train-list", args.train_list), ("--mel-basis", args.mel_basis)):
        if p is not None and not os.path.isfile(p):
            ap.error("%s %s is not a file" % (flag, p))
    try:
        griffinlim.check_config(args.n_fft, args.hop, args.n_fft if args.win_length is None else args.win_length, args.n_mels, args.fs, args.fmin, args.fmax)
    except (NotImplementedError, ValueError) as e:
        ap.error(str(e))
    if args.track_f0:
        pitch.check_arguments(ap, args)
    return args


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO if args.verbose else logging.WARN, format="%(asctime)s %(levelname)s: %(message)s")
    utts = read_wav_list(args.wav_scp, args.wav_dir)
    train_ids = None
    if args.train_list:
        with open(args.train_list) as f:
            train_ids = [ln.strip() for ln in f if ln.strip()]
    t0 = time.perf_counter()
    fx = features.from_args(args, args.device)
    tracker = pitch.from_args(args, args.device) if args.track_f0 else None
    resampler_for = resample.ResamplerCache(args.device, args.fs) if args.resample else None
    ids = extract(fx, utts, args.feature_root, args.batch_frames, args.durations_dir, args.f0_dir, tracker, args.f0_frames_out, resampler_for)
    torch.cuda.synchronize()
    have_f0 = bool(args.f0_dir) or args.track_f0
    stats = normalise_all(args.feature_root, ids, train_ids, bool(args.durations_dir), have_f0) if train_ids is not None else None
    logging.info("extracted %d utterances in %.2f s", len(ids), time.perf_counter() - t0)
    return ids, stats


if __name__ == "__main__":
    main()
