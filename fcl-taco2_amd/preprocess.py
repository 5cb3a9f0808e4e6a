"""Corpus + TextGrids -> everything `train` and `decode` read: the reference's preprocessing step (preprocess.py) as one command on MI355X.

    python -m fcl_taco2_amd.preprocess --data-root LJSpeech-1.1 --textgrid-root TextGrid --feature-root data

1. reads `<textgrid-root>/<utt>.TextGrid` of every wav (fcl_taco2_amd/textgrid.py): the `phones` tier -> phoneme sequence and durations in frames by the
   reference's integer rules;
2. writes `phn2idx.json` (the sorted labels numbered from 1, "PAD": 0; `--phn2idx FILE` reuses an existing table) and `durations_MFA-ori/<utt>.npy` [P, 1];
3. extracts log-mel, energy and F0 (the YIN tracker, or `--f0-dir` tracks) once, with fcl_taco2_amd/extract_features.py's extract() and
   normalise_all(): mels-ori/ en-ori/ f0-ori/ durations_MFA/ mels/ en/ f0/ mel_stats.npy f0_en_stats.npy.  A wav whose rate is not `--fs` is resampled
   on the device (fcl_taco2_amd/resample.py; `--no-resample` refuses it instead);
4. splits the corpus (`--n-valid`, `--n-test`, `--split-seed`, or the three lists) and writes train_data.json, val_data.json and test_data.json
   (fcl_taco2_amd/manifest.py); the statistics of step 3 are taken over the training utterances.
A wav without a TextGrid, or a TextGrid without a wav, is refused by id before the first device call."""
import argparse
import logging
import os
import time

import numpy as np
import torch

from . import extract_features as X
from . import features, griffinlim, manifest, pitch, resample, textgrid


def build_parser():
    ap = argparse.ArgumentParser(prog="fcl_taco2_amd.preprocess", description="wavs + TextGrids -> training features, phn2idx.json and the json manifests on MI355X")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--data-root", default=None, metavar="DIR", help="the corpus: every DIR/wavs/*.wav (utt_id = the file name without .wav)")
    src.add_argument("--wav-scp", default=None, metavar="FILE", help="`utt_id path` per line")
    ap.add_argument("--textgrid-root", required=True, metavar="DIR", help="<utt_id>.TextGrid of the forced aligner, with a `phones` interval tier")
    ap.add_argument("--feature-root", required=True, metavar="DIR")
    ap.add_argument("--f0-dir", default=None, metavar="DIR", help="<utt>.npy frame-level F0 in Hz (0 = unvoiced) from an external tracker, in place of the GPU tracker")
    ap.add_argument("--phn2idx", default=None, metavar="FILE", help="an existing phn2idx.json to number the phones with (a phone it lacks is refused)")
    ap.add_argument("--empty-label", default=None, metavar="LABEL", help="the label of an interval with empty text (default: kept empty)")
    ap.add_argument("--max-phn-dur", type=int, default=manifest.MAX_PHN_DUR, help="utterances with a longer phoneme (in frames) are left out of the manifests")
    ap.add_argument("--n-valid", type=int, default=500)
    ap.add_argument("--n-test", type=int, default=500)
    ap.add_argument("--split-seed", type=int, default=0)
    for k in ("train", "valid", "test"):
        ap.add_argument("--%s-list" % k, default=None, metavar="FILE", help="utterance ids, one per line: the three lists replace the seeded split")
    ap.add_argument("--speaker", default="LJ", help="utt2spk of every utterance")
    ap.add_argument("--no-resample", action="store_true", help="refuse a wav whose rate is not --fs instead of resampling it")
    ap.add_argument("--batch-frames", type=int, default=51200, help="frames per GPU batch")
    ap.add_argument("--n-mels", type=int, default=griffinlim.DEFAULTS["n_mels"])
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--verbose", type=int, default=1)
    g = ap.add_argument_group("analysis (the defaults are the reference's preprocessing)")
    g.add_argument("--mel-basis", default=None, metavar="FILE.npy", help="[n_mels, n_fft / 2 + 1] mel filterbank replacing the built Slaney one")
    griffinlim.add_analysis_arguments(g)
    pitch.add_pitch_arguments(ap.add_argument_group("F0 tracking (without --f0-dir; the defaults are the range of the reference's tracker)"))
    return ap


def parse_args(argv=None):
    """Parses and checks what can be checked before the first device call; flag errors end in ap.error (SystemExit 2)."""
    ap = build_parser()
    args = ap.parse_args(argv)
    lists = [args.train_list, args.valid_list, args.test_list]
    if any(lists) and not all(lists):
        ap.error("--train-list, --valid-list and --test-list come together")
    if args.batch_frames < 1 or args.max_phn_dur < 1:
        ap.error("--batch-frames and --max-phn-dur must be positive")
    for flag, d in (("--data-root", args.data_root and os.path.join(args.data_root, "wavs")), ("--textgrid-root", args.textgrid_root), ("--f0-dir", args.f0_dir)):
        if d is not None and not os.path.isdir(d):
            ap.error("%s: %s is not a directory" % (flag, d))
    for flag, p in [("--wav-scp", args.wav_scp), ("--phn2idx", args.phn2idx), ("--mel-basis", args.mel_basis)] + list(zip(("--train-list", "--valid-list", "--test-list"), lists)):
        if p is not None and not os.path.isfile(p):
            ap.error("%s %s is not a file" % (flag, p))
    try:
        griffinlim.check_config(args.n_fft, args.hop, args.n_fft if args.win_length is None else args.win_length, args.n_mels, args.fs, args.fmin, args.fmax)
    except (NotImplementedError, ValueError) as e:
        ap.error(str(e))
    if not args.f0_dir:
        pitch.check_arguments(ap, args)
    return args


def read_alignments(ids, textgrid_root, fs, hop, empty_label=None):
    """-> ({utt: (phones, durations)}, every label: the raw ones of the `phones` tiers and what the alignment rules made of them)"""
    have = set(n[: -len(".TextGrid")] for n in os.listdir(textgrid_root) if n.endswith(".TextGrid"))
    missing, extra = [u for u in ids if u not in have], sorted(have - set(ids))
    if missing:
        raise ValueError("%d utterances have a wav but no TextGrid in %s (first: %s)" % (len(missing), textgrid_root, missing[0]))
    if extra:
        raise ValueError("%d TextGrids in %s have no wav (first: %s)" % (len(extra), textgrid_root, extra[0]))
    aligned, labels = {}, set()
    for u in ids:
        path = os.path.join(textgrid_root, u + ".TextGrid")
        tier = textgrid.read_textgrid(path)["phones"]
        try:
            aligned[u] = textgrid.alignment(tier, fs, hop, empty_label)
        except ValueError as e:
            raise ValueError("%s: %s" % (path, e))
        labels.update(p for _, _, p in tier)
        labels.update(aligned[u][0])
    return aligned, labels


def read_list(path):
    with open(path) as f:
        return [ln.strip() for ln in f if ln.strip()]


def split(args, ids):
    """(train, valid, test) ids from the three lists or the seeded permutation"""
    if not args.train_list:
        return manifest.split_ids(ids, args.n_valid, args.n_test, args.split_seed)
    parts = [read_list(p) for p in (args.train_list, args.valid_list, args.test_list)]
    seen, have = set(), set(ids)
    for flag, part in zip(("--train-list", "--valid-list", "--test-list"), parts):
        for u in part:
            if u not in have:
                raise ValueError("%s names %s, which has no wav" % (flag, u))
            if u in seen:
                raise ValueError("%s names %s, which is listed twice" % (flag, u))
            seen.add(u)
    if not parts[0]:
        raise ValueError("--train-list is empty: no statistics")
    return tuple(parts)


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO if args.verbose else logging.WARN, format="%(asctime)s %(levelname)s: %(message)s")
    root = args.feature_root
    utts = X.read_wav_list(args.wav_scp, os.path.join(args.data_root, "wavs") if args.data_root else None)
    ids = [u for u, _ in utts]
    t0 = time.perf_counter()
    aligned, labels = read_alignments(ids, args.textgrid_root, args.fs, args.hop, args.empty_label)
    table = textgrid.load_symbol_table(args.phn2idx) if args.phn2idx else textgrid.symbol_table(labels)
    tokens = {u: textgrid.token_ids(aligned[u][0], table, u) for u in ids}
    train_ids, valid_ids, test_ids = split(args, ids)
    os.makedirs(os.path.join(root, "durations_MFA-ori"), exist_ok=True)
    textgrid.write_symbol_table(os.path.join(root, "phn2idx.json"), table)
    for u in ids:
        np.save(os.path.join(root, "durations_MFA-ori", u + ".npy"), np.array(aligned[u][1], dtype=np.int64).reshape(-1, 1))

    fx = features.from_args(args, args.device)
    tracker = None if args.f0_dir else pitch.from_args(args, args.device)
    resampler_for = None if args.no_resample else resample.ResamplerCache(args.device, args.fs)
    X.extract(fx, utts, root, args.batch_frames, os.path.join(root, "durations_MFA-ori"), args.f0_dir, tracker, None, resampler_for)
    torch.cuda.synchronize()
    stats = X.normalise_all(root, ids, train_ids, True, True)

    entries = {}
    for u in ids:
        durs = np.load(os.path.join(root, "durations_MFA", u + ".npy")).reshape(-1)
        sub = lambda d: os.path.join(root, d, u + ".npy")
        entries[u] = manifest.entry(u, aligned[u][0], tokens[u], durs, int(durs.sum()), fx.plan.A, sub("mels"), sub("durations_MFA"), sub("f0"), sub("en"))
    written = {}
    for mode, part in (("train", train_ids), ("val", valid_ids), ("test", test_ids)):
        written[mode] = manifest.write_manifest(os.path.join(root, mode + "_data.json"), [entries[u] for u in part], len(table), args.speaker, args.max_phn_dur)
    logging.info("preprocessed %d utterances in %.2f s: %d train / %d val / %d test in the manifests, %d symbols", len(ids), time.perf_counter() - t0,
                 len(written["train"]), len(written["val"]), len(written["test"]), len(table))
    return dict(ids=ids, train=train_ids, valid=valid_ids, test=test_ids, written=written, stats=stats, phn2idx=table)


if __name__ == "__main__":
    main()
