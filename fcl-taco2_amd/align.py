"""Forced-alignment driver on MI355X: wavs and phoneme transcripts -> TextGrids that `preprocess` reads, on fcl_taco2_amd/alignment.py.

    python -m fcl_taco2_amd.align --wav-dir wavs --transcripts phones.txt --textgrid-out TextGrid --optional sp --model-out align.npz
    python -m fcl_taco2_amd.align --wav-dir more_wavs --transcripts more.txt --textgrid-out TextGrid2 --optional sp --model align.npz
    python -m fcl_taco2_amd.align --wav-dir wavs --transcripts words.txt --lexicon lexicon.txt --optional sp --textgrid-out TextGrid

`--transcripts` holds one utterance per line, `utt ph ph ...`: the phonemes -- or, with `--lexicon`, `utt word word ...` (below).  Every utterance of
the transcripts needs `<utt>.wav` (16-bit PCM mono) in `--wav-dir`.  Without `--model` the inventory is the set of labels and the models are
trained on these very utterances from a flat start (`--iterations`, default 15: not tuned, the synthetic corpora of the tests converge within 6);
with `--model` the driver only aligns.  `--mixtures N` (1 .. 8, default 1: single Gaussians) then grows every state into a mixture: the component target
per state doubles (2, 4, ..., at last N), the components are split at each target and `--mix-iterations` rounds (default 4) of alignment and
re-estimation follow; a component is split only while it holds at least twice `--min-occupancy` frames (default 10).  `--model-out` keeps the
mixtures, `--model` aligns with them (and ignores the training flags, as it ignores `--iterations`).  `--optional` names the labels that may be skipped as a whole (pauses between words); such a label must stand
between two mandatory ones.  A label outside the inventory, an utterance longer than 4096 frames or 1024 rows (phonemes x states) and a misplaced
optional label are refused by name before the first device call.

Per utterance `<utt>.TextGrid` (long text format, one tier `phones`) goes to `--textgrid-out`: a boundary at frame k is written as
(k hop + 0.5) / fs, the last interval ends at the wav's end, so that textgrid.alignment() gives back the aligner's durations with the last one less
by 1, which preprocess's last-duration rule restores.  `--durations-out` also keeps the durations as `<utt>.npy` (int64, summing to the frame
count).  `--report` holds the mean score per frame of every iteration and the utterances that could not be aligned (they get no TextGrid); with mixtures
its `settings` also name `mixtures` and every iteration its `components`, the component total of that round.

`--lexicon FILE` (lines `WORD PH PH ...`, one pronunciation per line, `WORD(2)` for further ones; lexicon.py) makes the transcripts word text: every
word stands in the utterance's graph with all its pronunciations side by side (at most 7), the one label `--optional` names is inserted as a silence
between the words and at both ends (`--no-boundary-silence`: between the words only), and the alignment picks pronunciations and pauses (DESIGN.md
§6x).  Words are compared lower-cased and without surrounding punctuation; there is no G2P: with `--oov refuse` (the default) the words the lexicon
lacks are listed with their counts and nothing runs, with `--oov skip` the utterances that hold one are left out and named in the report.  Without
`--model` the inventory is the silence label and every label in the pronunciations of the words that occur.  The TextGrids keep the tier `phones`
as it is and gain a tier `words`: a word spans its phones, a silence is an interval with empty text.  `--pronunciations-out FILE` writes
`utt ph ph ...` of the chosen paths, the format `--transcripts` takes without a lexicon; the report gains, per word, how often each of its
pronunciations was chosen."""
import argparse
import collections
import json
import logging
import os

import numpy as np
import torch

from . import alignment, extract_features as X, features, griffinlim, lexicon, resample, textgrid


def read_transcripts(path):
    """`utt ph ph ...` lines -> {utt: [labels]} in file order; a duplicate id or a line without labels is refused"""
    out = {}
    with open(path, encoding="utf-8") as f:
        for no, ln in enumerate(f, 1):
            parts = ln.split()
            if not parts:
                continue
            if len(parts) < 2:
                raise ValueError("%s:%d: utterance %s has no labels" % (path, no, parts[0]))
            if parts[0] in out:
                raise ValueError("%s:%d: utterance %s appears twice" % (path, no, parts[0]))
            out[parts[0]] = parts[1:]
    if not out:
        raise ValueError("no transcripts in %s" % path)
    return out


def build_parser():
    ap = argparse.ArgumentParser(prog="fcl_taco2_amd.align", description="flat-start forced alignment of phoneme transcripts on MI355X")
    ap.add_argument("--wav-dir", required=True, metavar="DIR", help="<utt>.wav, 16-bit PCM mono")
    ap.add_argument("--transcripts", required=True, metavar="FILE", help="lines `utt ph ph ...`")
    ap.add_argument("--textgrid-out", required=True, metavar="DIR", help="<utt>.TextGrid with the tier `phones`")
    ap.add_argument("--durations-out", default=None, metavar="DIR", help="<utt>.npy: durations in frames")
    ap.add_argument("--optional", nargs="*", default=[], metavar="LABEL", help="labels that may be skipped (pauses); with --lexicon the one silence label")
    ap.add_argument("--lexicon", default=None, metavar="FILE", help="lines `WORD PH PH ...`: --transcripts then holds words, aligned through all their pronunciations")
    ap.add_argument("--oov", choices=("refuse", "skip"), default="refuse", help="words the lexicon lacks: stop and list them, or leave their utterances out")
    ap.add_argument("--no-boundary-silence", action="store_true", help="with --lexicon: no optional silence at the two ends of an utterance")
    ap.add_argument("--pronunciations-out", default=None, metavar="FILE", help="with --lexicon: `utt ph ph ...` of the chosen paths")
    ap.add_argument("--states", type=int, default=alignment.STATES_DEFAULT, help="states per phoneme, 1 .. %d" % alignment.STATES_MAX)
    ap.add_argument("--iterations", type=int, default=alignment.ITERATIONS_DEFAULT, help="alignment / re-estimation rounds after the flat start (not tuned)")
    ap.add_argument("--mixtures", type=int, default=1, help="Gaussians per state after the mixture stage, 1 .. %d (1: single Gaussians)" % alignment.MIXTURES_MAX)
    ap.add_argument("--mix-iterations", type=int, default=alignment.MIX_ITERATIONS_DEFAULT, help="alignment / re-estimation rounds at each component target")
    ap.add_argument("--min-occupancy", type=float, default=alignment.MIN_OCCUPANCY_DEFAULT, help="a component is split only while it holds twice this many frames")
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--model-out", default=None, metavar="FILE.npz", help="keep the trained models")
    g.add_argument("--model", default=None, metavar="FILE.npz", help="align with these models, without training")
    ap.add_argument("--resample", action="store_true", help="resample wavs whose rate is not --fs on the GPU instead of refusing them")
    ap.add_argument("--report", default=None, metavar="FILE.json", help="per-iteration mean score per frame, the utterances without an alignment")
    ap.add_argument("--batch-cells", type=int, default=alignment.BATCH_CELLS, help="cells S x T per GPU batch")
    ap.add_argument("--batch-frames", type=int, default=51200, help="frames per feature-extraction batch")
    ap.add_argument("--n-mels", type=int, default=griffinlim.DEFAULTS["n_mels"])
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--verbose", type=int, default=1)
    g = ap.add_argument_group("analysis (the defaults are the reference's preprocessing)")
    g.add_argument("--mel-basis", default=None, metavar="FILE.npy", help="[n_mels, n_fft / 2 + 1] mel filterbank replacing the built Slaney one")
    griffinlim.add_analysis_arguments(g)
    return ap


def parse_args(argv=None):
    """Parses and checks what can be checked before the first device call; flag errors end in ap.error (SystemExit 2)."""
    ap = build_parser()
    args = ap.parse_args(argv)
    if not os.path.isdir(args.wav_dir):
        ap.error("--wav-dir %s is not a directory" % args.wav_dir)
    for flag, p in (("--transcripts", args.transcripts), ("--model", args.model), ("--mel-basis", args.mel_basis), ("--lexicon", args.lexicon)):
        if p is not None and not os.path.isfile(p):
            ap.error("%s %s is not a file" % (flag, p))
    if not 1 <= args.states <= alignment.STATES_MAX:
        ap.error("--states must lie in 1 .. %d" % alignment.STATES_MAX)
    if args.iterations < 0 or args.batch_cells < 1 or args.batch_frames < 1:
        ap.error("--iterations must not be negative, --batch-cells and --batch-frames must be positive")
    if not 1 <= args.mixtures <= alignment.MIXTURES_MAX:
        ap.error("--mixtures must lie in 1 .. %d" % alignment.MIXTURES_MAX)
    if args.mix_iterations < 0:
        ap.error("--mix-iterations must not be negative")
    if not args.min_occupancy >= 1.0:
        ap.error("--min-occupancy must be at least 1")
    if args.lexicon is not None and len(args.optional) != 1:
        ap.error("--lexicon needs --optional to name exactly one label, the silence")
    if args.lexicon is None and (args.pronunciations_out or args.no_boundary_silence or args.oov != "refuse"):
        ap.error("--pronunciations-out, --no-boundary-silence and --oov go with --lexicon")
    if args.n_mels - 1 < alignment.ORDER:
        ap.error("--n-mels must exceed the %d cepstra the features take" % alignment.ORDER)
    try:
        griffinlim.check_config(args.n_fft, args.hop, args.n_fft if args.win_length is None else args.win_length, args.n_mels, args.fs, args.fmin, args.fmax)
    except (NotImplementedError, ValueError) as e:
        ap.error(str(e))
    return args


def plan_utterances(args, transcripts):
    """[(utt, path, rate, samples at the analysis rate)] from the headers alone; a missing wav, another rate without --resample and more than 4096
    frames are refused by name"""
    out = []
    for u in transcripts:
        path = os.path.join(args.wav_dir, u + ".wav")
        if not os.path.isfile(path):
            raise ValueError("utterance %s of %s has no wav: %s is missing" % (u, args.transcripts, path))
        rate, n = X.wav_rate_and_samples(path)
        if rate != args.fs:
            if not args.resample:
                raise ValueError("%s: sampling rate %d, --fs is %d (--resample resamples on the device)" % (path, rate, args.fs))
            L, M, _ = resample.check_rates(rate, args.fs)
            n = resample.out_samples(n, L, M)
        T = features.frames_of(n, args.hop)
        if T > alignment.FRAMES_MAX:
            raise ValueError("utterance %s has %d frames; the alignment covers 1 .. %d" % (u, T, alignment.FRAMES_MAX))
        out.append((u, path, rate, n))
    return out


def extract(args, utts, af):
    """the aligner's features of every utterance, on the device, in feature batches of --batch-frames"""
    dev, fs = af.extractor.plan.device, args.fs
    cache = resample.ResamplerCache(args.device, fs) if args.resample else None
    feats, batch, frames = [], [], 0

    def flush():
        if not batch:
            return
        xs = [torch.from_numpy(X.read_wav(path, rate)).to(dev) for _, path, rate, _ in batch]
        lens = [int(x.numel()) for x in xs]
        groups = {}
        for i, (_, _, rate, _) in enumerate(batch):
            if rate != fs:
                groups.setdefault(rate, []).append(i)
        for rate, g in groups.items():
            y, out_lens = cache(rate).resample_packed(torch.cat([xs[i] for i in g]), [lens[i] for i in g])
            o = np.concatenate([[0], np.cumsum(out_lens)])
            for k, i in enumerate(g):
                xs[i], lens[i] = y[int(o[k]) : int(o[k + 1])], int(out_lens[k])
        if lens != [n for _, _, _, n in batch]:
            raise RuntimeError("align: the sample counts read do not match the headers' (%s .. %s)" % (batch[0][0], batch[-1][0]))
        ids = [u for u, _, _, _ in batch]
        mel, energy, frame_lens = af.extractor.extract_packed(torch.cat(xs), lens, ids=ids)
        feats.extend(af.from_mel(mel, energy, frame_lens))
        del batch[:]

    for item in utts:
        T = features.frames_of(item[3], args.hop)
        if batch and frames + T > args.batch_frames:
            flush()
            frames = 0
        batch.append(item)
        frames += T
    flush()
    return feats


def check_words(args, transcripts, lex):
    """the words the lexicon lacks: refused with their counts (--oov refuse), or their utterances taken out of `transcripts` (--oov skip)
    -> {utt: [its words the lexicon lacks]} of the utterances left out"""
    missing = {u: sorted(set(w for w in lexicon.normalise_words(tr) if w not in lex)) for u, tr in transcripts.items()}
    missing = {u: m for u, m in missing.items() if m}
    if not missing:
        return {}
    if args.oov == "refuse":
        counts = collections.Counter(w for u in missing for w in lexicon.normalise_words(transcripts[u]) if w not in lex)
        raise ValueError("%d words of %s are not in %s (in %d utterances; --oov skip leaves those out): %s"
                         % (len(counts), args.transcripts, args.lexicon, len(missing), ", ".join("%s (%d)" % (w, counts[w]) for w in sorted(counts))))
    for u in missing:
        del transcripts[u]
    if not transcripts:
        raise ValueError("every utterance of %s holds a word that is not in %s" % (args.transcripts, args.lexicon))
    return missing


def word_tier(r, fs, hop, n_samples):
    """the `words` tier of a result of Aligner.align(lexicon=): a word spans its phones, a silence is an interval with empty text"""
    texts, durs, last = [], [], None
    for w, d in zip(r["label_words"], r["durations"]):
        if w >= 0 and w == last:
            durs[-1] += d
        else:
            texts.append(r["words"][w] if w >= 0 else "")
            durs.append(d)
        last = w
    return textgrid.frame_intervals(texts, durs, fs, hop, n_samples)


def align(args):
    """-> the --report document"""
    transcripts = read_transcripts(args.transcripts)
    lex = lexicon.read_lexicon(args.lexicon) if args.lexicon else None
    skipped = check_words(args, transcripts, lex) if lex is not None else {}
    ids = list(transcripts)
    model = alignment.AlignModel.load(args.model) if args.model else None
    if lex is not None:
        phones = model.phones if model else sorted(set(args.optional) | set(lex.labels(w for tr in transcripts.values() for w in tr)))
    else:
        phones = model.phones if model else sorted(set(p for tr in transcripts.values() for p in tr))
    states = model.K if model else args.states
    for p in args.optional:
        if p not in phones:
            logging.warning("--optional %s: no such label in the %s", p, "model" if model else "transcripts")
    al = alignment.Aligner(args.device, phones, states, optional=[p for p in args.optional if p in phones], model=model, batch_cells=args.batch_cells)
    word_kw = dict(lexicon=lex, boundary=not args.no_boundary_silence) if lex is not None else {}
    for u in ids:  # every refusal of a transcript, before the first device call
        if lex is not None:
            alignment.build_word_graph(transcripts[u], lex, al.index, al.silence(), al.K, word_kw["boundary"], u)
        else:
            alignment.build_graph(transcripts[u], al.index, al.optional, al.K, u)
    utts = plan_utterances(args, transcripts)
    af = alignment.AlignFeatures(features.from_args(args, args.device))
    if model is not None and model.settings != af.settings:
        diff = sorted(k for k in set(model.settings) | set(af.settings) if model.settings.get(k) != af.settings.get(k))
        raise ValueError("%s was trained on other features: %s differ" % (args.model, ", ".join(diff)))
    al.settings = af.settings
    feats = extract(args, utts, af)
    trs = [transcripts[u] for u in ids]
    history = dict(score=[], failed=[], components=[])
    if model is None:
        history = al.fit(feats, trs, args.iterations, ids=ids, mixtures=args.mixtures, mix_iterations=args.mix_iterations, min_occupancy=args.min_occupancy,
                         **word_kw)
        for it, s in enumerate(history["score"]):
            if args.mixtures > 1:
                logging.info("iteration %d: %d components, mean score per frame %.4f, %d utterances without an alignment", it + 1, history["components"][it], s,
                             len(history["failed"][it]))
            else:
                logging.info("iteration %d: mean score per frame %.4f, %d utterances without an alignment", it + 1, s, len(history["failed"][it]))
        if args.model_out:
            al.model.save(args.model_out)
    res = al.align(feats, trs, ids=ids, **word_kw)
    os.makedirs(args.textgrid_out, exist_ok=True)
    if args.durations_out:
        os.makedirs(args.durations_out, exist_ok=True)
    failed, frames, total = [], 0, 0.0
    for (u, _, _, n), r in zip(utts, res):
        if not r["ok"]:
            failed.append(u)
            continue
        frames, total = frames + sum(r["durations"]), total + r["score"]
        rows = textgrid.frame_intervals(r["phones"], r["durations"], args.fs, args.hop, n)
        tiers = {"phones": rows}
        if lex is not None:
            tiers["words"] = word_tier(r, args.fs, args.hop, n)
        textgrid.write_textgrid(os.path.join(args.textgrid_out, u + ".TextGrid"), tiers, rows[-1][1])
        if args.durations_out:
            np.save(os.path.join(args.durations_out, u + ".npy"), np.asarray(r["durations"], dtype=np.int64))
    doc = dict(n_utt=len(ids), n_aligned=len(ids) - len(failed), not_aligned=failed, score_per_frame=total / max(frames, 1),
               iterations=[dict(score_per_frame=s, not_aligned=f) for s, f in zip(history["score"], history["failed"])],
               settings=dict(states=al.K, optional=sorted(al.optional), phones=al.phones, trained=model is None, model=args.model, features=af.settings,
                             resample=bool(args.resample)))
    if lex is not None:
        variants = {}
        for r in res:
            if r["ok"]:
                for w, v in zip(r["words"], r["pronunciations"]):
                    variants.setdefault(w, [0] * len(lex.lookup(w)))[v] += 1
        doc["lexicon"] = dict(path=args.lexicon, boundary_silence=not args.no_boundary_silence, oov=args.oov, skipped=skipped,
                              variants={w: variants[w] for w in sorted(variants)})
        if args.pronunciations_out:
            with open(args.pronunciations_out, "w", encoding="utf-8") as f:
                for u, r in zip(ids, res):
                    if r["ok"]:
                        f.write(u + " " + " ".join(r["phones"]) + "\n")
    mixtures = al.model.max_components if model is not None else args.mixtures
    if mixtures > 1:  # with single Gaussians the report is the one it has always been, byte for byte
        doc["settings"]["mixtures"] = mixtures
        for entry, g in zip(doc["iterations"], history["components"]):
            entry["components"] = g
    return doc


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO if args.verbose else logging.WARN, format="%(asctime)s %(levelname)s: %(message)s")
    doc = align(args)
    torch.cuda.synchronize()
    if args.report:
        with open(args.report, "w") as f:
            json.dump(doc, f, indent=1)
    print("align: %d of %d utterances aligned, mean score per frame %.4f" % (doc["n_aligned"], doc["n_utt"], doc["score_per_frame"]))
    return doc


if __name__ == "__main__":
    main()
