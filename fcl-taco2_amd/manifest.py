"""The json manifests `train` and `decode` read, and the train / validation / test split: the last third of the reference's preprocessing step
(make_json, preprocess.py lines 199-241, and the split of lines 306-310), host only."""
import json

import numpy as np

MAX_PHN_DUR = 50


def entry(utt, phones, token_ids, durations, frames, n_mels, mel, dur, f0, en):
    """one utterance of a manifest: phones / token_ids / durations (adjusted: they sum to `frames`) per phoneme, and the four feature files"""
    return dict(utt=utt, phones=list(phones), token_ids=[str(i) for i in token_ids], durations=[int(d) for d in durations], frames=int(frames),
                n_mels=int(n_mels), mel=mel, dur=dur, f0=f0, en=en)


def write_manifest(path, entries, num_phns, speaker="LJ", max_phn_dur=MAX_PHN_DUR):
    """{"utts": {utt: ...}} as make_json writes it: input1 the mel [T, n_mels], input2 durations_MFA [P, 1], input3 f0 [P, 1], input4 en [P, 1], each
    with filetype "npy"; output[0] target1 with shape [P, num_phns] and text / token / tokenid space-joined; utt2spk.  Utterances whose largest
    duration exceeds max_phn_dur are left out (they still counted in the statistics, as in the reference).  Returns the ids written."""
    utts = {}
    for e in entries:
        P = len(e["phones"])
        if not (len(e["token_ids"]) == len(e["durations"]) == P):
            raise ValueError("utterance %s: %d phones, %d token ids, %d durations" % (e["utt"], P, len(e["token_ids"]), len(e["durations"])))
        if max(e["durations"]) > max_phn_dur:
            continue
        inputs = [dict(feat=e["mel"], filetype="npy", name="input1", shape=[e["frames"], e["n_mels"]]),
                  dict(feat=e["dur"], filetype="npy", name="input2", shape=[P, 1]),
                  dict(feat=e["f0"], filetype="npy", name="input3", shape=[P, 1]),
                  dict(feat=e["en"], filetype="npy", name="input4", shape=[P, 1])]
        text = " ".join(e["phones"])
        utts[e["utt"]] = dict(input=inputs, output=[dict(name="target1", shape=[P, int(num_phns)], text=text, token=text, tokenid=" ".join(e["token_ids"]))],
                              utt2spk=speaker)
    with open(path, "w", encoding="utf-8") as f:
        json.dump({"utts": utts}, f, indent=4, ensure_ascii=False, sort_keys=True, separators=(",", ": "))
    return sorted(utts)


def split_ids(ids, n_valid, n_test, seed=0):
    """(train, valid, test): a numpy.random.RandomState(seed) permutation of the sorted ids; the first n_valid are validation, the next n_test test,
    the rest training, each in sorted order.  (The reference's split is unseeded: there is nothing to match.)  More held-out utterances than the
    corpus has, or none left to train on, is refused."""
    ids = sorted(ids)
    if len(set(ids)) != len(ids):
        raise ValueError("duplicate utterance ids")
    if n_valid < 0 or n_test < 0 or n_valid + n_test >= len(ids):
        raise ValueError("%d validation + %d test utterances asked for, the corpus has %d (at least one must remain for training)" % (n_valid, n_test, len(ids)))
    perm = [ids[i] for i in np.random.RandomState(seed).permutation(len(ids))]
    return sorted(perm[n_valid + n_test :]), sorted(perm[:n_valid]), sorted(perm[n_valid : n_valid + n_test])
