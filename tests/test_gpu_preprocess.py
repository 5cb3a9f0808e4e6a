"""python -m fcl_taco2_amd.preprocess end to end on four tiny wavs with generated TextGrids, two at 22050 Hz and two holding the same signals at
16000 Hz: the reference's directory layout plus phn2idx.json and the three manifests, the resampled path byte for byte against Resampler +
FeatureExtractor on the same samples, and extract_features with and without --resample."""
import json
import os
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FS, HOP = 22050, 256
UTTS = {"ua": (22050, 140.0, 4000 / 22050), "ub": (22050, 190.0, 4800 / 22050), "va": (16000, 140.0, 4000 / 22050), "vb": (16000, 190.0, 4800 / 22050)}  # rate, F0, seconds
LABELS = ["sil", "AH0", "B", ""]  # the empty last label becomes 'sil' by the end-of-utterance rule


def write_wav(path, x, rate):
    pcm = np.clip(np.rint(np.asarray(x, dtype=np.float64) * 32767.0), -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(rate)
        f.writeframes(pcm.tobytes())
    return pcm.astype(np.float32) / np.float32(32768.0)


def write_textgrid(path, seconds):
    cuts = [0.0, 0.2 * seconds, 0.5 * seconds, 0.8 * seconds, seconds]
    out = ['File type = "ooTextFile"', 'Object class = "TextGrid"', "", "xmin = 0", "xmax = %r" % seconds, "tiers? <exists>", "size = 1", "item []:", "    item [1]:",
           '        class = "IntervalTier"', '        name = "phones"', "        xmin = 0", "        xmax = %r" % seconds, "        intervals: size = 4"]
    for i, lab in enumerate(LABELS):
        out += ["        intervals [%d]:" % (i + 1), "            xmin = %r" % cuts[i], "            xmax = %r" % cuts[i + 1], '            text = "%s"' % lab]
    path.write_text("\n".join(out) + "\n")


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    assert torch.cuda.is_available()
    root = tmp_path_factory.mktemp("corpus")
    (root / "wavs").mkdir()
    (root / "TextGrid").mkdir()
    samples = {}
    for u, (rate, f0, seconds) in UTTS.items():
        t = np.arange(int(round(seconds * rate))) / rate
        x = 0.4 * sum(np.sin(2 * np.pi * k * f0 * t) / k for k in (1, 2, 3, 4))
        samples[u] = write_wav(root / "wavs" / (u + ".wav"), x, rate)
        write_textgrid(root / "TextGrid" / (u + ".TextGrid"), seconds)
    return root, samples


def launches(fn):
    from fcl_taco2_amd import _lib

    _lib.prof_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, set(_lib.prof_collect())
    finally:
        _lib.prof_enable(False)


def test_preprocess_end_to_end(corpus, tmp_path):
    from fcl_taco2_amd import extract_features as X, features, preprocess, resample, train

    root, samples = corpus
    out = tmp_path / "data"
    argv = ["--data-root", str(root), "--textgrid-root", str(root / "TextGrid"), "--feature-root", str(out), "--n-valid", "1", "--n-test", "1", "--batch-frames", "40",
            "--verbose", "0"]
    res, seen = launches(lambda: preprocess.main(argv))
    assert {"rs_resample_kernel", "fx_logmel_kernel<1024>", "fx_segment_mean_kernel"} <= seen, sorted(seen)
    assert sorted(os.listdir(out)) == ["durations_MFA", "durations_MFA-ori", "en", "en-ori", "f0", "f0-ori", "f0_en_stats.npy", "mel_stats.npy", "mels", "mels-ori",
                                       "phn2idx.json", "test_data.json", "train_data.json", "val_data.json"]
    assert json.load(open(out / "phn2idx.json")) == {"": "1", "AH0": "2", "B": "3", "sil": "4", "PAD": 0} == res["phn2idx"]
    assert res["ids"] == ["ua", "ub", "va", "vb"] and len(res["train"]) == 2 and len(res["valid"]) == len(res["test"]) == 1
    assert sorted(res["train"] + res["valid"] + res["test"]) == res["ids"]
    n_out = {"ua": 4000, "ub": 4800, "va": resample.out_samples(len(samples["va"]), 441, 320), "vb": resample.out_samples(len(samples["vb"]), 441, 320)}
    assert 3990 <= n_out["va"] <= 4000 and 4790 <= n_out["vb"] <= 4800
    for u in res["ids"]:
        T = n_out[u] // HOP + 1
        d, d0, m = np.load(out / "durations_MFA" / (u + ".npy")), np.load(out / "durations_MFA-ori" / (u + ".npy")), np.load(out / "mels-ori" / (u + ".npy"))
        assert d0.shape == (4, 1) and d.shape == (4,) and int(d.sum()) == T == m.shape[0] and np.array_equal(d[:-1], d0[:-1, 0]) and m.shape[1] == 80
        for k in ("mels", "f0", "en", "f0-ori", "en-ori"):
            a = np.load(out / k / (u + ".npy"))
            assert a.shape[0] == (T if k == "mels" else 4) and np.isfinite(a).all(), (u, k)
        assert (np.load(out / "f0-ori" / (u + ".npy")) != 0).any()  # the tracker found the tone
    # the manifests hold every utterance once, with the rule-made 'sil' at the end
    utts = {}
    for mode, part in (("train", res["train"]), ("val", res["valid"]), ("test", res["test"])):
        js = json.load(open(out / (mode + "_data.json")))["utts"]
        assert sorted(js) == sorted(part)
        utts.update(js)
    assert all(v["output"][0]["token"] == "sil AH0 B sil" and v["output"][0]["tokenid"] == "4 2 3 4" and v["output"][0]["shape"] == [4, 5] and v["utt2spk"] == "LJ"
               for v in utts.values())
    man = train.read_train_manifest(str(out / "train_data.json"))
    xs, ys, _, ds, f0, en = train.load_batch(man)
    assert len(xs) == 2 and all(len(x) == len(d) == len(f) == len(e) == 4 and int(d.sum()) == y.shape[0] for x, y, d, f, e in zip(xs, ys, ds, f0, en))
    assert sorted(y.shape[0] for y in ys) == sorted(m["olen"] for m in man)

    # a 16 kHz file: the driver's mels-ori is FeatureExtractor on Resampler output of the same samples, byte for byte
    fx = features.FeatureExtractor(features.FeaturePlan(DEV))
    rs = resample.Resampler(resample.ResamplePlan(DEV, 16000, FS))
    for u in ("va", "vb"):
        y, lens = rs.resample_packed(samples[u], [len(samples[u])])
        mel, _, T = fx.extract_packed(y, lens)
        assert lens == [n_out[u]] and np.load(out / "mels-ori" / (u + ".npy")).tobytes() == mel.cpu().numpy().tobytes()

    # extract_features: today's refusal without --resample, the driver's files with it
    base = ["--wav-dir", str(root / "wavs"), "--verbose", "0"]
    with pytest.raises(ValueError, match=r"va\.wav: sampling rate 16000, --fs is 22050 \(there is no resampler\)"):
        X.main(base + ["--feature-root", str(tmp_path / "o1")])
    (ids, _), seen = launches(lambda: X.main(base + ["--feature-root", str(tmp_path / "o2"), "--resample"]))
    assert ids == res["ids"] and "rs_resample_kernel" in seen
    for u in ids:
        assert (tmp_path / "o2" / "mels-ori" / (u + ".npy")).read_bytes() == (out / "mels-ori" / (u + ".npy")).read_bytes(), u
    with pytest.raises(ValueError, match=r"sampling rate 16000, --fs is 22050"):
        preprocess.main(argv[:5] + [str(tmp_path / "o3"), "--no-resample", "--n-valid", "1", "--n-test", "1", "--verbose", "0"])


def test_unpaired_files_are_refused_by_id(corpus, tmp_path):
    from fcl_taco2_amd import preprocess

    root, _ = corpus
    tg = tmp_path / "TextGrid"
    tg.mkdir()
    for u in ("ua", "ub", "va"):
        (tg / (u + ".TextGrid")).write_bytes((root / "TextGrid" / (u + ".TextGrid")).read_bytes())
    argv = ["--data-root", str(root), "--feature-root", str(tmp_path / "data"), "--n-valid", "1", "--n-test", "1", "--verbose", "0", "--textgrid-root", str(tg)]
    with pytest.raises(ValueError, match=r"1 utterances have a wav but no TextGrid in .* \(first: vb\)"):
        preprocess.main(argv)
    for u in ("vb", "zz"):
        (tg / (u + ".TextGrid")).write_bytes((root / "TextGrid" / "ua.TextGrid").read_bytes())
    with pytest.raises(ValueError, match=r"1 TextGrids in .* have no wav \(first: zz\)"):
        preprocess.main(argv)
    assert not (tmp_path / "data").exists()  # refused before anything was written
