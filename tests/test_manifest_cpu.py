"""fcl_taco2_amd/manifest.py: the manifest writer against a literal expected file and through the readers of `train` and `decode`; the seeded split."""
import numpy as np
import pytest

from fcl_taco2_amd import manifest as MF

EXPECTED = """{
    "utts": {
        "LJ001-0001": {
            "input": [
                {
                    "feat": "data/mels/LJ001-0001.npy",
                    "filetype": "npy",
                    "name": "input1",
                    "shape": [
                        12,
                        80
                    ]
                },
                {
                    "feat": "data/durations_MFA/LJ001-0001.npy",
                    "filetype": "npy",
                    "name": "input2",
                    "shape": [
                        3,
                        1
                    ]
                },
                {
                    "feat": "data/f0/LJ001-0001.npy",
                    "filetype": "npy",
                    "name": "input3",
                    "shape": [
                        3,
                        1
                    ]
                },
                {
                    "feat": "data/en/LJ001-0001.npy",
                    "filetype": "npy",
                    "name": "input4",
                    "shape": [
                        3,
                        1
                    ]
                }
            ],
            "output": [
                {
                    "name": "target1",
                    "shape": [
                        3,
                        41
                    ],
                    "text": "sil ü AH0",
                    "token": "sil ü AH0",
                    "tokenid": "40 7 2"
                }
            ],
            "utt2spk": "LJ"
        }
    }
}"""


def one(utt="LJ001-0001", durations=(2, 4, 6), root="data"):
    return MF.entry(utt, ["sil", "ü", "AH0"], [40, 7, 2], durations, sum(durations), 80, *("%s/%s/%s.npy" % (root, d, utt) for d in ("mels", "durations_MFA", "f0", "en")))


def test_one_utterance_manifest_is_the_literal_layout(tmp_path):
    p = tmp_path / "train_data.json"
    assert MF.write_manifest(str(p), [one()], 41) == ["LJ001-0001"]
    assert p.read_text(encoding="utf-8") == EXPECTED


def test_manifest_goes_through_the_training_and_decoding_readers(tmp_path):
    from fcl_taco2_amd import decode, train

    rng = np.random.RandomState(0)
    specs = {"ub": (3, 5, 4), "ua": (2, 4, 6), "uc": (1, 51, 2)}  # uc: a phoneme of 51 frames, over the default limit of 50
    entries = []
    for u, d in specs.items():
        for k, a in (("mels", rng.randn(sum(d), 80).astype(np.float32)), ("durations_MFA", np.array(d, dtype=np.int64)),
                     ("f0", rng.randn(3, 1).astype(np.float32)), ("en", rng.randn(3, 1).astype(np.float32))):
            (tmp_path / k).mkdir(exist_ok=True)
            np.save(tmp_path / k / (u + ".npy"), a)
        entries.append(one(u, d, str(tmp_path)))
    p = tmp_path / "train_data.json"
    assert MF.write_manifest(str(p), entries, 41, speaker="S1") == ["ua", "ub"]  # uc is left out
    assert MF.write_manifest(str(tmp_path / "all.json"), entries, 41, max_phn_dur=51) == ["ua", "ub", "uc"]
    man = train.read_train_manifest(str(p))
    assert sorted(m["id"] for m in man) == ["ua", "ub"] and all(m["num_phns"] == 41 and m["ilen"] == 3 for m in man)
    assert {m["id"]: m["olen"] for m in man} == {"ua": 12, "ub": 12}
    xs, ys, _, ds, f0, en = train.load_batch(man)
    assert all(x.tolist() == [40, 7, 2] for x in xs) and [y.shape for y in ys] == [(12, 80), (12, 80)]
    assert all(int(d.sum()) == y.shape[0] and d.shape == f.shape == e.shape == (3, 1) for d, y, f, e in zip(ds, ys, f0, en))
    utts = decode.read_manifest(str(p))  # input[1] is the durations file, not a speaker embedding
    assert sorted(u[0] for u in utts) == ["ua", "ub"] and all(len(u) == 2 and u[1].tolist() == [40, 7, 2] for u in utts)
    with pytest.raises(ValueError, match="utterance bad: 3 phones, 3 token ids, 2 durations"):
        MF.write_manifest(str(p), [MF.entry("bad", ["a", "b", "c"], [1, 2, 3], [4, 5], 9, 80, "m", "d", "f", "e")], 41)


def test_split_is_deterministic_disjoint_and_complete():
    ids = ["u%03d" % i for i in range(40)]
    tr, va, te = MF.split_ids(ids[::-1], 5, 7, seed=3)
    assert (tr, va, te) == MF.split_ids(ids, 5, 7, seed=3)  # the order the ids arrive in does not matter
    assert len(va) == 5 and len(te) == 7 and len(tr) == 28 and sorted(tr + va + te) == ids
    perm = [ids[i] for i in np.random.RandomState(3).permutation(40)]
    assert va == sorted(perm[:5]) and te == sorted(perm[5:12]) and tr == sorted(perm[12:])
    assert MF.split_ids(ids, 5, 7, seed=4) != (tr, va, te)
    assert MF.split_ids(ids, 0, 0) == (ids, [], [])
    for nv, nt in ((30, 11), (40, 0), (20, 20), (-1, 2)):
        with pytest.raises(ValueError, match="the corpus has 40"):
            MF.split_ids(ids, nv, nt)
    with pytest.raises(ValueError, match="duplicate"):
        MF.split_ids(["a", "a", "b"], 1, 0)
