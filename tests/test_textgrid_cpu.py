"""fcl_taco2_amd/textgrid.py: the TextGrid parser on files generated here (long and short format, UTF-16, an escaped quote), and the reference's
alignment rules (preprocess.py lines 165-196) on hand-built tiers whose expected phones and durations are written out by hand."""
import json

import pytest

from fcl_taco2_amd import textgrid as TG

PHONES = [(0.0, 0.1, "sil"), (0.1, 0.35, "HH"), (0.35, 0.5, 'say "AH0"'), (0.5, 0.75, ""), (0.75, 1.25, "L OW1 ü")]
WORDS = [(0.0, 0.1, ""), (0.1, 1.25, "hello")]


def q(s):
    return '"%s"' % s.replace('"', '""')


def long_format(tiers, points=None):
    out = ['File type = "ooTextFile"', 'Object class = "TextGrid"', "", "xmin = 0 ", "xmax = 1.25 ", "tiers? <exists> ", "size = %d " % (len(tiers) + len(points or {})), "item []: "]
    k = 0
    for name, rows in tiers.items():
        k += 1
        out += ["    item [%d]:" % k, '        class = "IntervalTier" ', "        name = %s " % q(name), "        xmin = 0 ", "        xmax = 1.25 ",
                "        intervals: size = %d " % len(rows)]
        for i, (a, b, t) in enumerate(rows, 1):
            out += ["        intervals [%d]:" % i, "            xmin = %r " % a, "            xmax = %r " % b, "            text = %s " % q(t)]
    for name, rows in (points or {}).items():
        k += 1
        out += ["    item [%d]:" % k, '        class = "TextTier" ', "        name = %s " % q(name), "        xmin = 0 ", "        xmax = 1.25 ", "        points: size = %d " % len(rows)]
        for i, (a, t) in enumerate(rows, 1):
            out += ["        points [%d]:" % i, "            number = %r " % a, "            mark = %s " % q(t)]
    return "\n".join(out) + "\n"


def short_format(tiers):
    out = ['File type = "ooTextFile"', 'Object class = "TextGrid"', "", "0", "1.25", "<exists>", str(len(tiers))]
    for name, rows in tiers.items():
        out += ['"IntervalTier"', q(name), "0", "1.25", str(len(rows))]
        for a, b, t in rows:
            out += [repr(a), repr(b), q(t)]
    return "\n".join(out) + "\n"


def test_long_short_utf16_and_escaped_quotes_parse_alike(tmp_path):
    tiers = {"words": WORDS, "phones": PHONES}
    files = {"long.TextGrid": long_format(tiers).encode("utf-8"), "short.TextGrid": short_format(tiers).encode("utf-8"),
             "bom8.TextGrid": b"\xef\xbb\xbf" + long_format(tiers).encode("utf-8"), "u16le.TextGrid": long_format(tiers).encode("utf-16"),
             "u16be.TextGrid": b"\xfe\xff" + short_format(tiers).encode("utf-16-be"), "crlf.TextGrid": long_format(tiers).replace("\n", "\r\n").encode("utf-8")}
    for name, raw in files.items():
        (tmp_path / name).write_bytes(raw)
        got = TG.read_textgrid(str(tmp_path / name))
        assert got == tiers, name  # the same floats, the quote unescaped, the empty label kept, the non-ASCII label intact
    assert got["phones"][2][2] == 'say "AH0"' and got["phones"][3][2] == ""


def test_refusals_name_the_file(tmp_path):
    p = tmp_path / "x.TextGrid"
    p.write_text(long_format({"words": WORDS}))
    with pytest.raises(ValueError, match=r"x\.TextGrid: no interval tier named 'phones' \(tiers: words\)"):
        TG.read_textgrid(str(p))
    assert TG.read_textgrid(str(p), require=None) == {"words": WORDS}
    p.write_text(long_format({"words": WORDS}, points={"phones": [(0.5, "x")]}))
    with pytest.raises(ValueError, match=r"x\.TextGrid: tier 'phones' is a point tier"):
        TG.read_textgrid(str(p))
    whole = short_format({"phones": PHONES})
    for bad in (whole[: len(whole) // 2], whole.replace("ooTextFile", "ooBinaryFile"), whole.replace('"IntervalTier"', '"Tier"'), whole + "7\n", "",
                whole.replace("\n5\n", "\n5.5\n")):
        p.write_text(bad)
        with pytest.raises(ValueError, match=r"x\.TextGrid: malformed TextGrid"):
            TG.read_textgrid(str(p))
    p.write_bytes(b"\xff\xff\xff\xff")
    with pytest.raises(ValueError, match=r"x\.TextGrid: malformed TextGrid"):
        TG.read_textgrid(str(p))


# fs 22050, hop 256.  Sample bounds int(t * 22050) truncate: 0.1 s -> 2205, 0.29 s -> 6394 (6394.5 is not rounded up); frames int(sample / 256).
def test_alignment_rules_on_hand_built_tiers():
    A = lambda rows, **kw: TG.alignment(rows, 22050, 256, **kw)
    # bounds 0, 2205, 6394, 11025, 22050 samples -> frames 0, 8, 24, 43, 86
    tier = [(0.0, 0.1, "sil"), (0.1, 0.29, "AH0"), (0.29, 0.5, "B"), (0.5, 1.0, "IY1")]
    assert A(tier) == (["sil", "AH0", "B", "IY1"], [8, 16, 19, 43])  # a phone at the end: untouched, no merge
    for last in ("", "sp", "spn"):  # the last label becomes sil; second-to-last is a phone: no merge
        assert A(tier[:3] + [(0.5, 1.0, last)]) == (["sil", "AH0", "B", "sil"], [8, 16, 19, 43])
    for prev in ("sil", "sp", "spn"):  # merge: 'sil' from the first one's start (6394 -> frame 24) to the last one's end (22050 -> frame 86)
        for last in ("sil", "", "sp", "spn"):
            assert A(tier[:2] + [(0.29, 0.5, prev), (0.5, 1.0, last)]) == (["sil", "AH0", "sil"], [8, 16, 62])
    assert A(tier[:2] + [(0.29, 0.5, ""), (0.5, 1.0, "")]) == (["sil", "AH0", "", "sil"], [8, 16, 19, 43])  # '' before the end is no silence: no merge
    assert A(tier[:2] + [(0.29, 0.5, "sp"), (0.5, 1.0, "IY1")]) == (["sil", "AH0", "sp", "IY1"], [8, 16, 19, 43])  # sp inside stays
    # truncation, not rounding: 0.0116 s -> int(255.78) = 255 samples -> frame 0; 0.01161 s -> int(256.0005) = 256 -> frame 1; durations of 0
    assert A([(0.0, 0.0116, "a"), (0.0116, 0.01161, "b"), (0.01161, 0.0117, "c"), (0.0117, 0.1, "d")]) == (["a", "b", "c", "d"], [0, 1, 0, 7])
    assert int(0.1 * 22050) == 2205 and int(0.29 * 22050) == 6394
    # an empty label inside: kept as read, or renamed after the rules have run
    mid = [(0.0, 0.1, "sil"), (0.1, 0.29, ""), (0.29, 0.5, "B"), (0.5, 1.0, "")]
    assert A(mid) == (["sil", "", "B", "sil"], [8, 16, 19, 43])
    assert A(mid, empty_label="sp") == (["sil", "sp", "B", "sil"], [8, 16, 19, 43])
    # fewer than two intervals: the merge rule is skipped (the reference indexes parts[-2] and crashes)
    assert A([(0.0, 1.0, "")]) == (["sil"], [86]) and A([(0.0, 1.0, "AH0")]) == (["AH0"], [86])
    with pytest.raises(ValueError, match="no intervals"):
        A([])
    # other rates: 16 kHz, hop 200
    assert TG.alignment([(0.0, 0.0125, "a"), (0.0125, 0.5, "sp")], 16000, 200) == (["a", "sil"], [1, 39])


def test_symbol_table_and_lookup(tmp_path):
    raw = ["sp", "AH0", "B", "", "AH0", "sp"]
    table = TG.symbol_table(raw + ["sil"])  # 'sil' only comes out of the end-of-utterance rule
    assert table == {"": "1", "AH0": "2", "B": "3", "sil": "4", "sp": "5", "PAD": 0}
    assert TG.token_ids(["sil", "B", ""], table, "u1") == ["4", "3", "1"]
    path = tmp_path / "phn2idx.json"
    TG.write_symbol_table(str(path), table)
    assert path.read_text() == '{\n    "": "1",\n    "AH0": "2",\n    "B": "3",\n    "PAD": 0,\n    "sil": "4",\n    "sp": "5"\n}'
    loaded = TG.load_symbol_table(str(path))
    assert loaded == table
    with pytest.raises(ValueError, match="utterance u7: phone 'ZH' is not in the symbol table"):
        TG.token_ids(["B", "ZH"], loaded, "u7")
    with pytest.raises(ValueError, match="PAD"):
        TG.symbol_table(["a", "PAD"])
    path.write_text(json.dumps({"a": "1"}))
    with pytest.raises(ValueError, match="not a phn2idx.json"):
        TG.load_symbol_table(str(path))
