"""Praat TextGrid -> phoneme sequence and durations in frames: the first third of the reference's preprocessing step (preprocess.py lines 158-196,
270-291), host only.  The reference reads the aligner's TextGrids with a third-party reader that is not available here; this module parses the text
formats itself and restates the reference's integer rules exactly.

    tiers = read_textgrid("LJ001-0001.TextGrid")            # {"phones": [(xmin, xmax, text), ...], "words": [...]}
    phones, durations = alignment(tiers["phones"], 22050, 256)
    phn2idx = symbol_table(labels)                            # the reference's phn2idx.json
"""
import json
import math
import re

SIL_PHONES = ("sil", "sp", "spn")
END_AS_SIL = ("", "sp", "spn")

# the values of a TextGrid in file order, long or short format: quoted strings ("" is an escaped quote), <exists> flags, and free-standing numbers
# (the long format's `intervals [3]:` indices stand in brackets and are no values)
_TOKEN = re.compile(r'"((?:[^"]|"")*)"|(<exists>|<absent>)|(?<![\w\[.+-])([-+]?\d+(?:\.\d*)?(?:[eE][-+]?\d+)?)(?![\w\].])')


def _decode(raw):
    if raw[:2] in (b"\xff\xfe", b"\xfe\xff"):
        return raw.decode("utf-16")
    if raw[:3] == b"\xef\xbb\xbf":
        return raw[3:].decode("utf-8")
    return raw.decode("utf-8")


class _Values(object):
    def __init__(self, text, path):
        self.path, self.i = path, 0
        self.v = [("s", m.group(1).replace('""', '"')) if m.group(1) is not None else ("f", m.group(2)) if m.group(2) else ("n", m.group(3))
                  for m in _TOKEN.finditer(text)]

    def take(self, kind, what):
        if self.i >= len(self.v) or self.v[self.i][0] != kind:
            got = "the end of the file" if self.i >= len(self.v) else repr(self.v[self.i][1])
            raise ValueError("%s: malformed TextGrid: expected %s, found %s" % (self.path, what, got))
        self.i += 1
        return self.v[self.i - 1][1]

    def number(self, what):
        return float(self.take("n", what))

    def count(self, what):
        s = self.take("n", what)
        if not s.isdigit():
            raise ValueError("%s: malformed TextGrid: %s must be a count, found %r" % (self.path, what, s))
        return int(s)


def read_textgrid(path, require="phones"):
    """Reads a Praat TextGrid in the long or the short text format (UTF-8, or UTF-16 with a byte-order mark; `""` inside a quoted string is a quote)
    -> {tier name: [(xmin, xmax, text)]} of its interval tiers, times as float64; of two tiers with one name the first counts.  A missing `require`
    tier, a point tier under that name and a malformed file are refused naming the file."""
    with open(path, "rb") as f:
        raw = f.read()
    try:
        text = _decode(raw)
    except UnicodeDecodeError as e:
        raise ValueError("%s: malformed TextGrid: not UTF-8 and no UTF-16 byte-order mark (%s)" % (path, e))
    v = _Values(text, path)
    if v.take("s", 'File type = "ooTextFile"') != "ooTextFile" or v.take("s", 'Object class = "TextGrid"') != "TextGrid":
        raise ValueError("%s: malformed TextGrid: not an ooTextFile of class TextGrid" % path)
    v.number("xmin")
    v.number("xmax")
    tiers, points = {}, set()
    if v.take("f", "the tiers? flag") == "<exists>":
        for _ in range(v.count("the number of tiers")):
            cls, name = v.take("s", "a tier class"), v.take("s", "a tier name")
            v.number("the tier's xmin")
            v.number("the tier's xmax")
            n = v.count("the tier's size")
            if cls == "IntervalTier":
                rows = []
                for _ in range(n):
                    a, b = v.number("an interval's xmin"), v.number("an interval's xmax")
                    rows.append((a, b, v.take("s", "an interval's text")))
                tiers.setdefault(name, rows)
            elif cls == "TextTier":
                for _ in range(n):
                    v.number("a point's time")
                    v.take("s", "a point's mark")
                points.add(name)
            else:
                raise ValueError("%s: malformed TextGrid: tier class %r" % (path, cls))
    if v.i != len(v.v):
        raise ValueError("%s: malformed TextGrid: %d values after the last tier" % (path, len(v.v) - v.i))
    if require is not None and require not in tiers:
        raise ValueError("%s: %s" % (path, "tier %r is a point tier; an interval tier is needed" % require if require in points else
                                     "no interval tier named %r (tiers: %s)" % (require, ", ".join(sorted(tiers)) or "none")))
    return tiers


def alignment(intervals, fs, hop, empty_label=None):
    """[(xmin, xmax, text)] of the `phones` tier -> (phones, durations in frames), the rules of preprocess.py lines 165-196 exactly:
    sample bounds int(start fs), int(end fs) in float64; a last label in {'', 'sp', 'spn'} becomes 'sil'; if the second-to-last label is in
    {'sil', 'sp', 'spn'} and the last is 'sil' the two merge ('sil', the first one's start, the last one's end); duration = int(e / hop) - int(s / hop)
    on the sample bounds.  A tier with fewer than two intervals skips the merge rule (the reference indexes out of range there and crashes); an empty
    tier is refused.  An interval with empty text elsewhere is kept as read, so that the phonemes cover the frames contiguously; empty_label renames
    it after the rules above have run."""
    if len(intervals) == 0:
        raise ValueError("the phones tier has no intervals")
    parts = [[int(s * fs), int(e * fs), p] for s, e, p in intervals]
    if parts[-1][2] in END_AS_SIL:
        parts[-1][2] = "sil"
    if len(parts) >= 2 and parts[-2][2] in SIL_PHONES and parts[-1][2] == "sil":
        parts[-2][2] = "sil"
        parts[-2][1] = parts[-1][1]
        parts = parts[:-1]
    phones = [empty_label if p == "" and empty_label is not None else p for _, _, p in parts]
    durations = [int(e / hop) - int(s / hop) for s, e, _ in parts]
    return phones, durations


def frame_intervals(phones, durations, fs, hop, n_samples):
    """Durations in frames -> [(xmin, xmax, text)] that alignment() reads back: a boundary at frame k stands at (k hop + 0.5) / fs seconds, so that
    int(time fs) == k hop whatever the rounding of the division; the first interval begins at 0 and the last ends at the wav's end, n_samples / fs
    (moved up by single ulps until int(time fs) == n_samples).  alignment() therefore returns these durations with the last one less by 1 when they
    sum to n_samples // hop + 1, the frame count of features.py: what preprocess's own last-duration rule restores."""
    if len(phones) != len(durations) or not phones:
        raise ValueError("frame_intervals: %d phones and %d durations" % (len(phones), len(durations)))
    edges = [0]
    for d in durations:
        if int(d) < 0:
            raise ValueError("frame_intervals: a negative duration")
        edges.append(edges[-1] + int(d))
    if (edges[-1] - 1) * int(hop) > int(n_samples):
        raise ValueError("frame_intervals: %d frames begin past the end of %d samples at hop %d" % (edges[-1], int(n_samples), int(hop)))
    times = [0.0] + [(k * int(hop) + 0.5) / float(fs) for k in edges[1:-1]]
    end = int(n_samples) / float(fs)
    while int(end * fs) < int(n_samples):
        end = math.nextafter(end, math.inf)
    times.append(end)
    return [(times[i], times[i + 1], str(p)) for i, p in enumerate(phones)]


def write_textgrid(path, tiers, xmax):
    """{tier name: [(xmin, xmax, text)]} (or a list of (name, intervals)) -> a Praat TextGrid in the long text format, interval tiers only.  Times
    are written with repr, the shortest digits that read back to the same float64."""
    items = list(tiers.items()) if isinstance(tiers, dict) else list(tiers)
    q = lambda s: '"%s"' % str(s).replace('"', '""')
    out = ['File type = "ooTextFile"', 'Object class = "TextGrid"', "", "xmin = 0", "xmax = %r" % float(xmax), "tiers? <exists>", "size = %d" % len(items),
           "item []:"]
    for i, (name, rows) in enumerate(items, 1):
        out += ["    item [%d]:" % i, '        class = "IntervalTier"', "        name = %s" % q(name), "        xmin = 0", "        xmax = %r" % float(xmax),
                "        intervals: size = %d" % len(rows)]
        for j, (a, b, text) in enumerate(rows, 1):
            out += ["        intervals [%d]:" % j, "            xmin = %r" % float(a), "            xmax = %r" % float(b), "            text = %s" % q(text)]
    with open(path, "w", encoding="utf-8") as f:
        f.write("\n".join(out) + "\n")


def symbol_table(all_labels):
    """The reference's phn2idx.json (preprocess.py lines 277-281): the sorted distinct labels numbered from 1, as strings, and "PAD": 0.  all_labels:
    the raw labels of every TextGrid plus whatever alignment() made of them (a 'sil' that only the end-of-utterance rule produces would otherwise be
    missing, which is where the reference fails with a KeyError)."""
    table = {p: str(i) for i, p in enumerate(sorted(set(all_labels)), 1)}
    if "PAD" in table:
        raise ValueError("the label PAD is reserved for the padding index")
    table["PAD"] = 0
    return table


def write_symbol_table(path, table):
    with open(path, "w", encoding="utf-8") as f:
        json.dump(table, f, indent=4, ensure_ascii=False, sort_keys=True, separators=(",", ": "))


def load_symbol_table(path):
    """an existing phn2idx.json: {label: "index", "PAD": 0}"""
    with open(path, "rb") as f:
        table = json.load(f)
    if not isinstance(table, dict) or table.get("PAD") != 0:
        raise ValueError('%s: not a phn2idx.json (an object with "PAD": 0)' % path)
    return table


def token_ids(phones, table, utt):
    """the phones' indices as the strings the manifest joins; a phone the table lacks is refused naming it and the utterance"""
    for p in phones:
        if p not in table or p == "PAD":
            raise ValueError("utterance %s: phone %r is not in the symbol table" % (utt, p))
    return [str(table[p]) for p in phones]
