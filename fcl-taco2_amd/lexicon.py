"""A pronunciation lexicon for the forced aligner (alignment.build_word_graph, `align --lexicon`), host only.

    lex = read_lexicon("cmudict.txt")       # lines `WORD PH PH ...`, one pronunciation per line
    lex.lookup("The")                       # [["DH", "AH0"], ["DH", "IY0"]]: every pronunciation, in file order; None for a word it lacks

A trailing `(n)` on the word (`THE(2)`) is stripped; lines that begin with `;;;` or `#` and empty lines are skipped; identical pronunciations of one
word are merged; file order is variant order.  A word keeps at most 7 pronunciations -- what the 8 predecessor slots of a lattice row hold beside one
silence --: the later ones are dropped and the word is named in a logged warning.  Words are compared after normalise() on both sides; the labels are
used exactly as the lexicon spells them (stress digits are the user's business).  There is no G2P: a word the lexicon lacks is the caller's to refuse."""
import logging
import re

VARIANTS_MAX = 7
PUNCTUATION = "\"'`.,;:!?()[]{}<>-–—‘’“”…"  # stripped from both ends of a token; inner apostrophes and hyphens stay
_SUFFIX = re.compile(r"\(\d+\)$")


def normalise(token):
    """str.lower(), then the characters of PUNCTUATION stripped from both ends; None for a token of which nothing is left"""
    t = str(token).lower().strip(PUNCTUATION)
    return t or None


def normalise_words(tokens):
    """the normalised tokens of a transcript, those that become empty dropped"""
    return [w for w in (normalise(t) for t in tokens) if w is not None]


class Lexicon(object):
    """{normalised word: [pronunciation, ...]}, a pronunciation being a list of labels"""

    def __init__(self, entries=None):
        self.entries = {}
        self.truncated = []  # the words that had more than VARIANTS_MAX pronunciations
        for word, prons in (entries or {}).items():
            for p in prons:
                self.add(word, p)

    def add(self, word, pron):
        w, pron = normalise(_SUFFIX.sub("", str(word))), [str(p) for p in pron]
        if w is None or not pron:
            raise ValueError("lexicon: the entry %r has no word or no labels" % (word,))
        have = self.entries.setdefault(w, [])
        if pron in have:
            return
        if len(have) >= VARIANTS_MAX:
            if w not in self.truncated:
                self.truncated.append(w)
            return
        have.append(pron)

    def lookup(self, token):
        w = normalise(token)
        return None if w is None else self.entries.get(w)

    def __contains__(self, token):
        return self.lookup(token) is not None

    def __len__(self):
        return len(self.entries)

    def labels(self, words=None):
        """the sorted labels of the pronunciations of `words` (of every word without them); unknown words are passed over"""
        prons = self.entries.values() if words is None else [self.lookup(w) or [] for w in words]
        return sorted(set(p for vs in prons for v in vs for p in v))


def read_lexicon(path):
    """`WORD PH PH ...` lines -> Lexicon; a line with a word and no labels is refused naming the file and the line"""
    lex = Lexicon()
    with open(path, encoding="utf-8") as f:
        for no, ln in enumerate(f, 1):
            if ln.startswith(";;;") or ln.startswith("#"):
                continue
            parts = ln.split()
            if not parts:
                continue
            if len(parts) < 2 or normalise(_SUFFIX.sub("", parts[0])) is None:
                raise ValueError("%s:%d: a lexicon line is `WORD PH PH ...`, got %r" % (path, no, ln.strip()))
            lex.add(parts[0], parts[1:])
    if not len(lex):
        raise ValueError("no pronunciations in %s" % path)
    if lex.truncated:
        logging.warning("lexicon %s: more than %d pronunciations, the first %d kept: %s", path, VARIANTS_MAX, VARIANTS_MAX, ", ".join(lex.truncated))
    return lex
