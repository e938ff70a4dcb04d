"""Pseudoalignment with equivalence classes (pseudoalign_device.hpp) restated in plain Python: a dictionary of canonical
k-mers to masks, string windows, Python integers. Independent of the device code and of kmer_color_ref.py's counters; slow (small
inputs only). Not a test module.

class_masks(index, colors, k): canonical k-mer -> the mask of its first window in window order (the class's mask).
fragment(masks, k, records, n_colors): kmers / valid / found / hits[c] of one fragment, summed over its one or two records.
assign(valid, found, hits, P, over, min_kmers): the mask of the rule, in integers.
Aligner: what api.Pseudoaligner answers -- align(), classes(), totals, color_reads(), reset()."""
from matchtigs_amd import synth

ACGT = frozenset("ACGTacgt")


def class_masks(index, colors, k):
    out, i = {}, 0
    for s in index:
        s = s.upper()
        for p in range(len(s) - k + 1):
            out.setdefault(synth.canonical(s[p:p + k]), int(colors[i]))  # the first occurrence wins
            i += 1
    if i != len(colors):
        raise ValueError(f"{len(colors)} masks for {i} windows")
    return out


def masks_by_record(index, record_colors, k):
    """One mask per window, in window order, from one colour per record: every k-mer carries the colours of ALL records that show it."""
    union = {}
    for s, c in zip(index, record_colors):
        s = s.upper()
        for p in range(len(s) - k + 1):
            x = synth.canonical(s[p:p + k])
            union[x] = union.get(x, 0) | (1 << c)
    return [union[synth.canonical(s.upper()[p:p + k])] for s in index for p in range(len(s) - k + 1)]


def found_masks(masks, k, records):
    """The class masks of the valid and found windows of the records, one entry per window (repeats included), and kmers / valid."""
    kmers = valid = 0
    out = []
    for s in records:
        for p in range(len(s) - k + 1):
            kmers += 1
            w = s[p:p + k]
            if not all(c in ACGT for c in w):
                continue
            valid += 1
            x = synth.canonical(w.upper())
            if x in masks:
                out.append(masks[x])
    return kmers, valid, out


def fragment(masks, k, records, n_colors):
    kmers, valid, ms = found_masks(masks, k, records)
    hits = [sum((m >> c) & 1 for m in ms) for c in range(n_colors)]
    return kmers, valid, len(ms), hits


def assign(valid, found, hits, permille=1000, over="found", min_kmers=1):
    denom = {"found": found, "valid": valid}[over]
    mask = 0
    for c, h in enumerate(hits):
        if denom >= min_kmers and h > 0 and h * 1000 >= permille * denom:
            mask |= 1 << c
    return mask


def intersection(masks, k, records, over="found"):
    """The classical rule by sets, no counters: the colours common to every found window (over valid: and every valid window found)."""
    kmers, valid, ms = found_masks(masks, k, records)
    if not ms or (over == "valid" and len(ms) != valid):
        return 0
    out = ~0
    for m in ms:
        out &= m
    return out & ((1 << 64) - 1)


class Aligner:
    def __init__(self, index, colors, n_colors, k, permille=1000, over="found", min_kmers=1):
        if not 1 <= n_colors <= 64 or any(int(x) >> n_colors for x in colors):
            raise ValueError("a colour outside 0 .. n_colors - 1")
        if not 1 <= permille <= 1000 or over not in ("found", "valid") or min_kmers < 1:
            raise ValueError("a bad parameter")
        self.masks, self.k, self.C = class_masks(index, colors, k), k, n_colors
        self.rule = (permille, over, min_kmers)
        self.reset()

    def reset(self):
        self._classes = {}  # mask -> [fragments, first]
        self.totals = {"fragments": 0, "eligible": 0, "assigned": 0, "ambiguous": 0}

    def align(self, reads, mates=None):
        if mates is not None and len(mates) != len(reads):
            raise ValueError("reads and mates differ in number")
        out = {"kmers": [], "valid": [], "found": [], "hits": [], "masks": []}
        permille, over, min_kmers = self.rule
        for r, s in enumerate(reads):
            kmers, valid, found, hits = fragment(self.masks, self.k, [s] if mates is None else [s, mates[r]], self.C)
            mask = assign(valid, found, hits, permille, over, min_kmers)
            for f, v in zip(("kmers", "valid", "found", "hits", "masks"), (kmers, valid, found, hits, mask)):
                out[f].append(v)
            ordinal = self.totals["fragments"]
            self.totals["fragments"] += 1
            self.totals["eligible"] += (found if over == "found" else valid) >= min_kmers
            self.totals["assigned"] += mask != 0
            self.totals["ambiguous"] += bin(mask).count("1") > 1
            if mask:
                self._classes.setdefault(mask, [0, ordinal])[0] += 1
        return out

    def classes(self):
        order = sorted(self._classes, key=lambda m: self._classes[m][1])
        return {"mask": order, "carriers": [bin(m).count("1") for m in order], "fragments": [self._classes[m][0] for m in order],
                "first": [self._classes[m][1] for m in order]}

    def color_reads(self):
        assigned, unique = [0] * self.C, [0] * self.C
        for m, (n, _) in self._classes.items():
            for c in range(self.C):
                if (m >> c) & 1:
                    assigned[c] += n
                    unique[c] += n * (m == 1 << c)
        return assigned, unique


# ---- the worked example of DESIGN.md 33 ----
EXAMPLE_K = 4
EXAMPLE_INDEX = ["ACGTTGCATGG", "ACGTTGCCTGG", "TTTTTTT", "CATGGA"]
EXAMPLE_RECORD_COLORS = [0, 1, 2, 2]
# (reads, mates or None, kmers, valid, found, hits, mask at P = 1000 over found, mask at P = 500 over found)
EXAMPLE_ROWS = [
    ("ACGTTGC", None, 4, 4, 4, [4, 4, 0], 0b011, 0b011),
    ("TGCATGGA", None, 5, 5, 5, [4, 0, 3], 0, 0b101),
    ("GCATGNACGTT", None, 8, 4, 4, [4, 2, 1], 0b001, 0b011),
    ("CCAGGCAACGT", None, 8, 8, 8, [4, 8, 0], 0b010, 0b011),
    ("GGGGGGG", None, 4, 4, 0, [0, 0, 0], 0, 0),
    ("TGCATGG", "AAAAAC", 7, 7, 6, [4, 0, 4], 0, 0b101),
    ("ACG", None, 0, 0, 0, [0, 0, 0], 0, 0),
]


def example_colors():
    return masks_by_record(EXAMPLE_INDEX, EXAMPLE_RECORD_COLORS, EXAMPLE_K)


# ---- the command line's files ----
def out_lines(names, result):
    lines = ["record\tkmers\tvalid\tfound\tcolors"]
    for name, n, v, f, m in zip(names, result["kmers"], result["valid"], result["found"], result["masks"]):
        colors = ",".join(str(c) for c in range(64) if (m >> c) & 1) or "-"
        lines.append(f"{name}\t{n}\t{v}\t{f}\t{colors}")
    return lines


def class_lines(sample, classes):
    return [f"{sample}\t{i}\t{m:x}\t{c}\t{n}" for i, (m, c, n) in enumerate(zip(classes["mask"], classes["carriers"], classes["fragments"]))]
