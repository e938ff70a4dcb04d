"""Payloads by position on the sparse minimizer index (tig_payload_device.hpp) restated in plain Python on top of
tig_locate_ref.py. Not a test module.

A payload is one value per window of the indexed text, in window order. Payload(values, kind, n_colors, layout) keeps it as the device
does -- dense, or the maximal runs of equal consecutive values -- and at(ordinal) is the lookup; width, layout and device_bytes follow
the rules of the header. ordinal(off, k, t) turns the global start t of an index window into its place in window order. abundance()
and color_hits() are "the payload at TigLocateRef.where's position", shaped like kmer_abundance_ref.abundance / kmer_color_ref.color_hits,
which stay the arbiters: they know nothing about positions or layouts.

payload_pair(rng, k) is the generator the GPU test draws its random cases from, and seen_flags() says which of the hazards a case
shows; test_tig_payload_ref.py checks without a GPU that the generator shows all of them at every k the GPU test uses."""
import bisect

import tig_index_cases as cases
import tig_index_ref as T
import tig_locate_ref as TL
from matchtigs_amd import synth

RUN = 64  # query positions per thread of the gather (kw::RUN)
WEIGHT_BYTES, MASK_BYTES = 4, 8


def runs_of(values):
    """(start, value) of the maximal runs of equal consecutive values: start[0] == 0, ascending."""
    starts, vals = [], []
    for w, v in enumerate(values):
        if w == 0 or v != values[w - 1]:
            starts.append(w)
            vals.append(v)
    return starts, vals


def weight_width(values):
    """The narrowest of 1, 2, 4 bytes that holds the largest weight."""
    top = max(values, default=0)
    return 1 if top < 1 << 8 else 2 if top < 1 << 16 else 4


def mask_width(n_colors):
    """The narrowest of 1, 2, 4, 8 bytes that holds n_colors bits."""
    return 1 if n_colors <= 8 else 2 if n_colors <= 16 else 4 if n_colors <= 32 else 8


class Payload:
    def __init__(self, values, kind="weights", n_colors=None, layout=None):
        values = [int(v) for v in values]
        self.windows = len(values)
        self.value_bytes = WEIGHT_BYTES if kind == "weights" else MASK_BYTES
        self.width = weight_width(values) if kind == "weights" else mask_width(n_colors)
        assert all(v < 1 << (8 * self.width) for v in values)
        self.starts, self.vals = runs_of(values)
        self.runs = len(self.starts)
        self.runs_bytes = (8 + self.value_bytes) * self.runs
        self.dense_bytes = self.width * self.windows
        self.layout = layout or ("runs" if self.runs_bytes < self.dense_bytes else "dense")  # a tie is dense
        self.device_bytes = self.runs_bytes if self.layout == "runs" else self.dense_bytes
        self.dense = values if self.layout == "dense" else None

    def at(self, ordinal):
        assert 0 <= ordinal < self.windows
        if self.layout == "dense":
            return self.dense[ordinal]
        return self.vals[bisect.bisect_right(self.starts, ordinal) - 1]  # the largest i with start[i] <= ordinal

    def info(self):
        return {"layout": self.layout, "width": self.width, "windows": self.windows, "runs": self.runs, "device_bytes": self.device_bytes}


def window_offsets(off, k):
    """win_off[r] = the windows of the records before r."""
    out = [0]
    for r in range(len(off) - 1):
        out.append(out[-1] + max(0, off[r + 1] - off[r] - k + 1))
    return out


def ordinal(off, k, t, win_off=None):
    win_off = window_offsets(off, k) if win_off is None else win_off
    r = bisect.bisect_right(off, t) - 1
    while off[r + 1] == off[r]:  # (never: t starts a window, so its record is not empty)
        r -= 1
    assert off[r] <= t and t + k <= off[r + 1]
    return win_off[r] + (t - off[r])


def _walk(ref, query, each):
    """kmers / valid / found per query record; each(record, global position, where) per found window."""
    k = ref.k
    out = {"kmers": [], "valid": [], "found": []}
    base = 0
    for r, s in enumerate(query):
        n = max(0, len(s) - k + 1)
        v = f = 0
        for i in range(n):
            w = s[i:i + k]
            if all(c in T.ACGT for c in w):
                v += 1
                t = ref.where(w.upper())
                if t is not None:
                    f += 1
                    each(r, base + i, t)
        out["kmers"].append(n)
        out["valid"].append(v)
        out["found"].append(f)
        base += len(s)
    return out


def abundance(ref, payload, query):
    """kmer_abundance_ref.abundance's dictionary from the payload at where()'s position. ref: a TigLocateRef."""
    win_off = window_offsets(ref.off, ref.k)
    hits = [[] for _ in query]
    per_window = [0] * sum(len(s) for s in query)

    def each(r, p, t):
        w = payload.at(ordinal(ref.off, ref.k, t, win_off))
        hits[r].append(w)
        per_window[p] = w

    out = _walk(ref, query, each)
    out.update(sum=[sum(h) for h in hits], min=[min(h, default=0) for h in hits], max=[max(h, default=0) for h in hits], per_window=per_window)
    return out


def color_hits(ref, payload, n_colors, query):
    """kmer_color_ref.color_hits' dictionary from the payload at where()'s position."""
    win_off = window_offsets(ref.off, ref.k)
    per_color = [[0] * n_colors for _ in query]
    per_window = [0] * sum(len(s) for s in query)

    def each(r, p, t):
        m = payload.at(ordinal(ref.off, ref.k, t, win_off))
        per_window[p] = m
        for c in range(n_colors):
            per_color[r][c] += (m >> c) & 1

    out = _walk(ref, query, each)
    out.update(per_color=per_color, per_window=per_window)
    return out


def runny(rng, n, values, longest=6):
    """n values in runs of 1 .. longest equal ones, drawn from `values`."""
    out = []
    while len(out) < n:
        out += [rng.choice(values)] * rng.randint(1, longest)
    return out[:n]


def payload_pair(rng, k):
    """tig_index_cases.random_pair plus what the payloads need: a query record of more than 2 RUN positions that the index's own
    records fill (more than one thread folds it), one foreign record (nothing found), and per window of the index a weight and a mask
    in short runs -- the weights reach every width, the masks use n_colors bits with the top one set somewhere."""
    index, query = cases.random_pair(rng, k)
    index = index + [cases.dna(rng, k + rng.randint(2, 9))]  # (never without a window)
    own = "".join(index).upper()
    query = query + [(own * (2 * RUN // len(own) + 2))[:2 * RUN + k + 7], ""]
    windows = sum(max(0, len(s) - k + 1) for s in index)
    top = rng.choice([255, 256, 65535, 65536, (1 << 32) - 1])
    weights = runny(rng, windows, [0, 1, 2, 3, top, top - 1, rng.randint(0, top)])
    n_colors = rng.choice([1, 8, 9, 16, 17, 32, 33, 64])
    full = (1 << n_colors) - 1
    masks = runny(rng, windows, [0, 1, full, 1 << (n_colors - 1), rng.randint(0, full), rng.randint(0, full)])
    return index, query, weights, masks, n_colors


SEEN = ("first of a run", "last of a run", "inside a run", "repeat with another payload", "record without a hit", "record over two threads")


def seen_flags(index, weights, query, k):
    """Which hazards of SEEN the case shows, from dictionaries alone (no minimizers): the first window of every class, the runs of the
    weights, and the found windows of the query."""
    text, off = "".join(index).upper(), [0]
    for s in index:
        off.append(off[-1] + len(s))
    first, differing, o = {}, set(), 0
    for r in range(len(index)):
        for t in range(off[r], off[r + 1] - k + 1):
            x = synth.canonical(text[t:t + k])
            if x not in first:
                first[x] = o
            elif weights[first[x]] != weights[o]:
                differing.add(x)
            o += 1
    starts, _ = runs_of(weights)
    heads, tails = set(starts), {s - 1 for s in starts[1:]} | {len(weights) - 1}
    seen = dict.fromkeys(SEEN, False)
    base = 0
    for s in query:
        blocks, found = set(), 0
        for i in range(len(s) - k + 1):
            w = s[i:i + k]
            if not all(c in T.ACGT for c in w):
                continue
            x = synth.canonical(w.upper())
            if x not in first:
                continue
            found += 1
            blocks.add((base + i) // RUN)
            o = first[x]
            seen["first of a run"] |= o in heads
            seen["last of a run"] |= o in tails
            seen["inside a run"] |= o not in heads and o not in tails
            seen["repeat with another payload"] |= x in differing
        seen["record without a hit"] |= found == 0
        seen["record over two threads"] |= len(blocks) > 1
        base += len(s)
    return seen


def palindrome_weights(ref, text, hard):
    """One weight per window of the palindrome text, all distinct (so the two occurrences of a class differ), and for every hard window
    x the pair (payload at the first passing candidate, payload at the minimum)."""
    k = ref.k
    weights = [1000 + i for i in range(len(text) - k + 1)]
    pairs = []
    for x in hard:
        c = ref.candidates(x)
        pairs.append((weights[c[0]], weights[min(c)]))
    return weights, pairs
