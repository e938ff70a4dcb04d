"""`locate` on the sparse minimizer index (tig_index_device.hip) restated in plain Python on top of tig_index_ref.py.

TigLocateRef.where(x) is the lookup rule with positions. Light bucket: the candidates of the bucket's entries, in entry order, that pass
the record bound and the compare of k characters are all the occurrences of x's class, and the answer is their MINIMUM. Heavy bucket:
the smallest start among the windows that went to the table. locate() is kmer_locate_ref.locate's folding of hits into runs with that
lookup; the arbiter stays kmer_locate_ref.locate, which knows nothing about how an index is organised.

first_is_not_minimum(x) says whether the first passing candidate differs from the minimum: entries ascend by anchor, but the two
candidates of an anchor use different offsets, so an occurrence on the other strand can lie earlier in the text while its anchor lies
later. palindrome_text() builds the inputs on which that happens."""
import bisect

import tig_index_ref as T
from matchtigs_amd import synth


class TigLocateRef(T.TigIndexRef):
    def __init__(self, seqs, k, m=None, bucket_limit=64):
        super().__init__(seqs, k, m, bucket_limit)
        self.heavy_where = {}  # canonical k-mer -> the smallest start of a window of its class, for the windows of the heavy buckets
        if self.heavy:
            for r in range(len(self.off) - 1):
                for q in range(self.off[r], self.off[r + 1] - k + 1):  # ascending: the first one seen is the smallest
                    x = self.text[q:q + k]
                    if self.bucket(T.minimizer(x, self.m)[0]) in self.heavy:
                        self.heavy_where.setdefault(synth.canonical(x), q)

    def candidates(self, x):
        """The starts of the index windows of x's class, in the order the light lookup meets them; None: x takes the heavy path."""
        k, w = self.k, self.w
        v, j1, jl = T.minimizer(x, self.m)
        b = self.bucket(v)
        if b in self.heavy:
            return None
        out = []
        for key, p in self.entries.get(b, ()):
            if key != v:
                continue
            lo, hi = self.record_bounds(p)
            offsets = (j1, w - 1 - jl) if j1 != w - 1 - jl else (j1,)  # x forward in the text; rc(x) forward in the text
            for q in (p - j for j in offsets):
                if q >= lo and q + k <= hi and self.text[q:q + k] in (x, synth.revcomp(x)):
                    out.append(q)
        return out

    def where(self, x):
        """x: k characters of ACGT, upper case, as the query shows them. The smallest start of an index window of its class, or None."""
        c = self.candidates(x)
        if c is None:
            return self.heavy_where.get(synth.canonical(x))
        return min(c) if c else None

    def takes_heavy_path(self, x):
        return self.candidates(x) is None

    def first_is_not_minimum(self, x):
        c = self.candidates(x)
        return bool(c) and c[0] != min(c)


def locate(index, query_seqs):
    """kmer_locate_ref.locate's result with TigLocateRef.where as the lookup."""
    k, text, t_off = index.k, index.text, index.off

    def record_of(t):
        return bisect.bisect_right(t_off, t) - 1

    kmers, valid, found, runs = [], [], [], []
    for qr, s in enumerate(query_seqs):
        n = max(0, len(s) - k + 1)
        v = f = 0
        prev = None
        for i in range(n):
            w = s[i:i + k]
            hit = None
            if all(c in T.ACGT for c in w):
                v += 1
                t = index.where(w.upper())
                if t is not None:
                    f += 1
                    hit = (t, 0 if w.upper() == text[t:t + k] else 1)
            if hit is not None:
                t, strand = hit
                if (prev is not None and prev[1] == strand and t == (prev[0] - 1 if strand else prev[0] + 1)
                        and record_of(t) == record_of(prev[0])):
                    runs[-1][2] += 1
                    if strand:
                        runs[-1][5] -= 1
                else:
                    tr = record_of(t)
                    runs.append([qr, i, 1, strand, tr, t - t_off[tr]])
            prev = hit
        kmers.append(n)
        valid.append(v)
        found.append(f)
    return {"kmers": kmers, "valid": valid, "found": found, "runs": [tuple(r) for r in runs]}


def palindrome_text(rng, k, m):
    """A reverse-complement palindrome h + rc(h) of even length k + d, 1 <= d <= k - m, between random flanks: every window inside the
    palindrome has its reverse complement mirrored inside it too."""
    ds = [d for d in range(1, k - m + 1) if (k + d) % 2 == 0]
    h = "".join(rng.choices("ACGT", k=(k + rng.choice(ds)) // 2))
    flank = lambda: "".join(rng.choices("ACGT", k=rng.randint(k, 2 * k)))
    return flank() + h + synth.revcomp(h) + flank()


def palindrome_case(rng, k, m, limit=64, tries=400):
    """(text, [windows x of text or of rc(text) with first_is_not_minimum(x)]) for the first text of `tries` that has such a window."""
    for _ in range(tries):
        text = palindrome_text(rng, k, m)
        ix = TigLocateRef([text], k, m, limit)
        hard = [s[i:i + k] for s in (text, synth.revcomp(text)) for i in range(len(s) - k + 1) if ix.first_is_not_minimum(s[i:i + k])]
        if hard:
            return text, hard
    raise AssertionError(f"no palindrome text at k={k} m={m} whose first passing candidate is not the minimum")
