"""The sparse minimizer index (tig_index_device.hip) restated in plain Python: strings, a dict of lists, a set.

The m-mer at a text position has the key mix64(canonical 2-bit code); the minimizer of a window is the class with the smallest key
among its w = k - m + 1 m-mers, its anchor the global position of the leftmost m-mer of that class. TigIndexRef keeps the
concatenated text, the record offsets, the anchors grouped by the top bits of their key, and -- for the buckets with more than
bucket_limit anchors -- the set of canonical k-mers whose minimizer falls into one. contains() is the lookup rule: the two candidate
starts per anchor of the class, kept only inside one record, decided by a compare of k characters. query() is
kmer_query_ref.query with that lookup, the window passed in the orientation the query shows it."""
import numpy as np

from matchtigs_amd import synth

ACGT = frozenset("ACGTacgt")
M64 = (1 << 64) - 1
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def mix64(z):
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
    return z ^ (z >> 31)


def mmer_key(s):
    """The key of the class of the m-mer s (upper case): mix64 of the canonical code, first base in the highest bits."""
    c = synth.canonical(s)
    v = 0
    for ch in c:
        v = (v << 2) | CODE[ch]
    return mix64(v)


def default_m(k):
    return min(19, -(-2 * k // 3))


def minimizer(x, m):
    """(key, offset of the leftmost m-mer of the minimizer's class in x, offset of the rightmost)."""
    keys = [mmer_key(x[j:j + m]) for j in range(len(x) - m + 1)]
    v = min(keys)
    return v, keys.index(v), len(keys) - 1 - keys[::-1].index(v)


class TigIndexRef:
    def __init__(self, seqs, k, m=None, bucket_limit=64):
        assert all(c in ACGT for s in seqs for c in s), "the index holds ACGT only"
        self.k, self.m = k, default_m(k) if m is None else m
        assert 1 <= self.m <= min(k, 31)
        self.w = k - self.m + 1
        self.text = "".join(seqs).upper()
        self.off = [0]
        for s in seqs:
            self.off.append(self.off[-1] + len(s))
        windows = []  # (global start, key of the minimizer, anchor)
        for r in range(len(seqs)):
            lo, hi = self.off[r], self.off[r + 1]
            keys = [mmer_key(self.text[p:p + self.m]) for p in range(lo, hi - self.m + 1)]  # (what minimizer() would compute per window)
            for q in range(lo, hi - k + 1):
                ks = keys[q - lo:q - lo + self.w]
                v = min(ks)
                windows.append((q, v, q + ks.index(v)))
        self.occurrences = len(windows)
        marked = sorted({(p, v) for _, v, p in windows})
        self.bits = 3
        while (1 << self.bits) < len(marked):
            self.bits += 1
        self.buckets = 1 << self.bits
        per_bucket = {}
        for p, v in marked:
            per_bucket.setdefault(self.bucket(v), []).append((v, p))
        self.heavy = {b for b, e in per_bucket.items() if len(e) > bucket_limit}
        self.entries = {b: e for b, e in per_bucket.items() if b not in self.heavy}  # (ascending by position)
        self.anchors = sum(map(len, self.entries.values()))
        heavy_windows = [q for q, v, _ in windows if self.bucket(v) in self.heavy]
        self.heavy_windows = len(heavy_windows)
        self.table = {synth.canonical(self.text[q:q + k]) for q in heavy_windows}

    def bucket(self, key):
        return key >> (64 - self.bits)

    def record_bounds(self, p):
        r = max(i for i in range(len(self.off) - 1) if self.off[i] <= p)
        return self.off[r], self.off[r + 1]

    def contains(self, x):
        """x: k characters of ACGT, upper case, in the orientation the query shows them."""
        k, w = self.k, self.w
        v, j1, jl = minimizer(x, self.m)
        b = self.bucket(v)
        if b in self.heavy:
            return synth.canonical(x) in self.table
        for key, p in self.entries.get(b, ()):
            if key != v:
                continue
            lo, hi = self.record_bounds(p)
            for q in (p - j1, p - (w - 1 - jl)):  # x forward in the text; rc(x) forward in the text
                if q >= lo and q + k <= hi and self.text[q:q + k] in (x, synth.revcomp(x)):
                    return True
        return False


def query(index, seqs, k):
    """kmer_query_ref.query with TigIndexRef.contains as the lookup."""
    total = sum(len(s) for s in seqs)
    kmers, valid, found = [], [], []
    valid_bits, present_bits = [0] * ((total + 63) // 64), [0] * ((total + 63) // 64)
    base = 0
    for s in seqs:
        n = max(0, len(s) - k + 1)
        v = f = 0
        for i in range(n):
            x = s[i:i + k]
            if not all(c in ACGT for c in x):
                continue
            p = base + i
            v += 1
            valid_bits[p >> 6] |= 1 << (p & 63)
            if index.contains(x.upper()):
                f += 1
                present_bits[p >> 6] |= 1 << (p & 63)
        kmers.append(n)
        valid.append(v)
        found.append(f)
        base += len(s)
    return {"kmers": kmers, "valid": valid, "found": found, "valid_bits": valid_bits, "present_bits": present_bits}


def anchor_count_arrays(seq, off, k, m):
    """The distinct anchors of ASCII sequences (uint8 `seq` of ACGT, offsets `off`) by numpy, for inputs too large for the strings:
    the keys of all m-mers, the leftmost minimum of every window inside one record, the distinct positions."""
    lut = np.zeros(256, np.uint8)
    for i, c in enumerate(b"ACGT"):
        lut[c] = lut[c + 32] = i
    fwd, rc = synth._kmer_codes(lut[seq], m)
    z = np.minimum(fwd, rc)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    keys = z ^ (z >> np.uint64(31))
    w = k - m + 1
    first = np.lib.stride_tricks.sliding_window_view(keys, w).argmin(axis=1)  # (the first of equal minima: the leftmost)
    o = off.astype(np.int64)
    starts = np.concatenate([np.arange(o[r], max(o[r], o[r + 1] - k + 1)) for r in range(len(o) - 1)] or [np.zeros(0, np.int64)])
    return len(np.unique(starts + first[starts]))
