"""collision_cases.py -- inputs whose k-mers collide in all 64 bits of the window hash of kmer_window_device.hpp's wide path (k >= 32),
and a model of that hash family. Plain Python; not a test module.

The window hash is a pair of polynomial hashes mod 2^64 with an odd base B (one per strand). For the Thue-Morse word X of order n over
two letters (a, b) and Y = X with a and b swapped,
    hash(X) - hash(Y) = +-(a - b) * prod_{j < n} (B^(2^j) - 1).
For odd B, B^2 - 1 is divisible by 8 and B^(2^j) - 1 by 2^(j + 2) for j >= 1 (each squaring adds a factor B^(2^(j-1)) + 1, which is
even), so at n = 10 the product is divisible by 2^(1 + 3 + 4 + ... + 11) = 2^64: zero. A reversed Thue-Morse word of even order is the
word itself, so the reverse strand's hash collides as well. A common prefix and suffix multiply the difference by a power of B and
keep it zero: in records P + X + S and P + Y + S every window that contains the whole block collides with its counterpart, whatever B
is. Order 9 guarantees only 2^(1 + 3 + ... + 10) = 2^53 and reaches 2^64 for special bases alone (B near +-1 modulo a high power of two;
valuation() says exactly when): 1024 bases is the shortest block that collides for every odd base.

With the letter pairs A/T and C/G, Y is the reverse complement of X -- the same class, and useless. A/G and A/C give two classes."""
import random

from matchtigs_amd.synth import canonical, revcomp

MASK = (1 << 64) - 1
ORDER = 10
BLOCK = 1 << ORDER
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
KS = (1024, 1025, 1031, 1056)  # not multiples of 16, and one that is: same_class compares 16 bases at a time
K_NODES = BLOCK + 1            # the block as a (k-1)-mer: a node of the compaction, an end of the join


def thue_morse(order, a, b):
    """The Thue-Morse word of length 2^order over the letters a (for 0) and b (for 1): letter i is b iff i has an odd number of one bits."""
    return "".join(b if bin(i).count("1") & 1 else a for i in range(1 << order))


X = thue_morse(ORDER, "A", "G")
Y = thue_morse(ORDER, "G", "A")
assert len(X) == BLOCK and X != Y and canonical(X) != canonical(Y), "the two blocks must be two k-mer classes"


def strand_hashes(s, base):
    """(hf, hr) of the string s as the wide path defines them, for any odd base B: hf = sum (c_i + 1) B^(k-1-i), hr = sum (4 - c_i) B^i,
    codes A, C, G, T = 0 .. 3, mod 2^64. hr(s) = hf(revcomp(s))."""
    hf = hr = 0
    pw = 1
    for ch in s.upper():
        c = CODE[ch]
        hf = (hf * base + c + 1) & MASK
        hr = (hr + (4 - c) * pw) & MASK
        pw = (pw * base) & MASK
    return hf, hr


def window_hashes(s, k, base):
    """strand_hashes of every window of length k of s, in position order, from prefix and suffix sums (no modular inverse)."""
    s = s.upper()
    n = len(s)
    if n < k:
        return []
    pre = [0] * (n + 1)  # pre[i] = hf(s[:i])
    for i, ch in enumerate(s):
        pre[i + 1] = (pre[i] * base + CODE[ch] + 1) & MASK
    suf = [0] * (n + 1)  # suf[i] = hr(s[i:])
    for i in range(n - 1, -1, -1):
        suf[i] = (4 - CODE[s[i]] + base * suf[i + 1]) & MASK
    bk = pow(base, k, 1 << 64)
    return [((pre[i + k] - pre[i] * bk) & MASK, (suf[i] - bk * suf[i + k]) & MASK) for i in range(n - k + 1)]


def class_hash_key(h):
    """What a hash of the CLASS {x, rc(x)} can depend on: the unordered pair {hf, hr} (rc swaps the two)."""
    return (min(h), max(h))


def _v2(x):
    x &= MASK
    return 64 if x == 0 else (x & -x).bit_length() - 1


def valuation(order, a, b, base):
    """The power of two (capped at 64) that divides hf(T) - hf(T'), T the Thue-Morse word of that order over (a, b) and T' over (b, a):
    that of (a - b) * prod_{j < order} (B^(2^j) - 1). The words collide iff it is 64."""
    v = _v2(CODE[a] - CODE[b])
    for j in range(order):
        v += _v2(pow(base, 1 << j, 1 << 64) - 1)
    return min(v, 64)


def _dna(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def cases(seed=20261):
    """name -> records. F, L, R: 40 random bases; D1 .. D5: 30.
    pair        [L+X+R, L+Y+R]: every window that holds the block collides with the window at the same place of the other record;
    strand      [L+X+R, revcomp(L+Y+R)]: the same, resolved through the reverse-complement half of same_class;
    one_record  [F+X+F+Y+F]: the colliding windows lie 1064 positions apart in one record of one store;
    nodes       [C+X+T, T+Y+C] at k = 1025: the (k-1)-mer nodes X and Y collide; merged, they would turn 2 unitigs into 4 (the
                k-mers C+X and Y+C collide as well: X and Y both hash like 1024 times C, the mean of A and G);
    join        [D1+X, X+D2, Y+D3, D4+Y, revcomp(X+D5)] at k = 1025: the ends X and Y of the plain-FASTA join collide."""
    rng = random.Random(seed)
    F, L, R = (_dna(rng, 40) for _ in range(3))
    D = [_dna(rng, 30) for _ in range(5)]
    return {
        "pair": [L + X + R, L + Y + R],
        "strand": [L + X + R, revcomp(L + Y + R)],
        "one_record": [F + X + F + Y + F],
        "nodes": ["C" + X + "T", "T" + Y + "C"],
        "join": [D[0] + X, X + D[1], Y + D[2], D[3] + Y, revcomp(X + D[4])],
    }


def case_ks(name):
    return (K_NODES,) if name in ("nodes", "join") else KS


def index_inputs(k):
    """The two k-mer index cases on `pair` = [x, y], W windows per record; each -> index, weights, masks (2 colours), query.
    lookup  an index of x alone asked for y on both strands and for x: the probe of a query window of y meets the slot of its
            counterpart of x -- same home slot, same tag -- and compares the QUERY's bases with the INDEX's;
    claim   an index of x and y: two classes per probe sequence while the table is built, each with a weight and a mask of its own."""
    x, y = cases()["pair"]
    W = len(x) - k + 1
    return {
        "lookup": {"index": [x], "weights": [3 + i for i in range(W)], "masks": [1 + i % 3 for i in range(W)], "n_colors": 2,
                   "query": [y, revcomp(y), x]},
        "claim": {"index": [x, y], "weights": [10 + i for i in range(W)] + [1000 + i for i in range(W)], "masks": [1] * W + [2] * W,
                  "n_colors": 2, "query": [x, y, revcomp(y), revcomp(x)]},
    }


def window_classes(records, k):
    """The k-mer classes of the windows of the records, as canonical strings."""
    return {canonical(r[i:i + k].upper()) for r in records for i in range(len(r) - k + 1)}


def colliding_pairs(k):
    """Windows of L+X+R (40 + 1024 + 40 bases) that hold the whole block: starts max(0, 1064 - k) .. 40."""
    return 40 - max(0, 40 + BLOCK - k) + 1
