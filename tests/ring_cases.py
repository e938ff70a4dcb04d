"""ring_cases.py -- circular sequences for the compaction's closed-walk path (compact_device.hip: cycle_list, cycle_min_init, the
ping-pong cycle_min rounds, cycle_cut, the second pointer jumping; DESIGN.md 16 under rank), with answers in closed form. Plain
Python and numpy; not a test module.

A ring of L bases, primitive and sharing no (k-1)-mer with anything else, is one closed walk of L k-mers for every k (a record
that reads it wraps around as often as k needs). The device lists both orientations of every such k-mer: C = 2 * (the k-mers on
closed walks) elements out of n_or = 2 * (distinct k-mers). It then finds every cycle's minimum in log2_ceil(C) doubling rounds
that swap two buffers, so cycle_cut reads its minima from one buffer when that count is odd and from the other when it is even.
ODD and EVEN are one world with and without its longest ring: C = 17 110 (15 rounds) and C = 8 916 (14 rounds). Their lengths lie
around the wave (64), the workgroup and the powers of two up to 4097, the rings are written at rotations and on strands of their
own, and open chains lie between them: cycles of very different lengths interleave in the list, windows of 2^14 wrap hundreds of
times around a cycle of 2, and in most rings the smallest id is not the element listed first.
test_ring_cases.py holds all of it to the restatements on the CPU; test_gpu_ring_walks.py runs it on the device."""
import numpy as np

from matchtigs_amd.synth import revcomp

ODD = [1, 2, 3, 5, 31, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4097]
EVEN = ODD[:-1]
SINGLE = [[2048], [2049]]                             # alone: C = n_or = 4096 = 2^12, and 4098 (13 rounds)
UNITS = {1: "A", 2: "AC", 3: "AAG", 5: "AACCG"}       # primitive, and no two share a 4-mer on either strand
SMALL_UNITS = ["A", "AC", "AAG", "AACCG", "C"]
SMALL_KS = (4, 5, 6, 7, 8)
_ABC = np.frombuffer(b"ACGT", np.uint8)


def log2_ceil(n):
    """The smallest r with 2^r >= n (0 for n <= 1): the library's round counts are written in it."""
    r = 0
    while (1 << r) < n:
        r += 1
    return r


def dna(rng, n):
    """n random bases from a numpy Generator."""
    return _ABC[rng.integers(0, 4, n)].tobytes().decode()


def ring_record(c, k, rot=0, rc=False, n=None):
    """The record of n + k - 1 bases (n windows; default: all len(c)) that reads the circular string c from offset rot, wrapping as
    often as needed; rc: its reverse complement."""
    L = len(c)
    n = L if n is None else n
    rot %= L
    s = (c * ((rot + n + k - 1) // L + 1))[rot:rot + n + k - 1]
    return revcomp(s) if rc else s


def ring_world(k, lens, seed, colours=False, chains=True):
    """-> (records, record colours, rings). Ring i has lens[i] bases (UNITS where there is one, else random), is written from
    rotation 7 i on, every second one as its reverse complement, and is followed by a random linear record of 50 + 13 i bases
    (chains=False: rings only). colours=False: every record has colour 0. colours=True, three colours: rings 0, chains 1, and in
    colour 2, behind the ring's chain,
      i % 3 == 0            the whole ring again, on the other strand and from another rotation: abundance 2, one mask, still closed;
      i % 3 == 1, L > 8     an arc of L // 2 windows on the other strand: two masks on the ring (a split opens it), and
                            min_abundance = 2 keeps the arc alone."""
    rng = np.random.default_rng(seed)
    records, colors, rings = [], [], []
    for i, L in enumerate(lens):
        c = UNITS.get(L) or dna(rng, L)
        rings.append(c)
        rot, rc = 7 * i % L, bool(i % 2)
        records.append(ring_record(c, k, rot, rc))
        colors.append(0)
        if chains:
            records.append(dna(rng, 50 + 13 * i))
            colors.append(1 if colours else 0)
        if colours and i % 3 == 0:
            records.append(ring_record(c, k, rot + L // 2 + 1, not rc))
            colors.append(2)
        if colours and i % 3 == 1 and L > 8:
            records.append(ring_record(c, k, rot + 3, not rc, n=L // 2))
            colors.append(2)
    return records, colors, rings


def small_world(k):
    """The five unit rings alone, for k too small for random sequence: 5 closed walks for k = 5 .. 8; at k = 4 AAG and AACCG share
    the node GAA and open each other, which leaves 3."""
    return [ring_record(c, k, i, bool(i % 2)) for i, c in enumerate(SMALL_UNITS)]


def listed(k, unitigs, stats, closed):
    """(C, n_or) of a compaction from the restatement's result: the elements the device lists as lying on closed walks -- both
    orientations of their k-mers -- and all oriented k-mers."""
    return 2 * sum(len(u) - k + 1 for u, c in zip(unitigs, closed) if c), 2 * stats["distinct_kmers"]


def round_limits(C, n_or):
    """(lo, hi): a call that took the cycle path reports lo < rounds <= hi. The first pointer jumping gives up after
    log2_ceil(n_or) + 2 rounds; the minima take log2_ceil(C) more, the second pointer jumping at most log2_ceil(C) + 2."""
    lo = log2_ceil(n_or) + 2
    return lo, lo + log2_ceil(C) + log2_ceil(C) + 2


def ring_with_arc(c, k, arc_rot, arc_n, ring_rot):
    """-> ([record0, record1], the one unitig). record0: the reverse complement of the arc of arc_n windows of the ring c from
    arc_rot on; record1: the whole ring from ring_rot on. The leader is window 0 of record0 as read, so the unitig is the ring on
    record0's strand from that window on -- the reverse strand of record1, against which the ids of record1 run; the ids jump from
    the arc's end to wherever record1 begins."""
    L = len(c)
    record0 = ring_record(c, k, arc_rot, True, arc_n)
    record1 = ring_record(c, k, ring_rot)
    # window p of c, reverse-complemented, is window L - p - k of revcomp(c); record0 begins with the arc's last window
    unitig = ring_record(revcomp(c), k, (-(arc_rot + arc_n - 1) - k) % L)
    assert unitig[:k] == record0[:k]
    return [record0, record1], unitig


def plasmids(n, seed, lo=20, hi=400):
    """n random rings (circular strings) of lengths drawn from lo .. hi; ring_record(c, k) is the record that reads one once around."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, n)
    bases = _ABC[rng.integers(0, 4, int(lens.sum()))].tobytes().decode()
    at = np.concatenate([[0], np.cumsum(lens)])
    return [bases[int(at[i]):int(at[i + 1])] for i in range(n)]
