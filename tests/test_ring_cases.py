"""The ring cases (ring_cases.py) on the CPU: the generator against compact_ref.compact, abundance_ref.compact_counted and
color_split_ref.compact_classes. Every ring is one closed walk; the counts C of listed elements and n_or of oriented k-mers are the
ones the names ODD and EVEN promise, with log2_ceil(C) odd and even -- both branches of the minima's ping-pong in
compact_device.hip --; the coloured worlds keep, open and filter the rings they say they do; and the closed forms that
test_gpu_ring_walks.py uses where a restatement would take too long (ring_with_arc, "a disjoint ring comes out as itself") equal
the restatement's output at sizes it can still take. The expectations the GPU tests share are computed here, once per process."""
import functools

import numpy as np
import pytest

import abundance_ref as A
import color_split_ref as S
import compact_ref as R
import ring_cases as RC
from matchtigs_amd.synth import canonical, revcomp

KS = (31, 32, 33, 64)
COLOUR_KS = (31, 32, 33)
WORLDS = {"odd": RC.ODD, "even": RC.EVEN}
SEED = 2027


# ---- the inputs and expectations the GPU tests share ----
@functools.lru_cache(maxsize=None)
def world(name, k, colours=False):
    """-> (records, colours, rings); name: odd, even, 2048, 2049 (a ring alone) or small (the unit rings alone)."""
    if name == "small":
        return RC.small_world(k), [0] * len(RC.SMALL_UNITS), list(RC.SMALL_UNITS)
    if name in WORLDS:
        return RC.ring_world(k, WORLDS[name], SEED + k, colours)
    return RC.ring_world(k, [int(name)], SEED + k, colours, chains=False)


@functools.lru_cache(maxsize=None)
def compacted(name, k):
    """-> (unitigs, statistics, closed flags, C, n_or) of compact_ref.compact."""
    out = R.compact(world(name, k)[0], k)
    return out + RC.listed(k, *out)


@functools.lru_cache(maxsize=None)
def classed(name, k, m, split):
    """color_split_ref.compact_classes of the coloured world -> (unitigs, statistics, closed, abundance, colours, classes)."""
    recs, colors, _ = world(name, k, True)
    return S.compact_classes(recs, colors, 3, k, m, split)


PLAIN = [(n, k) for k in KS for n in ("odd", "even")] + [("2048", 31), ("2049", 31)] + [("small", k) for k in RC.SMALL_KS]
# name, k -> closed walks, C, log2_ceil(C)
WANT = {**{("odd", k): (18, 17110, 15) for k in KS}, **{("even", k): (17, 8916, 14) for k in KS}, ("2048", 31): (1, 4096, 12),
        ("2049", 31): (1, 4098, 13), **{("small", k): (5, 24, 5) for k in (5, 6, 7, 8)}, ("small", 4): (3, 8, 3)}


def test_log2_ceil():
    assert [RC.log2_ceil(n) for n in (0, 1, 2, 3, 4, 5, 8, 9, 4096, 4097, 4098, 8916, 17110, 1 << 21, (1 << 21) + 1)] == [
        0, 0, 1, 2, 2, 3, 3, 4, 12, 13, 13, 14, 15, 21, 22]
    assert RC.round_limits(17110, 21808) == (17, 17 + 15 + 17) and RC.round_limits(2, 2) == (3, 3 + 1 + 3)


def test_ring_record():
    c = "AACCG"
    assert RC.ring_record(c, 3) == "AACCGAA" and RC.ring_record(c, 3, rot=2) == "CCGAACC" and RC.ring_record(c, 3, rot=7) == "CCGAACC"
    assert RC.ring_record(c, 3, rot=4, n=2) == "GAAC" and RC.ring_record(c, 3, rc=True) == revcomp("AACCGAA")
    assert RC.ring_record("AC", 7) == "ACACACAC" and RC.ring_record("A", 31, rot=5) == "A" * 31 and len(RC.ring_record(c, 64, 3)) == 68
    for k in (4, 31, 64):  # the windows of any reading are the ring's, on either strand
        whole = {canonical(w) for w in (RC.ring_record(c, k)[i:i + k] for i in range(5))}
        assert len(whole) == 5
        for rot in range(6):
            for rc in (False, True):
                r = RC.ring_record(c, k, rot, rc)
                assert len(r) == 5 + k - 1 and {canonical(r[i:i + k]) for i in range(5)} == whole
                arc = RC.ring_record(c, k, rot, rc, n=2)
                assert len(arc) == k + 1 and {canonical(arc[i:i + k]) for i in range(2)} < whole


@pytest.mark.parametrize("name,k", PLAIN)
def test_every_ring_is_a_closed_walk_and_the_counts_are_the_promised_ones(name, k):
    recs, _, rings = world(name, k)
    unitigs, stats, closed, C, n_or = compacted(name, k)
    walks, want_C, rounds = WANT[name, k]
    assert (stats["closed_walks"], C, RC.log2_ceil(C)) == (walks, want_C, rounds) and n_or == 2 * stats["distinct_kmers"] >= C
    if name in WORLDS:  # the chains between the rings are unitigs of their own
        assert stats["unitigs"] > stats["closed_walks"] and n_or > C
        assert sorted(len(u) - k + 1 for u, c in zip(unitigs, closed) if c) == WORLDS[name]
        assert [len(c) for c in rings] == WORLDS[name] and stats["longest_unitig_kmers"] == max(WORLDS[name])
        # the ids do not follow the walk: a ring written as its reverse complement is emitted on that strand
        assert sum(u != RC.ring_record(c, k, 7 * i) for i, (u, c) in enumerate(zip([u for u, c in zip(unitigs, closed) if c], rings))) >= 8
    elif name != "small":
        assert n_or == C and unitigs == recs
    elif k > 4:
        assert n_or == C and unitigs == recs and all(closed)
    else:
        assert [u for u, c in zip(unitigs, closed) if c] == [recs[0], recs[1], recs[4]] == ["AAAA", "GTGTG", "CCCC"] and stats["unitigs"] == 5


def test_both_parities_of_the_ping_pong_are_there():
    """What the GPU module relies on: the worlds differ in the parity of log2_ceil(C), and a ring alone gives C = 2^m exactly."""
    for k in KS:
        assert RC.log2_ceil(compacted("odd", k)[3]) % 2 == 1 and RC.log2_ceil(compacted("even", k)[3]) % 2 == 0
    assert compacted("2048", 31)[3] == 1 << 12 and RC.log2_ceil(compacted("2049", 31)[3]) % 2 == 1
    assert {RC.log2_ceil(compacted("small", k)[3]) % 2 for k in RC.SMALL_KS} == {1}
    # the coloured worlds, split: the other parity of each
    for k in COLOUR_KS:
        odd, even = classed("odd", k, 1, True), classed("even", k, 1, True)
        assert RC.log2_ceil(RC.listed(k, *odd[:3])[0]) == 14 and RC.log2_ceil(RC.listed(k, *even[:3])[0]) == 13


@pytest.mark.parametrize("name", ["odd", "even"])
@pytest.mark.parametrize("k", COLOUR_KS)
def test_the_coloured_worlds_keep_open_and_filter_what_they_say(name, k):
    n = len(WORLDS[name])
    arcs = [i for i, L in enumerate(WORLDS[name]) if i % 3 == 1 and L > 8]
    twice = [i for i in range(n) if i % 3 == 0]
    assert (len(arcs), len(twice)) == (5, 6)
    recs, colors, rings = world(name, k, True)
    assert len(recs) == 2 * n + 11 and sorted(set(colors)) == [0, 1, 2] and colors.count(2) == 11
    plain = compacted(name, k)
    for split in (False, True):
        unitigs, stats, closed, ab, col, classes = classed(name, k, 1, split)
        assert stats["closed_walks"] == (n - 5 if split else n) and stats["distinct_kmers"] == plain[1]["distinct_kmers"]
        assert ab["max_abundance"] == 2 and ab["spectrum"][2] == sum(WORLDS[name][i] for i in twice) + sum(WORLDS[name][i] // 2 for i in arcs)
        assert classes["masks"][:3] == [5, 2, 1] and sorted(classes["masks"]) == [1, 2, 5]  # ring 0 is A: in colours 0 and 2
        if not split:
            assert unitigs == plain[0] and 2 * 1024 in ab["unitig_sums"]
        else:  # an opened ring: its arc and the rest, two chains
            assert stats["unitigs"] == plain[1]["unitigs"] + 5 and classes["n_runs"] == stats["unitigs"]
        counted = A.compact_counted(recs, k, 1)
        assert counted[0] == plain[0] and counted[3]["distinct_all"] == ab["distinct_all"]
        # m = 2: the six rings given twice, closed, and the five arcs, open; nothing else
        unitigs, stats, closed, ab, col, classes = classed(name, k, 2, split)
        assert (stats["closed_walks"], stats["unitigs"]) == (6, 11) and set(col["kmer_colors"]) == {5} and set(ab["kmer_counts"]) == {2}
        assert sorted(len(u) - k + 1 for u, c in zip(unitigs, closed) if c) == [WORLDS[name][i] for i in twice]
        assert sorted(len(u) - k + 1 for u, c in zip(unitigs, closed) if not c) == [WORLDS[name][i] // 2 for i in arcs]
        assert (unitigs, stats, closed) == A.compact_counted(recs, k, 2)[:3]


@pytest.mark.parametrize("k", [31, 32])
@pytest.mark.parametrize("L", [40, 64, 257, 5000, 60_000])
def test_ring_with_arc_in_closed_form(L, k):
    c = RC.dna(np.random.default_rng(L + k), L)
    for arc_rot, arc_n, ring_rot in ((L // 4, L // 5, (2 * L) // 3), (L - 3, 7, 0)) if L <= 5000 else ((L // 4, L // 5, (2 * L) // 3),):
        recs, unitig = RC.ring_with_arc(c, k, arc_rot, arc_n, ring_rot)
        assert len(recs[0]) == arc_n + k - 1 and len(recs[1]) == len(unitig) == L + k - 1
        unitigs, stats, closed = R.compact(recs, k)
        assert unitigs == [unitig] and closed == [True] and stats["distinct_kmers"] == L
        # the emitted strand is record0's, the reverse of the one the ring was written on
        assert unitig.startswith(recs[0]) and canonical(unitig[:k]) == canonical(recs[1][(arc_rot + arc_n - 1 - ring_rot) % L:][:k])
        assert unitig[:k] in (revcomp(c) * (2 + k // L)) and (L < 2 * k or unitig[:k] not in c * 2)


def test_a_record_that_is_one_whole_disjoint_ring_comes_out_as_itself():
    for k in (31, 32):
        rings = RC.plasmids(300, 17 + k)
        assert min(map(len, rings)) < k and max(map(len, rings)) > 350
        recs = [RC.ring_record(c, k) for c in rings]
        unitigs, stats, closed = R.compact(recs, k)
        assert unitigs == recs and stats["closed_walks"] == len(recs) == 300 and all(closed)
        # ... and with an arc in front, as its closed form
        both = [RC.ring_with_arc(c, k, len(c) // 2, len(c) // 3, 0) for c in rings]
        unitigs, stats, closed = R.compact([r for pair, _ in both for r in pair], k)
        assert unitigs == [u for _, u in both] and stats["closed_walks"] == 300 and stats["records"] == 600
