"""The collision cases (collision_cases.py) on the CPU: they hold what they are for. For a handful of odd bases -- 3, 2^64 - 1 and
seeded random 64-bit ones, none of them taken from the library -- the windows of every case have fewer distinct unordered hash pairs
{hf, hr} than k-mer classes, by exactly the number of engineered pairs where the base is an ordinary one. A table that settled
identity by the hash alone, in any of its 64 bits, would therefore report a wrong distinct_kmers on them: that is why
test_gpu_hash_collisions.py is sharp. Blocks of 256 and 512 bases do not collide. And the restatements the GPU tests compare with
run on every case; the few facts that make the cases readable are pinned here."""
import functools
import random

import pytest

import abundance_ref as A
import collision_cases as CC
import color_split_ref as S
import compact_ref as R
import fasta_in_ref as FA
import kmer_abundance_ref as KA
import kmer_color_ref as KC
import kmer_compare_ref as CMP
import kmer_locate_ref as LOC
import kmer_query_ref as Q
from matchtigs_amd.synth import canonical, revcomp

_rng = random.Random(64)
# bases under which nothing but the engineered pairs collides: 3, and random ones with B = 3 or 5 mod 8 (see the test further down)
GENERIC = [3] + [(_rng.getrandbits(64) & ~7) | (3, 5)[i % 2] for i in range(4)]
BASES = GENERIC + [2 ** 64 - 1]                               # ... and -1, the weakest odd base there is: B^i = +-1
CASES = CC.cases()
WINDOW_CASES = [(name, k) for name in ("pair", "strand", "one_record") for k in CC.KS]


# ---- the expectations the GPU tests share (computed once per process) ----
@functools.lru_cache(maxsize=None)
def compacted(name, k):
    return R.compact(CASES[name], k)


@functools.lru_cache(maxsize=None)
def compared(name, k, both):
    x, y = CASES[name]
    return CMP.compare([x, y], [y, x], k) if both else CMP.compare([x], [y], k)


@functools.lru_cache(maxsize=None)
def counted(k, m):
    """abundance_ref.compact_counted of [x, y, y] plus the count of every k-mer of its unitigs, in window order."""
    x, y = CASES["pair"]
    out = A.compact_counted([x, y, y], k, m)
    return out + (KA.window_counts(out[0], [x, y, y], k),)


@functools.lru_cache(maxsize=None)
def coloured(k, split):
    return S.compact_classes(CASES["pair"], [0, 1], 2, k, 1, split)


@functools.lru_cache(maxsize=None)
def indexed(which, k):
    """-> (the inputs, query, locate, abundance and color_hits of the restatements)."""
    c = CC.index_inputs(k)[which]
    return (c, Q.query(Q.index_set(c["index"], k), c["query"], k), LOC.locate(c["index"], c["query"], k),
            KA.abundance(c["index"], c["weights"], c["query"], k), KC.color_hits(c["index"], c["masks"], c["n_colors"], c["query"], k))


@functools.lru_cache(maxsize=None)
def joined():
    return FA.graph_dict(CASES["join"], CC.K_NODES)


# ---- the hash model ----
def test_the_blocks_are_two_classes_and_the_bad_letter_pairs_are_one():
    assert len(CC.X) == len(CC.Y) == 1024 and set(CC.X) == set(CC.Y) == {"A", "G"}
    assert CC.X[:8] == "AGGAGAAG" and CC.Y[:8] == "GAAGAGGA" and CC.X == CC.X[::-1]  # (even order: its own reverse)
    assert canonical(CC.X) != canonical(CC.Y) and CC.X != revcomp(CC.X)
    assert canonical(CC.thue_morse(10, "A", "C")) != canonical(CC.thue_morse(10, "C", "A"))
    for a, b in ("AT", "CG"):  # Y = revcomp(X): one class, no use
        assert CC.thue_morse(10, b, a) == revcomp(CC.thue_morse(10, a, b))


@pytest.mark.parametrize("base", BASES)
def test_the_model_is_the_headers_definition(base):
    """strand_hashes against the two sums written out term by term, hr(s) = hf(revcomp(s)), and the windows' hashes from prefix sums
    against strand_hashes of the windows."""
    s = CASES["pair"][0][30:30 + 75]
    k = len(s)
    hf = sum((CC.CODE[c] + 1) * pow(base, k - 1 - i, 1 << 64) for i, c in enumerate(s)) & CC.MASK
    hr = sum((4 - CC.CODE[c]) * pow(base, i, 1 << 64) for i, c in enumerate(s)) & CC.MASK
    assert CC.strand_hashes(s, base) == (hf, hr) and CC.strand_hashes(revcomp(s), base) == (hr, hf)
    for rec, k in ((s, 33), (s, 75), (CASES["pair"][1], 1031)):
        assert CC.window_hashes(rec, k, base) == [CC.strand_hashes(rec[i:i + k], base) for i in range(len(rec) - k + 1)]
    assert CC.window_hashes(s, 76, base) == []


@pytest.mark.parametrize("base", BASES)
def test_order_10_collides_in_all_64_bits_and_shorter_blocks_do_not(base):
    for a, b in (("A", "G"), ("A", "C"), ("C", "T")):
        for order in (8, 9, 10, 11):
            x, y = CC.thue_morse(order, a, b), CC.thue_morse(order, b, a)
            hx, hy = CC.strand_hashes(x, base), CC.strand_hashes(y, base)
            collide = CC.valuation(order, a, b, base) == 64  # from the factorisation of the difference
            assert (hx[0] == hy[0]) == collide and (hx[1] == hy[1]) == collide, (order, a, b)
            assert collide or order < 10  # order 10 and beyond: for every odd base
            if base in GENERIC:
                assert collide == (order >= 10), (order, a, b)  # nobody shortens the block
            if collide:  # a common prefix and suffix keep it
                p, s = "ACGTTGCA" * 3, "TTGACC"
                assert CC.strand_hashes(p + x + s, base) == CC.strand_hashes(p + y + s, base)
                assert CC.class_hash_key(CC.strand_hashes(p + x + s, base)) == CC.class_hash_key(CC.strand_hashes(revcomp(p + y + s), base))


def test_generic_bases_are_those_of_the_smallest_valuation():
    """B = 3 or 5 mod 8 (B^2 - 1 divisible by 8 and no more): order 9 reaches 2^55 at the most. The seed gives such bases."""
    assert all(b % 8 in (3, 5) for b in GENERIC) and len(set(BASES)) == len(BASES)
    assert max(CC.valuation(9, "A", "G", b) for b in GENERIC) <= 55 and CC.valuation(2, "A", "C", 2 ** 64 - 1) == 64


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("name,k", WINDOW_CASES)
def test_fewer_hash_pairs_than_classes(name, k, base):
    recs = CASES[name]
    classes = CC.window_classes(recs, k)
    pairs = {CC.class_hash_key(h) for r in recs for h in CC.window_hashes(r, k, base)}
    deficit = k - 1023
    assert deficit == CC.colliding_pairs(k)
    windows = sum(len(r) - k + 1 for r in recs)
    assert len(classes) == windows  # no k-mer repeats: every window is a class of its own
    assert len(pairs) <= len(classes) - deficit < len(classes)
    if base in GENERIC:
        assert len(pairs) == len(classes) - deficit
    # which windows: those that hold the whole block, against their counterparts
    if name == "one_record":
        h = CC.window_hashes(recs[0], k, base)
        for p in range(40 + 1024 - k, 41):
            assert recs[0][p:p + k] != recs[0][p + 1064:p + 1064 + k] and CC.class_hash_key(h[p]) == CC.class_hash_key(h[p + 1064])
    else:
        hx = CC.window_hashes(CASES["pair"][0], k, base)
        hy = CC.window_hashes(CASES["pair"][1], k, base)
        assert sum(a == b for a, b in zip(hx, hy)) >= deficit and [a == b for a, b in zip(hx, hy)][40 + 1024 - k:41] == [True] * deficit
        if name == "strand":  # the counterpart of window p lies at W - 1 - p of the reverse complement, strands swapped
            hz = CC.window_hashes(recs[1], k, base)
            assert [(f, r) for r, f in reversed(hz)] == hy


@pytest.mark.parametrize("base", BASES)
def test_the_nodes_and_the_ends_collide_as_k_minus_1_mers(base):
    L = CC.K_NODES - 1
    recs = CASES["nodes"]
    assert len(CC.window_classes(recs, L)) == 6
    pairs = {CC.class_hash_key(h) for r in recs for h in CC.window_hashes(r, L, base)}
    assert len(pairs) <= 5 and (len(pairs) == 5 or base not in GENERIC)
    # Their k-mers: C+X against T+Y and X+T against Y+C have other prefixes and suffixes and do not collide, but C+X and Y+C do.
    # The signed sum over the block is 0 mod 2^64, so X and Y both hash like the mean of A and G, 1024 times C: C+X ~ C^1025 ~ Y+C.
    assert CC.strand_hashes(CC.X, base) == CC.strand_hashes("C" * 1024, base) == CC.strand_hashes(CC.Y, base)
    kmer_pairs = {CC.class_hash_key(h) for r in recs for h in CC.window_hashes(r, CC.K_NODES, base)}
    assert len(kmer_pairs) <= 3 and (len(kmer_pairs) == 3 or base not in GENERIC)
    ends = [e for r in CASES["join"] for e in (r[:L], r[-L:])]
    assert len({canonical(e) for e in ends}) == 7
    pairs = {CC.class_hash_key(CC.strand_hashes(e, base)) for e in ends}
    assert len(pairs) <= 6 and (len(pairs) == 6 or base not in GENERIC)


# ---- the restatements on the cases ----
@pytest.mark.parametrize("name,k", WINDOW_CASES)
def test_the_window_cases_hold_what_they_are_for(name, k):
    recs = CASES[name]
    windows = sum(len(r) - k + 1 for r in recs)
    unitigs, stats, closed = compacted(name, k)
    assert stats["windows"] == stats["distinct_kmers"] == windows and not any(closed)
    if name == "one_record":
        assert unitigs == recs and windows == 2168 - k + 1
        return
    assert [len(r) - k + 1 for r in recs] == [{1024: 81, 1025: 80, 1031: 74, 1056: 49}[k]] * 2
    assert stats["unitigs"] == 2 and unitigs == recs and stats["distinct_kmers"] == 2 * (len(recs[0]) - k + 1)
    c = compared(name, k, False)
    assert c["common"] == 0 and c["only_in_a"] == c["only_in_b"] == windows // 2
    assert (c["first_only_in_a_record"], c["first_only_in_a_pos"], c["first_only_in_b_record"], c["first_only_in_b_pos"]) == (0, 0, 0, 0)
    c = compared(name, k, True)
    assert c["common"] == c["distinct_a"] == c["distinct_b"] == windows and c["only_in_a"] == c["only_in_b"] == 0


@pytest.mark.parametrize("k", CC.KS)
def test_the_counted_and_coloured_cases_hold_what_they_are_for(k):
    x, y = CASES["pair"]
    W = len(x) - k + 1
    unitigs, stats, _, ab, counts = counted(k, 1)
    assert unitigs == [x, y] and counts == [1] * W + [2] * W and ab["max_abundance"] == 2 and ab["spectrum"][1:4] == [W, W, 0]
    unitigs, stats, _, ab, counts = counted(k, 2)
    assert unitigs == [y] and counts == [2] * W and ab["dropped"] == W and stats["distinct_kmers"] == W
    for split in (False, True):
        unitigs, stats, _, _, col, classes = coloured(k, split)
        assert unitigs == [x, y] and col["kmer_colors"] == [1] * W + [2] * W and col["shared"] == [[W, 0], [0, W]]
        assert classes["masks"] == [1, 2] and classes["kmers"] == [W, W] and classes["runs"] == [1, 1]


@pytest.mark.parametrize("k", CC.KS)
def test_the_index_cases_hold_what_they_are_for(k):
    W = 1104 - k + 1
    c, q, loc, ab, col = indexed("lookup", k)
    assert q["found"] == loc["found"] == ab["found"] == col["found"] == [0, 0, W] and q["valid"] == [W] * 3
    assert loc["runs"] == [(2, 0, W, 0, 0, 0)] and ab["sum"] == [0, 0, sum(c["weights"])] and col["per_color"][:2] == [[0, 0], [0, 0]]
    c, q, loc, ab, col = indexed("claim", k)
    assert q["found"] == q["valid"] == [W] * 4
    assert loc["runs"] == [(0, 0, W, 0, 0, 0), (1, 0, W, 0, 1, 0), (2, 0, W, 1, 1, 0), (3, 0, W, 1, 0, 0)]
    assert ab["min"] == [10, 1000, 1000, 10] and ab["max"] == [10 + W - 1, 1000 + W - 1, 1000 + W - 1, 10 + W - 1]
    assert col["per_color"] == [[W, 0], [0, W], [0, W], [W, 0]]


def test_the_node_and_join_cases_hold_what_they_are_for():
    k = CC.K_NODES
    unitigs, stats, _ = compacted("nodes", k)
    assert stats["unitigs"] == 2 and stats["distinct_kmers"] == 4 and unitigs == CASES["nodes"]  # (merged nodes X and Y: 4 unitigs)
    g = joined()
    recs = CASES["join"]
    assert all(len(r) == 1054 for r in recs)
    # D1+X ends in X, X+D2 begins with it, revcomp(X+D5) ends in its mirror; Y+D3 begins with Y and D4+Y ends in it
    node_x, node_y = int(g["edge_to"][0]), int(g["edge_from"][4])
    assert int(g["edge_from"][2]) == node_x and int(g["edge_to"][8]) == int(g["mirror"][node_x])
    assert int(g["edge_to"][6]) == node_y and len({node_x, node_y, int(g["mirror"][node_x]), int(g["mirror"][node_y])}) == 4
    assert len(g["mirror"]) == 14  # X, Y and the five other ends, two nodes each (12 if X and Y were one class)
    assert g["edge_weight"].tolist() == [30] * 10
