"""The bubbles of the unitig graph as variant calls, made on the GPU (unitig_bubbles_device.hip): api.unitig_bubbles
against the restatement (unitig_bubbles_ref.py), every array exactly -- the hand cases of bubble_ref at narrow and wide k, alone
and concatenated; the unitigs of its 300 fuzz inputs; engineered arms whose lengths lie around the 16-base word, the 64-lane wave
and the 1 024-base step of the allele kernel, on either strand; a hub of 300 arms; 2 000 SNPs; abundances, colours, the errors."""
import random

import numpy as np
import pytest

import bubble_ref as B
import compact_ref as R
import unitig_bubbles_ref as UB

pytestmark = pytest.mark.gpu
KS = [5, 11, 16, 17, 31, 32, 33, 64]
HAND = ["snp_tie", "deletion_goes", "deletion_wins", "three_alleles", "long_arm", "hairpin", "ring_snp"]


def _dna(rng):
    return lambda n: "".join(rng.choice("ACGT") for _ in range(n))


def _unitigs(records, k):
    out = B.compact_simplified(records, k)
    return out[0], out[3]["unitig_sums"]


_hand = {}


def _hand_world(k):
    """{name: (unitigs, kc)} of bubble_ref's hand cases at k, [g, wide] among them, and all of them one after the other; made once."""
    if k in _hand:
        return _hand[k]
    rng = random.Random(25 if k == 11 else 2500 + k)
    cases = B.hand_cases(rng, _dna(rng), k)
    w = {name: _unitigs(cases[name][0], k) for name in HAND}
    w["wide"] = _unitigs([cases["_parts"]["g"], cases["_parts"]["wide"]], k)
    w["all"] = ([s for name in sorted(w) for s in w[name][0]], [c for name in sorted(w) for c in w[name][1]])
    _hand[k] = w
    return w


def _fuzz_world(k):
    """The unitigs of the fuzz inputs at k, one after the other, with their abundance sums."""
    seqs, kc = [], []
    for records, kk, _ in B.fuzz_cases():
        if kk == k:
            s, c = _unitigs(records, k)
            seqs += s
            kc += c
    return seqs, kc


def _nodes(rng, k, used):
    """Two (k-1)-mers an arm may run between, new on both strands."""
    dna = _dna(rng)
    while True:
        x, y = dna(k - 1), dna(k - 1)
        if x == R.revcomp(x) or y == R.revcomp(y) or R.canonical(x) == R.canonical(y) or R.canonical(x) in used or R.canonical(y) in used:
            continue
        used.update((R.canonical(x), R.canonical(y)))
        return x, y


def _change(s, i, rng):
    return s[:i] + B.other_base(rng, s[i]) + s[i + 1:]


ARM_LENGTHS = [15, 16, 17, 31, 32, 33, 63, 64, 65]
LONG_KMERS = 1100


def _arm_world(k, seed, turn):
    """Per length of ARM_LENGTHS (bases) and for one arm of LONG_KMERS k-mers: a bubble of the arm x + mid + y and variants of it -- a SNP
    in the last base of mid (the last before the k - 1 shared ones), one in its first base, one in its middle, three bases inserted
    right behind x, one base of the middle deleted, the first and the last base of mid changed (an mnp across the whole arm) -- and,
    for the long arm, a SNP beyond the first 1 024 bases from either end. Arm j of a bubble is given as its reverse complement iff
    (j + turn) is odd, the records are shuffled, and the first arm has three times the abundance of the others unless seed is odd
    (then all tie). -> (records, kc)."""
    rng = random.Random(seed)
    dna = _dna(rng)
    used = set()
    recs = []
    for length in ARM_LENGTHS + [LONG_KMERS + k - 1]:
        if length < 2 * (k - 1) + 1:
            continue  # (no room for a base between the two nodes)
        x, y = _nodes(rng, k, used)
        mid = dna(length - 2 * (k - 1))
        m = len(mid)
        mids = [mid, _change(mid, m - 1, rng), _change(mid, 0, rng), _change(mid, m // 2, rng), dna(3) + mid, mid[:m // 2] + mid[m // 2 + 1:]]
        if m > 2:
            mids.append(_change(_change(mid, 0, rng), m - 1, rng))
        if m > 1064:
            mids += [_change(mid, 1060, rng), _change(mid, m - 1061, rng), _change(_change(mid, 3, rng), m - 4, rng)]
        for j, v in enumerate(dict.fromkeys(mids)):  # (two variants of a short mid may coincide: once)
            arm = x + v + y
            recs.append((R.revcomp(arm) if (j + turn) % 2 else arm, (3 if j == 0 and seed % 2 == 0 else 1) * (len(arm) - k + 1)))
    rng.shuffle(recs)
    return [r for r, _ in recs], [c for _, c in recs]


def _hub_world(k=13, arms=300):
    rng = random.Random(77)
    dna = _dna(rng)
    used = set()
    x, y = _nodes(rng, k, used)
    mids = set()
    while len(mids) < arms:
        mids.add(dna(rng.randrange(1, 9)))
    recs = [x + m + y if i % 3 else R.revcomp(x + m + y) for i, m in enumerate(sorted(mids))]
    x2, y2 = _nodes(rng, k, used)
    recs += [x2 + "A" + y2, x2 + "C" + y2, dna(40)]  # a small bubble and a loose record beside the hub
    rng.shuffle(recs)
    return recs, [(u * 7919) % 997 + 1 for u in range(len(recs))]


def _kc(n):
    """Engineered abundance sums: small values and, on record 0, one above 2^32."""
    kc = [(u * 7919) % 997 + 1 for u in range(n)]
    if n:
        kc[0] = (1 << 32) + 6
    return kc


_cache = {}


def _world(name):
    """(records, k, L, kc) of a named world, made once."""
    if name not in _cache:
        kind, _, arg = name.partition(":")
        if kind == "hand":
            k, _, case = arg.partition("/")
            seqs, kc = _hand_world(int(k))[case]
            _cache[name] = (seqs, int(k), 4 * int(k), kc)
        elif kind == "fuzz":
            seqs, kc = _fuzz_world(int(arg))
            _cache[name] = (seqs, int(arg), 2 * int(arg), kc)
        elif kind == "arms":
            k, seed, turn = (int(x) for x in arg.split("/"))
            seqs, kc = _arm_world(k, seed, turn)
            _cache[name] = (seqs, k, 1200, kc)
        elif kind == "hub":
            seqs, kc = _hub_world()
            _cache[name] = (seqs, 13, 26, kc)
    return _cache[name]


_wants = {}


def _want(name):
    """The restated bubbles of a world with its own L and abundances, computed once and left unchanged."""
    if name not in _wants:
        seqs, k, L, kc = _world(name)
        _wants[name] = UB.bubbles_of_sequences(seqs, k, L, kc)
    return _wants[name]


def _assert_same(got, want, seqs, k):
    assert got.arm_off.dtype == np.uint64 and got.arm_off.tolist() == want["arm_off"]
    for f in UB.U32_FIELDS:
        a = getattr(got, f)
        assert a.dtype == np.uint32 and a.tolist() == want[f], f
    assert got.arm_strand.dtype == np.uint8 and got.arm_strand.tolist() == want["arm_strand"]
    assert got.arm_abundance.dtype == np.uint64 and got.arm_abundance.tolist() == want["arm_abundance"]
    if want["carried"] is None:
        assert got.carried is None
    else:
        assert got.carried.dtype == np.uint32 and got.carried.tolist() == want["carried"]
    assert len(got) == len(want["arm_off"]) - 1 and got.k == k
    assert got.kinds() == want["kinds"] and got.alleles(seqs) == want["alleles"] and got.describe() == UB.describe(want)
    assert got.tsv(seqs, k) == UB.bubbles_tsv(want)


def _graph(name):
    from matchtigs_amd import api

    if ("graph", name) not in _cache:
        seqs, k, _, _ = _world(name)
        _cache[("graph", name)] = api.Bigraph.from_sequences(seqs, k)
    return _cache[("graph", name)]


def _check(name, **kw):
    from matchtigs_amd import api

    seqs, k, L, kc = _world(name)
    got = api.unitig_bubbles(_graph(name), seqs, k, L, kc=kc, **kw)
    _assert_same(got, _want(name), seqs, k)
    return got


@pytest.mark.parametrize("k", KS)
def test_the_hand_cases(product_lib, k):
    from matchtigs_amd import api

    for case in HAND + ["wide", "all"]:
        got = _check(f"hand:{k}/{case}")
        if k <= 5:
            continue  # (a tiny k has other forks: the restatement alone says what comes out)
        kinds = sorted(x for x in got.kinds() if x != "ref")
        assert kinds == {"snp_tie": ["snp"], "deletion_goes": ["del"], "deletion_wins": ["ins"], "three_alleles": ["snp", "snp"],
                         "long_arm": ["complex", "snp"], "hairpin": [], "ring_snp": ["snp"], "wide": ["mnp"]}.get(case, kinds), case
        if case in ("snp_tie", "deletion_goes", "deletion_wins", "wide"):
            assert got.prefix.tolist() == [0, k - 1]
        if case == "wide":
            assert got.differences.tolist() == [0, 2] and len(got.alleles(_world(f"hand:{k}/wide")[0])[1][0]) == k
    seqs, kk, L, kc = _world(f"hand:{k}/all")
    if k > 5:
        assert "identical" in _want(f"hand:{k}/all")["kinds"]  # g's own stretches repeat from case to case
    # without abundances every arm weighs its k-mers, and a short L keeps the long arm out
    for some_L, some_kc in ((L, None), (k + 1, None), (L, _kc(len(seqs)))):
        got = api.unitig_bubbles(_graph(f"hand:{k}/all"), seqs, k, some_L, kc=some_kc)
        _assert_same(got, UB.bubbles_of_sequences(seqs, k, some_L, some_kc), seqs, k)


@pytest.mark.parametrize("k", [4, 5, 6])
def test_the_unitigs_of_the_fuzz_inputs(product_lib, k):
    got = _check(f"fuzz:{k}")
    assert len(got) >= 30 and int(got.arm_strand.sum()) >= 10 and int(np.diff(got.arm_off).max()) >= 3


@pytest.mark.parametrize("name", ["arms:7/2/0", "arms:7/2/1", "arms:7/3/0", "arms:12/4/1", "arms:33/5/0"])
def test_arms_around_the_word_the_wave_and_the_step(product_lib, name):
    from matchtigs_amd import api

    seqs, k, L, kc = _world(name)
    want = _want(name)
    if name.startswith("arms:7/2/"):  # what the world is for (the first arm of every bubble weighs most: it is the reference)
        lengths = sorted({want["arm_kmers"][a] + k - 1 for a in range(len(want["arm_kmers"])) if want["kinds"][a] == "ref"})
        assert lengths == ARM_LENGTHS + [LONG_KMERS + k - 1]
        assert {"snp", "mnp", "ins", "del"} <= set(want["kinds"]) and 0 < sum(want["arm_strand"]) < len(want["arm_strand"])
        assert max(want["prefix"]) > 1024 and max(want["suffix"]) > 1024 and max(want["differences"]) == 2
    got = _check(name)
    again = api.unitig_bubbles(_graph(name), seqs, k, L, kc=kc)  # a second call: equal arrays
    assert all(np.array_equal(getattr(again, f), getattr(got, f)) for f in UB.FIELDS)
    shorter = api.unitig_bubbles(_graph(name), seqs, k, 40, kc=kc)  # the arms of 40 k-mers and more are no candidates
    _assert_same(shorter, UB.bubbles_of_sequences(seqs, k, 40, kc), seqs, k)


def test_a_hub_of_three_hundred_arms(product_lib):
    got = _check("hub:")
    assert sorted(np.diff(got.arm_off).tolist()) == [2, 300]


@pytest.mark.parametrize("n_colors", [1, 3, 64])
def test_carriers(product_lib, n_colors):
    from matchtigs_amd import api

    name = "arms:7/2/1"
    seqs, k, L, kc = _world(name)
    rng = np.random.default_rng(n_colors)
    n_kmers = sum(len(s) - k + 1 for s in seqs)
    masks = rng.integers(0, 1 << min(n_colors, 62), n_kmers, dtype=np.uint64)
    if n_colors == 64:
        masks |= rng.integers(0, 4, n_kmers, dtype=np.uint64) << np.uint64(62)
        assert int((masks >> np.uint64(63)).sum()) > 100
    got = api.unitig_bubbles(_graph(name), seqs, k, L, kc=kc, kmer_colors=masks, n_colors=n_colors)
    want = UB.bubbles_of_sequences(seqs, k, L, kc, masks.tolist(), n_colors)
    _assert_same(got, want, seqs, k)
    assert got.carried.shape == (len(got.arm_unitig), n_colors) and got.carried.tolist() == want["carried"]
    assert got.arm_unitig.tolist() == want["arm_unitig"] and int(got.arm_kmers.max()) > 1000
    assert got.tsv(seqs, k, [f"s{c}" for c in range(n_colors)]) == UB.bubbles_tsv(want, [f"s{c}" for c in range(n_colors)])
    if n_colors == 64:
        assert int(got.carried[:, 63].sum()) > 0
    full = api.unitig_bubbles(_graph(name), seqs, k, L, kmer_colors=np.full(n_kmers, (1 << n_colors) - 1, np.uint64), n_colors=n_colors)
    assert np.array_equal(full.carried, np.repeat(full.arm_kmers[:, None], n_colors, axis=1))  # carried == kmers: every sample shows every allele


def test_products_beyond_64_bits(product_lib):
    from matchtigs_amd import api

    two = ["AACC" + "T" + "GGAT", "AACC" + "G" + "GGAT"]
    graph = api.Bigraph.from_sequences(two, 5)
    assert api.unitig_bubbles(graph, two, 5, 9, kc=[1 << 63, (1 << 63) + 1]).arm_unitig.tolist() == [1, 0]
    assert api.unitig_bubbles(graph, two, 5, 9, kc=[(1 << 63) + 1, 1 << 63]).arm_unitig.tolist() == [0, 1]
    got = api.unitig_bubbles(graph, two, 5, 9, kc=[(1 << 64) - 1, (1 << 64) - 1])
    assert got.arm_unitig.tolist() == [0, 1] and got.arm_abundance.tolist() == [(1 << 64) - 1] * 2 and got.kinds() == ["ref", "snp"]
    three = ["AACCTGGAT", "AACCGGGAT", "ATCCGGTT"]  # the case of test_unitig_bubbles_ref.py's TSV
    got = api.unitig_bubbles(api.Bigraph.from_sequences(three, 5), three, 5, 6, kc=[10, 5, 9], kmer_colors=[1, 1, 1, 1, 1, 2, 2, 3, 2, 2, 3, 3, 3, 1], n_colors=2)
    assert got.arm_unitig.tolist() == [2, 0, 1] and got.prefix.tolist() == [0, 4, 2] and got.suffix.tolist() == [0, 4, 6]
    assert got.carried.tolist() == [[4, 3], [5, 0], [1, 5]] and got.kinds() == ["ref", "ins", "ins"]


def test_the_smallest_arm_has_two_kmers(product_lib):
    """x = ACCGTA and y = GTATCC overlap in GTA: ACCGTATCC runs from x to y in two k-mers, beside an arm that goes the long way."""
    from matchtigs_amd import api

    k = 7
    seqs = ["ACCGTATC", "ACCGTA" + "GGCATTCAGGACAT" + "CGTATC", "TTTTGACCGTA", "CGTATCAAAG"]
    graph = api.Bigraph.from_sequences(seqs, k)
    for L in (0, 1, 2, 3, 20, 21, 100):
        got = api.unitig_bubbles(graph, seqs, k, L)
        _assert_same(got, UB.bubbles_of_sequences(seqs, k, L), seqs, k)
        assert len(got) == (1 if L >= 21 else 0), L  # the long arm has 20 k-mers
    # 1 : 1, the short arm is the smaller unitig and the reference: prefix and suffix are capped by its 8 bases
    assert got.kinds() == ["ref", "ins"] and got.arm_unitig.tolist() == [0, 1] and got.arm_kmers.tolist() == [2, 20]
    assert (int(got.prefix[1]), int(got.suffix[1])) == (2, 6) and got.alleles(seqs)[1] == ("", "CGTAGGCATTCAGGACAT")
    long_first = api.unitig_bubbles(graph, seqs, k, 100, kc=[2, 40, 1, 1])
    _assert_same(long_first, UB.bubbles_of_sequences(seqs, k, 100, [2, 40, 1, 1]), seqs, k)
    assert long_first.kinds() == ["ref", "del"] and (int(long_first.prefix[1]), int(long_first.suffix[1])) == (2, 6)


@pytest.fixture(scope="module")
def snps(product_lib):
    """DESIGN.md 25's world: 2 000 SNP records on 200 000 bases -> (records, the counted compaction's store and abundance sums)."""
    from matchtigs_amd import api

    k = 31
    rng = random.Random(2900)
    g = "".join(rng.choices("ACGT", k=200_000))
    records, sites = B.plant_snps(rng, g, k, 2000)
    store, compaction, abundance = api.compact_unitigs_counted(records, k, 1)
    assert compaction.unitigs == 1 + 3 * 2000
    return records, k, store, abundance.unitig_sums


def test_two_thousand_snps(snps):
    from matchtigs_amd import api

    records, k, store, sums = snps
    seqs = store.sequences()
    graph = api.Bigraph.from_sequences(store.arrays(), k)
    got = api.unitig_bubbles(graph, store, k, 2 * k, kc=sums)
    _assert_same(got, UB.bubbles_of_sequences(seqs, k, 2 * k, sums.tolist()), seqs, k)
    assert len(got) == 2000 and got.kinds().count("snp") == 2000 and got.prefix[1::2].tolist() == [k - 1] * 2000
    popped = api.compact_unitigs_simplified(records, k, pop_bubbles=2 * k, rounds=1)[6]
    assert len(got.arm_unitig) - len(got) == popped.arms == 2000
    t = api.last_unitig_bubbles_times()
    assert sorted(t) == sorted(["upload_ms", "group_ms", "allele_ms", "carrier_ms", "download_ms", "bubbles", "arms", "peak_arena_bytes"])
    assert t["bubbles"] == 2000 and t["arms"] == 4000 and t["peak_arena_bytes"] > 0
    assert min(t["upload_ms"], t["group_ms"], t["allele_ms"], t["download_ms"]) > 0
    # the same from a (data, offsets) pair, and dummy edges a tig computation left change nothing
    api.GreedytigAlgorithm.compute_tigs(graph, api.GreedytigAlgorithmConfiguration.new(1, k))
    assert graph.edge_count() > graph.original_edge_count()
    after = api.unitig_bubbles(graph, store.arrays(), k, 2 * k, kc=sums)
    assert all(np.array_equal(getattr(after, f), getattr(got, f)) for f in UB.FIELDS)


def test_nothing_to_find_and_the_arguments(product_lib):
    from matchtigs_amd import api

    empty = api.unitig_bubbles(api.Bigraph.from_unitig_links(np.zeros(0, np.uint64), []), [], 5, 9)
    assert len(empty) == 0 and empty.arm_off.tolist() == [0] and all(len(getattr(empty, f)) == 0 for f in UB.FIELDS[1:]) and empty.carried is None
    assert empty.describe() == "0 bubbles, 0 arms: 0 snp, 0 mnp, 0 ins, 0 del, 0 complex; the largest has 0 arms"
    seqs = ["AACCTGGAT", "AACCGGGAT", "TTTTTGCAGAG"]
    graph = api.Bigraph.from_sequences(seqs, 5)
    masks = np.ones(17, np.uint64)
    for L in (0, 1, 5):
        none = api.unitig_bubbles(graph, seqs, 5, L, kmer_colors=masks, n_colors=2)
        assert len(none) == 0 and none.arm_off.tolist() == [0] and none.carried.shape == (0, 2)
    assert len(api.unitig_bubbles(graph, seqs, 5, 6)) == 1
    for kw in (dict(kc=[1, 2]), dict(kmer_colors=masks[:-1], n_colors=2), dict(kmer_colors=masks, n_colors=0), dict(kmer_colors=masks, n_colors=65),
               dict(kmer_colors=masks)):
        with pytest.raises(ValueError):
            api.unitig_bubbles(graph, seqs, 5, 6, **kw)
    with pytest.raises(ValueError):
        api.unitig_bubbles(graph, seqs[:2], 5, 6)
    with pytest.raises(ValueError):
        api.unitig_bubbles(graph, seqs, 10, 6)  # a record is shorter than k
