"""Monochromatic unitigs and colour classes on the GPU against the restatement (color_split_ref.py), as exact integers:
the split and the unsplit store with their counts, masks and classes on the fixture of test_color_split_ref.py (the colour cases of
test_gpu_kmer_color.py plus closed walks that open, a chain that comes out flipped, one that spells across the wrap-around, a closed
walk that stays closed, neighbouring unitigs of one mask) at k = 4, 31, 32, 33, 3 and 64 colours, m = 1 and 2; every call twice; a
store as input; the empties; the arguments; and the dictionary where its kernels take another path -- more runs and more windows than
one sweep of the counts kernel's grid, runs across a wave's and a workgroup's edge, more classes than the LDS table holds, one class
only, a unitig boundary inside a stretch of one mask at a multiple of 64 and one before it."""
import random

import numpy as np
import pytest

import color_split_ref as S
import kmer_abundance_ref as KA
import kmer_color_ref as KC
from matchtigs_amd import _lib, api, synth
from test_color_split_ref import CS, split_case
from test_gpu_kmer_color import KS, _dna

pytestmark = pytest.mark.gpu
SWEEP = api.COLOR_CLASS_GRID * api.COLOR_CLASS_BLOCK  # the runs one sweep of the counts kernel covers


@pytest.fixture(scope="module")
def gpu(product_lib):
    import torch

    if product_lib.mtg_device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("these tests need a GPU: the compaction has no CPU path")
    return torch


@pytest.fixture(scope="module", params=[(k, C) for k in KS for C in CS], ids=lambda p: f"k{p[0]}-C{p[1]}")
def case(request):
    k, C = request.param
    recs, colors, _ = split_case(k, C)
    return k, C, recs, colors, {}


def _want(case, m, split):
    k, C, recs, colors, cache = case
    if (m, split) not in cache:
        cache[(m, split)] = S.compact_classes(recs, colors, C, k, m, split)
    return cache[(m, split)]


def _assert_classes(cc, want, kmer_colors, n_unitigs, split):
    for f in ("masks", "kmers", "runs", "first", "kmer_class"):
        got = getattr(cc, f)
        assert got.dtype == (np.uint32 if f == "kmer_class" else np.uint64), f
        assert np.array_equal(got, np.asarray(want[f], got.dtype)), f
    assert int(cc.kmers.sum()) == len(kmer_colors) == len(cc.kmer_class) and int(cc.runs.sum()) == want["n_runs"]
    assert (np.diff(cc.first.astype(np.int64)) > 0).all() and (len(cc.first) == 0 or cc.first[0] == 0)
    assert np.array_equal(cc.masks[cc.kmer_class], kmer_colors)
    if split:
        assert int(cc.runs.sum()) == n_unitigs


def _same(a, b):
    """Two results of the classes call, array for array."""
    assert a[0].sequences() == b[0].sequences() and np.array_equal(a[0].arrays()[1], b[0].arrays()[1]) and a[1] == b[1]
    for f in ("distinct_all", "distinct_kept", "max_abundance", "kept_occurrences"):
        assert getattr(a[2], f) == getattr(b[2], f), f
    for f in ("spectrum", "unitig_sums", "kmer_counts"):
        assert np.array_equal(getattr(a[2], f), getattr(b[2], f)), f
    for f in ("kmer_colors", "per_color", "shared", "occupancy"):
        assert np.array_equal(getattr(a[3], f), getattr(b[3], f)), f
    if len(a) > 4 and len(b) > 4:
        for f in ("masks", "kmers", "runs", "first", "kmer_class"):
            assert np.array_equal(getattr(a[4], f), getattr(b[4], f)), f


def test_the_constants_are_the_librarys(gpu):
    assert api.color_class_limits() == {"lds": api.COLOR_CLASS_LDS, "grid": api.COLOR_CLASS_GRID, "block": api.COLOR_CLASS_BLOCK}
    assert api.COLOR_CLASS_LDS <= 4096


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("m", [1, 2])
def test_store_stats_and_classes_equal_the_restatement(gpu, case, m, split):
    k, C, recs, colors, _ = case
    unitigs, stats, closed, ab, col, classes = _want(case, m, split)
    unsplit = _want(case, m, False)
    before = (api.compact_unitigs(recs, k), api.compact_unitigs_counted(recs, k, m, kmer_counts=True), api.compact_unitigs_colored(recs, k, colors, C, m))
    got = api.compact_unitigs_colored_classes(recs, k, colors, C, min_abundance=m, split=split)
    store, c, a, co, cc = got
    print(c.describe(), "|", cc.describe())
    assert store.sequences() == unitigs and c == api.Compaction(**stats)
    assert c.distinct_kmers == c.unitig_characters - (k - 1) * c.unitigs and c.closed_walks == sum(closed)
    for f in ("distinct_all", "distinct_kept", "max_abundance", "kept_occurrences"):
        assert getattr(a, f) == ab[f] == unsplit[3][f], f
    assert a.spectrum.tolist() == ab["spectrum"] and a.unitig_sums.dtype == np.uint64 and a.unitig_sums.tolist() == ab["unitig_sums"]
    assert a.kmer_counts.dtype == np.uint32 and a.kmer_counts.tolist() == ab["kmer_counts"]
    assert co.n_colors == C and co.kmer_colors.dtype == np.uint64 and co.kmer_colors.tolist() == col["kmer_colors"]
    for f in ("per_color", "shared", "occupancy"):  # functions of the k-mer set: the unsplit call's
        assert getattr(co, f).tolist() == col[f] == unsplit[4][f], f
    _assert_classes(cc, classes, co.kmer_colors, c.unitigs, split)
    n = [len(u) - k + 1 for u in unitigs]
    assert cc.unitig_classes(n).dtype == np.uint32 and cc.unitig_classes(n).tolist() == [classes["kmer_class"][i] for i in np.cumsum([0] + n[:-1])]
    if split:  # monochromatic: one class per unitig
        assert np.array_equal(np.repeat(cc.unitig_classes(n), n), cc.kmer_class)
        if k > 4 and m == 1:
            assert c.unitigs > before[2][1].unitigs and c.closed_walks < before[2][1].closed_walks  # (closed walks of two masks open)
    else:  # everything but the classes is the coloured call's, array for array
        _same(got, before[2])
    # twice the same; arrays go in as lists do; the older calls answer as before
    cat = np.frombuffer("".join(recs).encode(), np.uint8)
    off = np.concatenate([[0], np.cumsum([len(s) for s in recs])]).astype(np.uint64)
    _same(got, api.compact_unitigs_colored_classes(recs, k, colors, C, m, split))
    _same(got, api.compact_unitigs_colored_classes((cat, off), k, np.array(colors, np.int64), C, m, bool(split)))
    after = (api.compact_unitigs(recs, k), api.compact_unitigs_counted(recs, k, m, kmer_counts=True), api.compact_unitigs_colored(recs, k, colors, C, m))
    assert before[0][0].sequences() == after[0][0].sequences() and before[0][1] == after[0][1]
    _same(before[1] + (before[2][3],), after[1] + (after[2][3],))
    _same(before[2], after[2])
    t = api.last_color_class_times()
    assert set(t) == {"heads_ms", "table_ms", "ids_ms", "counts_ms", "download_ms"}
    assert api.last_kmer_color_times()["stats_ms"] > 0 and api.last_compact_times()["insert_ms"] > 0


def test_the_times_belong_to_the_classes_call(gpu):
    recs, colors, _ = split_case(31, 3)
    api.compact_unitigs_colored_classes(recs, 31, colors, 3, split=True)
    t = api.last_color_class_times()
    assert all(t[f] > 0 for f in ("heads_ms", "table_ms", "ids_ms", "counts_ms")) and t["download_ms"] >= 0


@pytest.mark.parametrize("split", [False, True])
def test_a_store_goes_in_as_well(gpu, split):
    recs, colors, _ = split_case(31, 3)
    store = api.compact_unitigs(recs, 31)[0]  # its records: the unitigs; colour them by their number
    cols = [i % 3 for i in range(len(store))]
    want = S.compact_classes(store.sequences(), cols, 3, 31, 1, split)
    for _ in range(2):
        out, c, a, co, cc = api.compact_unitigs_colored_classes(store, 31, cols, 3, split=split)
        assert out.sequences() == want[0] and c == api.Compaction(**want[1]) and co.kmer_colors.tolist() == want[4]["kmer_colors"]
        _assert_classes(cc, want[5], co.kmer_colors, c.unitigs, split)
    if not split:
        assert out.sequences() == store.sequences()


@pytest.mark.parametrize("k", KS)
def test_empties(gpu, k):
    rng = random.Random(k)
    for split in (False, True):
        for recs in ([], [""], [_dna(rng, n) for n in (k - 1, 0, k // 2)], (np.zeros(0, np.uint8), np.zeros(1, np.uint64))):
            n = len(recs) if isinstance(recs, list) else 0
            for _ in range(2):
                store, c, a, co, cc = api.compact_unitigs_colored_classes(recs, k, [2] * n, 3, split=split)
                assert len(store) == 0 and c.distinct_kmers == 0 and len(a.kmer_counts) == 0 and len(co.kmer_colors) == 0 and not co.occupancy.any()
                assert all(len(getattr(cc, f)) == 0 and getattr(cc, f).dtype == np.uint64 for f in ("masks", "kmers", "runs", "first"))
                assert len(cc.kmer_class) == 0 and cc.kmer_class.dtype == np.uint32 and cc.describe() == "0 classes in 0 runs"
                assert len(cc.unitig_classes([])) == 0
        recs = [_dna(rng, 3 * k), _dna(rng, 2 * k)]
        store, c, a, co, cc = api.compact_unitigs_colored_classes(recs, k, [0, 1], 2, min_abundance=10 ** 6, split=split)  # nothing reaches the threshold
        assert len(store) == 0 and a.distinct_kept == 0 and a.distinct_all > 0 and len(cc.masks) == 0 and len(cc.kmer_class) == 0


def test_bad_arguments_raise_before_the_library_is_called(monkeypatch):
    def no_library():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_lib, "load", no_library)
    recs = ["ACGTACGTAC", "ACGTTTGACA"]
    for args, kw in ((([0, 1], 2), {"min_abundance": 0}), (([0, 1], 0), {}), (([0, 1], 65), {}), (([0], 2), {}), (([0, 2], 2), {}),
                     (([0, -1], 2), {}), (([0.5, 1.0], 2), {}), (([0, 1], True), {}), (([0, 1], 2), {"split": 2}), (([0, 1], 2), {"split": None}),
                     (([0, 1], 2), {"split": "yes"})):
        with pytest.raises(ValueError):
            api.compact_unitigs_colored_classes(recs, 4, *args, **kw)
    with pytest.raises(ValueError):
        api.ColorClasses(*(np.zeros(1, np.uint64),) * 4, np.zeros(5, np.uint32)).unitig_classes([2, 2])


def test_the_dictionary_of_masks_handed_in(gpu):
    masks, n = [5, 5, 9, 5, 5, 1 << 63, 9], [2, 3, 2]
    for _ in range(2):
        cc = api.color_classes(masks, n)
        _assert_classes(cc, S.class_dictionary(n, masks), np.array(masks, np.uint64), 3, False)
        assert cc.masks.tolist() == [5, 9, 1 << 63] and cc.kmers.tolist() == [4, 2, 1] and cc.runs.tolist() == [2, 2, 1] and cc.first.tolist() == [0, 2, 5]
    empty = api.color_classes([], [])
    assert len(empty.masks) == 0 and len(empty.kmer_class) == 0 and empty.kmer_class.dtype == np.uint32
    for bad in (([5, 0], [2]), ([5, 5], [1]), ([5, 5], [2, 0]), ([5], [1.0]), ([[5]], [1])):
        with pytest.raises(ValueError):
            api.color_classes(*bad)


# ---- the dictionary where its kernels can go wrong: expectations from the numpy restatement on the call's own masks and lengths,
# which the small cases above tie to the dict reference, after the masks themselves have been checked against the input ----
def _assert_dictionary(got, k, split):
    store, c, a, co, cc = got
    n = (np.diff(store.arrays()[1]).astype(np.int64) - (k - 1))
    want = S.class_dictionary_np(n, co.kmer_colors)
    _assert_classes(cc, want, co.kmer_colors, c.unitigs, split)
    _assert_classes(api.color_classes(co.kmer_colors, n), want, co.kmer_colors, c.unitigs, split)  # the dictionary alone, of the same masks
    return want, n


def _run_bounds(want, n, masks):
    head = np.ones(len(masks), bool)
    head[1:] = masks[1:] != masks[:-1]
    head[np.cumsum(n) - n] = True
    starts = np.flatnonzero(head)
    return starts, np.append(starts[1:], len(masks)) - 1  # first and last window of every run


@pytest.fixture(scope="module")
def long_genome():
    return synth.random_genome(SWEEP + 9_000, seed=21, haplotypes=1)[0]


@pytest.mark.parametrize("split", [False, True])
def test_more_windows_than_one_sweep_and_runs_across_wave_and_workgroup_edges(gpu, long_genome, split):
    """(a) One genome in colour 0, colour 1 on a few stretches: across a wave's edge (window 128), a workgroup's (1024), a scan chunk's
    (4096) and the first sweep's end."""
    k, g = 31, long_genome
    stretches = [(100, 200), (1000, 1100), (4000, 4200), (SWEEP - 100, SWEEP + 100), (len(g) - k - 5, len(g) - k + 1)]
    recs, colors = [g] + [g[a:b + k - 1] for a, b in stretches], [0] + [1] * len(stretches)
    got = api.compact_unitigs_colored_classes(recs, k, colors, 2, split=split)
    masks = got[3].kmer_colors
    assert got[1].distinct_kmers == len(g) - k + 1 > SWEEP
    expect = np.ones(len(masks), np.uint64)
    for a, b in stretches:
        expect[a:b] = 3
    assert np.array_equal(masks, expect)  # one unitig read forwards unsplit; the split keeps the k-mers in place (leaders ascend)
    want, n = _assert_dictionary(got, k, split)
    lo, hi = _run_bounds(want, n, masks)
    assert ((lo // 64 != hi // 64) & (masks[lo] == 3)).any() and ((lo // api.COLOR_CLASS_BLOCK != hi // api.COLOR_CLASS_BLOCK) & (masks[lo] == 3)).any()
    assert got[4].masks.tolist() == [1, 3] and got[4].runs.tolist() == [len(stretches), len(stretches)] and got[4].first.tolist() == [0, 100]
    assert got[1].unitigs == (2 * len(stretches) if split else 1)
    _same(got, api.compact_unitigs_colored_classes(recs, k, colors, 2, split=split))


@pytest.mark.parametrize("split", [False, True])
def test_more_runs_than_one_sweep(gpu, long_genome, split):
    """More runs than the counts kernel's grid takes in one sweep: colour 1 on windows 4 j and 4 j + 1 of a genome in colour 0, so that
    the masks alternate two by two and every wave sees both classes 32 times."""
    k = 31
    g = long_genome + synth.random_genome(SWEEP + 9_000, seed=22, haplotypes=1)[0]
    N = len(g) - k + 1
    recs, colors = [g] + [g[j:j + k + 1] for j in range(0, N - 1, 4)], [0] + [1] * len(range(0, N - 1, 4))
    got = api.compact_unitigs_colored_classes(recs, k, colors, 2, split=split)
    masks = got[3].kmer_colors
    covered = np.zeros(N, bool)
    for j in range(0, N - 1, 4):
        covered[j:j + 2] = True
    assert np.array_equal(masks, np.where(covered, 3, 1).astype(np.uint64)) and got[1].distinct_kmers == N
    want, n = _assert_dictionary(got, k, split)
    assert want["n_runs"] > SWEEP + 64 and len(got[4].masks) == 2 and int(got[4].runs.sum()) == want["n_runs"]
    assert got[1].unitigs == (want["n_runs"] if split else 1)
    _same(got, api.compact_unitigs_colored_classes(recs, k, colors, 2, split=split))


def test_more_classes_than_the_lds_table_holds(gpu):
    """(b) More than four times COLOR_CLASS_LDS classes: random k-mers, each in two or three records of one window, of colours drawn so
    that no two k-mers have the same mask."""
    import itertools

    k, n = 31, 4 * api.COLOR_CLASS_LDS + 100
    rng = random.Random(77)
    combos = list(itertools.combinations(range(64), 2)) + list(itertools.combinations(range(64), 3))
    rng.shuffle(combos)
    recs, colors = [], []
    for j in range(n):
        x = _dna(rng, k)
        for i, c in enumerate(combos[j]):
            recs.append(synth.revcomp(x) if i % 2 else x)
            colors.append(c)
    order = list(range(len(recs)))
    rng.shuffle(order)
    recs, colors = [recs[i] for i in order], [colors[i] for i in order]
    masks = KC.kmer_masks(recs, colors, k)
    assert len(masks) == len(set(masks.values())) == n
    for split in (False, True):
        got = api.compact_unitigs_colored_classes(recs, k, colors, 64, split=split)
        store, c, a, co, cc = got
        assert co.kmer_colors.tolist() == [masks[synth.canonical(w)] for w in KA.windows(store.sequences(), k)]
        dict_want = S.class_dictionary([len(u) - k + 1 for u in store.sequences()], co.kmer_colors.tolist())
        _assert_classes(cc, dict_want, co.kmer_colors, c.unitigs, split)
        _assert_dictionary(got, k, split)
        assert len(cc.masks) == n > 4 * api.COLOR_CLASS_LDS and (cc.kmers == 1).all() and (cc.runs == 1).all() and c.unitigs == n
        _same(got, api.compact_unitigs_colored_classes(recs, k, colors, 64, split=split))


def test_a_few_classes_beyond_the_lds_table_with_many_runs_each(gpu):
    """Classes from COLOR_CLASS_LDS on that many runs of one wave share: the global path of the wave's combined add. COLOR_CLASS_LDS
    single k-mers open that many classes; then two masks alternate along one genome."""
    import itertools

    k = 31
    rng = random.Random(78)
    combos = (list(itertools.combinations(range(2, 64), 2)) + list(itertools.combinations(range(2, 64), 3)))[:api.COLOR_CLASS_LDS + 5]
    recs, colors = [], []
    for combo in combos:
        x = _dna(rng, k)
        recs += [x] * len(combo)
        colors += list(combo)
    g = synth.random_genome(6_000, seed=23, haplotypes=1)[0]
    N = len(g) - k + 1
    recs += [g] + [g[j:j + k + 3] for j in range(0, N - 3, 8)]
    colors += [0] + [1] * len(range(0, N - 3, 8))
    for split in (False, True):
        got = api.compact_unitigs_colored_classes(recs, k, colors, 64, split=split)
        want, n = _assert_dictionary(got, k, split)
        cc = got[4]
        assert len(cc.masks) == len(combos) + 2 and cc.masks[-2:].tolist() == [3, 1] and int(cc.runs[-2:].min()) > 700
        _same(got, api.compact_unitigs_colored_classes(recs, k, colors, 64, split=split))


@pytest.mark.parametrize("split", [False, True])
def test_everything_in_one_class(gpu, long_genome, split):
    """(c)"""
    k = 31
    got = api.compact_unitigs_colored_classes([long_genome, long_genome[500:900]], k, [0, 0], 1, split=split)
    _assert_dictionary(got, k, split)
    N = len(long_genome) - k + 1
    cc = got[4]
    assert cc.masks.tolist() == [1] and cc.kmers.tolist() == [N] and cc.runs.tolist() == [1] and cc.first.tolist() == [0] and not cc.kmer_class.any()


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("first", [128, 127])
def test_a_unitig_boundary_inside_one_mask_at_a_multiple_of_64(gpu, first, split):
    """(d) Two unitigs of one mask; the second begins at window 128 / 127: a run head that only the unitig's offset gives."""
    k = 31
    rng = random.Random(first)
    recs = [_dna(rng, first + k - 1), _dna(rng, k + 50)]
    got = api.compact_unitigs_colored_classes(recs, k, [1, 1], 2, split=split)
    store, c, a, co, cc = got
    assert [len(u) - k + 1 for u in store.sequences()] == [first, 51] and set(co.kmer_colors.tolist()) == {2}
    _assert_dictionary(got, k, split)
    assert cc.masks.tolist() == [2] and cc.kmers.tolist() == [first + 51] and cc.runs.tolist() == [2] and cc.first.tolist() == [0]
