"""The k-mer selection on the GPU (api.compact_unitigs_selected) against the restatement (kmer_select_ref.py), field for
field and as exact integers: the store, the compaction's counts, the abundance and the colour statistics over S_m, the counts and masks
of the output in window order, and the selection's counts -- at the k where the code takes another path (4, 31 and 32 on either side of
the narrow / wide switch, 33), with 1, 3 and 64 colours, m in {1, 2} and every rule set of kmer_select_cases.py; the trivial selection
byte for byte against the calls without one; filter windows that collide with the main record's in all 64 hash bits (k = 1025); a
filter over several workgroups and scans over more than one tile; cleaning, bubbles and the split by their properties; and the calls
without a selection before and after a selected one."""
import numpy as np
import pytest

import compact_ref
import kmer_select_cases as SC
import kmer_select_ref as S
import test_gpu_kmer_color as TC
from matchtigs_amd import api, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(product_lib):
    import torch

    if product_lib.mtg_device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("these tests need a GPU: the compaction has no CPU path")
    return torch


def _selection(kwargs, filter_records=None):
    """api.KmerSelection for the restatement's keyword arguments; filter_records: the same filter records in their stored order."""
    kw = {"require": kwargs.get("require", 0), "forbid": kwargs.get("forbid", 0), "min_colors": kwargs.get("min_colors", 0),
          "max_colors": kwargs.get("max_colors", 64), "subtract_min_abundance": kwargs.get("A_", 1), "intersect_min_abundance": kwargs.get("B", 1)}
    if filter_records is not None:
        return api.KmerSelection(filter_records=filter_records, **kw)
    return api.KmerSelection(subtract=kwargs.get("subtract"), intersect=kwargs.get("intersect"), **kw)


def _assert_equals_ref(got, want, k, C):
    store, c, a, col, classes, cleaning, bubbles, sel = got
    assert store.sequences() == want["unitigs"] and c == api.Compaction(**want["stats"])
    ab = want["abundance"]
    for f in ("distinct_all", "distinct_kept", "max_abundance", "kept_occurrences"):
        assert getattr(a, f) == ab[f], f
    assert a.spectrum.tolist() == ab["spectrum"] and a.unitig_sums.tolist() == ab["unitig_sums"]
    assert a.kmer_counts.dtype == np.uint32 and a.kmer_counts.tolist() == ab["kmer_counts"]
    if C:
        TC._assert_colors_equal_ref(col, want["colours"], C)  # masks of the output in window order; the statistics over S_m
        assert classes is not None and (len(col.kmer_colors) == 0 or np.array_equal(classes.masks[classes.kmer_class], col.kmer_colors))
    else:
        assert col is None and classes is None
    ws = want["selection"]
    print("selection", sel, ws)
    for f in ("input_kmers", "selected", "selected_occurrences", "subtract_windows", "intersect_windows", "subtract_hits", "intersect_hits"):
        assert getattr(sel, f) == ws[f], f
    for rule in S.RULES:
        assert getattr(sel, "rejected_" + rule) == ws["rejected_" + rule], rule
    assert sel.per_color_selected.dtype == np.uint64 and sel.per_color_selected.tolist() == ws["per_color_selected"]
    assert sel.rejected == ws["input_kmers"] - ws["selected"] and str(ws["selected"]) in sel.describe()
    assert cleaning == api.Cleaning(0, 0, 0, 0, 0, 0) and bubbles == api.Bubbles(0, 0, 0)


@pytest.mark.parametrize("k,C,m,name", SC.grid(), ids=lambda v: str(v))
def test_selected_compaction_equals_the_restatement(gpu, k, C, m, name):
    recs, colors, kwargs, filter_records = SC.case(k, C, name)
    want = S.compact_selected(recs, k, m, colors, C, **kwargs)
    got = api.compact_unitigs_selected(recs, k, _selection(kwargs, filter_records), min_abundance=m, record_colors=colors, n_colors=C, kmer_counts=True)
    _assert_equals_ref(got, want, k, C)
    t = api.last_compact_times()
    assert t["select_ms"] > 0 and (t["filter_ms"] > 0) == (want["selection"]["subtract_windows"] + want["selection"]["intersect_windows"] > 0)
    if name == "everything-rejected":
        assert len(got[0]) == 0 and got[1].distinct_kmers == 0 and got[2].distinct_kept > 0 and got[3].occupancy.sum() == got[2].distinct_kept


@pytest.mark.parametrize("k", SC.KS)
def test_without_colours_the_filters_alone(gpu, k):
    recs, _ = TC._case(k, 3)
    subtract, intersect, _ = SC.filters(k, recs)
    for m, kwargs in ((1, {"subtract": subtract, "A_": 2, "intersect": intersect}), (2, {"intersect": intersect, "B": 2})):
        want = S.compact_selected(recs, k, m, **kwargs)
        _assert_equals_ref(api.compact_unitigs_selected(recs, k, _selection(kwargs), min_abundance=m, kmer_counts=True), want, k, 0)
    # the filter sets as a store and as arrays
    store = api.compact_unitigs(S.pieces(subtract), k)[0]  # (its records: unitigs that spell the subtract set's k-mers once each)
    want = S.compact_selected(recs, k, subtract=store.sequences())
    cat = np.frombuffer("".join(store.sequences()).encode(), np.uint8)
    off = np.concatenate([[0], np.cumsum([len(s) for s in store.sequences()])]).astype(np.uint64)
    for given in (store, (cat, off)):
        _assert_equals_ref(api.compact_unitigs_selected(recs, k, api.KmerSelection(subtract=given), kmer_counts=True), want, k, 0)


@pytest.mark.parametrize("k", SC.KS)
@pytest.mark.parametrize("m", [1, 2])
def test_the_trivial_selection_is_byte_identical(gpu, k, m):
    recs, colors = TC._case(k, 64)
    store, c, a, col = api.compact_unitigs_colored(recs, k, colors, 64, min_abundance=m)
    got = api.compact_unitigs_selected(recs, k, api.KmerSelection(), min_abundance=m, record_colors=colors, n_colors=64)
    for x, y in ((store, got[0]),):
        assert all(np.array_equal(p, q) for p, q in zip(x.arrays(), y.arrays()))
    assert got[1] == c
    for f in ("distinct_all", "distinct_kept", "max_abundance", "kept_occurrences"):
        assert getattr(got[2], f) == getattr(a, f), f
    for f in ("spectrum", "unitig_sums", "kmer_counts"):
        assert np.array_equal(getattr(got[2], f), getattr(a, f)) and getattr(got[2], f).dtype == getattr(a, f).dtype, f
    for f in ("kmer_colors", "per_color", "shared", "occupancy"):
        assert np.array_equal(getattr(got[3], f), getattr(col, f)), f
    assert got[7].selected == got[7].input_kmers == a.distinct_kept and got[7].selected_occurrences == a.kept_occurrences
    assert np.array_equal(got[7].per_color_selected, col.per_color)
    store2, c2, a2 = api.compact_unitigs_counted(recs, k, m, kmer_counts=True)
    plain = api.compact_unitigs_selected(recs, k, api.KmerSelection(), min_abundance=m, kmer_counts=True)
    assert all(np.array_equal(p, q) for p, q in zip(store2.arrays(), plain[0].arrays())) and plain[1] == c2
    assert np.array_equal(plain[2].kmer_counts, a2.kmer_counts) and np.array_equal(plain[2].unitig_sums, a2.unitig_sums)
    assert plain[3] is None and len(plain[7].per_color_selected) == 0 and plain[7].selected == a2.distinct_kept


def test_windows_that_collide_in_all_64_hash_bits_are_not_subtracted(gpu):
    k, main, other = SC.collision_case()
    for subtract, hits in ((other, 0), (main, len(main) - k + 1)):
        want = S.compact_selected([main], k, subtract=[subtract])
        got = api.compact_unitigs_selected([main], k, api.KmerSelection(subtract=[subtract]), kmer_counts=True)
        _assert_equals_ref(got, want, k, 0)
        assert got[7].subtract_hits == hits and got[7].subtract_windows == len(main) - k + 1
        assert got[0].sequences() == ([main] if hits == 0 else [])
    got = api.compact_unitigs_selected([main], k, api.KmerSelection(intersect=[other, synth.revcomp(main)[:k + 3]]), kmer_counts=True)
    assert got[7].selected == 4 and got[7].intersect_hits == 4  # the last four windows of the main record, from the other strand


@pytest.mark.parametrize("k", SC.SIZE_KS)
def test_at_size(gpu, k):
    """k = 5 over 200 kb: the filter's windows span five workgroups. Only 512 canonical 5-mers exist, so the scans of more than one tile
    (2 048 items) over S_m and S_sel are reached with the same input at k = 9."""
    recs, colors, subtract, intersect = SC.size_case(k)
    kwargs = {"subtract": subtract, "A_": 3, "intersect": intersect, "min_colors": 2}
    want = S.compact_selected(recs, k, 2, colors, 3, **kwargs)
    if k == 9:
        assert want["selection"]["input_kmers"] > want["selection"]["selected"] > 2048
    got = api.compact_unitigs_selected(recs, k, _selection(kwargs), min_abundance=2, record_colors=colors, n_colors=3, kmer_counts=True)
    _assert_equals_ref(got, want, k, 3)


def _kmers(seqs, k):
    return [synth.canonical(s[i:i + k]) for s in seqs for i in range(len(s) - k + 1)]


@pytest.mark.parametrize("k", [4, 31, 32])
@pytest.mark.parametrize("split", [False, True])
def test_cleaning_bubbles_and_split_act_on_the_selected_set(gpu, k, split):
    recs, colors = TC._case(k, 3)
    subtract, intersect, _ = SC.filters(k, recs)
    kwargs = {"subtract": subtract, "A_": 2, "intersect": intersect + recs[50:], "min_colors": 1, "max_colors": 2}
    selected = S.compact_selected(recs, k, 1, colors, 3, **kwargs)["selected_set"]
    store, c, a, col, classes, cleaning, bubbles, sel = api.compact_unitigs_selected(
        recs, k, _selection(kwargs), pop_bubbles=2 * k, clip_tips=k, remove_isolated=k, rounds=3, record_colors=colors, n_colors=3, split=split,
        kmer_counts=True)
    out = _kmers(store.sequences(), k)
    assert sel.selected == len(selected) and len(set(out)) == len(out) == c.distinct_kmers
    assert len(out) == sel.selected - cleaning.tip_kmers - cleaning.isolated_kmers - bubbles.arm_kmers and set(out) <= selected
    assert int(a.unitig_sums.sum()) == sel.selected_occurrences - cleaning.removed_occurrences - bubbles.removed_occurrences
    assert cleaning.rounds_run >= 1 and (k == 4 or cleaning.removed_kmers + bubbles.arm_kmers > 0)
    if split:  # every unitig has one mask, and no two neighbours could be joined otherwise
        cuts = np.concatenate([[0], np.cumsum([len(u) - k + 1 for u in store.sequences()])])
        assert all(len(set(col.kmer_colors[lo:hi].tolist())) == 1 for lo, hi in zip(cuts[:-1], cuts[1:]))
    else:  # maximal: compacting the output again returns it
        assert compact_ref.compact(store.sequences(), k)[0] == store.sequences()
    # without cleaning the same selection is the restatement's
    want = S.compact_selected(recs, k, 1, colors, 3, **kwargs)
    _assert_equals_ref(api.compact_unitigs_selected(recs, k, _selection(kwargs), record_colors=colors, n_colors=3, kmer_counts=True), want, k, 3)


def test_calls_without_a_selection_are_unchanged_by_one(gpu):
    k = 31
    recs, colors = TC._case(k, 3)
    subtract, intersect, _ = SC.filters(k, recs)

    def others():
        s1, c1, a1, col1, cc1, cl1, b1 = api.compact_unitigs_simplified(recs, k, pop_bubbles=2 * k, clip_tips=k, record_colors=colors, n_colors=3, kmer_counts=True)
        s2, c2 = api.compact_unitigs(recs, k)
        s3, c3, a3, col3 = api.compact_unitigs_colored(recs, k, colors, 3, min_abundance=2)
        arrays = [s1.arrays()[0].tobytes(), s1.arrays()[1].tobytes(), a1.kmer_counts.tobytes(), col1.kmer_colors.tobytes(), col1.shared.tobytes(),
                  cc1.kmer_class.tobytes(), s2.arrays()[0].tobytes(), s3.arrays()[0].tobytes(), col3.occupancy.tobytes(), a3.unitig_sums.tobytes()]
        return arrays, (c1, cl1, b1, c2, c3)

    before = others()
    api.compact_unitigs_selected(recs, k, api.KmerSelection(subtract=subtract, intersect=intersect, forbid=[2]), record_colors=colors, n_colors=3)
    assert others() == before
    t = api.last_compact_times()
    assert t["filter_ms"] == 0 and t["select_ms"] == 0  # the last call had no selection


def test_arguments_are_refused_by_name(gpu):
    recs, colors = TC._case(31, 3)
    for kw, word in (({"require": [0], "forbid": [0]}, "share"), ({"min_colors": 3, "max_colors": 2}, "min_colors"),
                     ({"subtract_min_abundance": 0}, "subtract_min_abundance"), ({"intersect_min_abundance": 0}, "intersect_min_abundance"),
                     ({"max_colors": 65}, "max_colors"), ({"require": [64]}, "require"), ({"filter_records": [("both", "ACGT")]}, "role")):
        with pytest.raises(ValueError, match=word):
            api.KmerSelection(**kw)
    with pytest.raises(ValueError, match="forbid names colour 5 of 3"):
        api.compact_unitigs_selected(recs, 31, api.KmerSelection(forbid=[5]), record_colors=colors, n_colors=3)
    with pytest.raises(ValueError, match="need record_colors"):
        api.compact_unitigs_selected(recs, 31, api.KmerSelection(min_colors=1))
    with pytest.raises(ValueError, match="KmerSelection"):
        api.compact_unitigs_selected(recs, 31, None)
