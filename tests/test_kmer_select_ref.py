"""The restatement of the k-mer selection (kmer_select_ref.py) against the older restatements and against cases derived
by hand at k = 4; no GPU. Every case list of test_gpu_kmer_select.py runs through the restatement's own assertions here."""
import pytest

import abundance_ref as A
import kmer_color_ref as KC
import kmer_select_cases as SC
import kmer_select_ref as S
import test_gpu_kmer_color as TC
from matchtigs_amd import synth


@pytest.mark.parametrize("m", [1, 2])
def test_the_trivial_selection_is_the_coloured_compaction(m):
    recs, colors = TC._case(4, 3)
    unitigs, stats, closed, ab, col = KC.compact_colored(recs, colors, 3, 4, m)
    got = S.compact_selected(recs, 4, m, colors, 3)
    assert got["unitigs"] == unitigs and got["stats"] == stats and got["closed"] == closed and got["colours"] == col
    for f in ("distinct_all", "distinct_kept", "max_abundance", "kept_occurrences", "spectrum", "unitig_sums"):
        assert got["abundance"][f] == ab[f], f
    sel = got["selection"]
    assert sel["selected"] == sel["input_kmers"] == ab["distinct_kept"] and sel["selected_occurrences"] == ab["kept_occurrences"]
    assert sel["per_color_selected"] == col["per_color"] and all(sel["rejected_" + r] == 0 for r in S.RULES)
    # ... and without colours the counted one
    plain = S.compact_selected(recs, 4, m)
    assert (plain["unitigs"], plain["stats"], plain["closed"]) == A.compact_counted(recs, 4, m)[:3] and plain["colours"] is None


# k = 4, by hand. AAACAAGC: the windows AAAC, AACA, ACAA, CAAG, AAGC (all canonical as read, none a palindrome, no (k-1)-mer twice on
# either strand) spell one unitig.
MAIN = ["AAACAAGC"]


def test_subtracting_the_middle_of_a_unitig_gives_two():
    assert S.compact_selected(MAIN, 4)["unitigs"] == MAIN
    got = S.compact_selected(MAIN, 4, subtract=["ACAA"])
    assert got["unitigs"] == ["AAACA", "CAAGC"] and got["selection"]["rejected_subtract"] == 1 and got["selection"]["selected"] == 4
    assert got["selection"]["subtract_windows"] == 1 and got["selection"]["subtract_hits"] == 1
    assert got["abundance"]["distinct_kept"] == 5 and got["stats"]["distinct_kmers"] == 4  # the abundance's fields stay over S_m


def test_a_subtract_record_as_the_reverse_complement_and_in_lower_case():
    assert synth.revcomp("ACAA") == "TTGT"
    assert S.compact_selected(MAIN, 4, subtract=["ttgt"])["unitigs"] == ["AAACA", "CAAGC"]


def test_a_palindromic_filter_window_counts_once():
    # ACGT is its own reverse complement: one window, sub = 1; A = 2 keeps it
    main = ["AACGTC"]  # AACG ACGT CGTC
    assert S.filter_counts(["ACGT"], 4) == {"ACGT": 1}
    assert S.compact_selected(main, 4, subtract=["ACGT"], A_=2)["selection"]["rejected_subtract"] == 0
    assert S.compact_selected(main, 4, subtract=["ACGT"], A_=1)["selection"]["rejected_subtract"] == 1
    assert S.compact_selected(main, 4, subtract=["ACGT", "acgt"], A_=2)["selection"]["rejected_subtract"] == 1


def test_A_2_keeps_a_kmer_the_filter_shows_once():
    got = S.compact_selected(MAIN, 4, subtract=["ACAA", "AAAC", "GTTT"], A_=2)  # GTTT = rc(AAAC): AAAC twice, ACAA once
    assert got["selection"]["rejected_subtract"] == 1 and "AAAC" not in got["selected_set"] and "ACAA" in got["selected_set"]
    assert got["selection"]["subtract_windows"] == 3 and got["selection"]["subtract_hits"] == 3 and got["unitigs"] == ["AACAAGC"]


def test_intersect_with_B_2():
    panel = ["AAACA", "TGTTT", "CAAG"]  # AAAC and AACA twice (TGTT = rc(AACA), GTTT = rc(AAAC)), CAAG once
    got = S.compact_selected(MAIN, 4, intersect=panel, B=2)
    assert got["selected_set"] == {"AAAC", "AACA"} and got["unitigs"] == ["AAACA"] and got["selection"]["rejected_intersect"] == 3
    assert got["selection"]["intersect_windows"] == 5 and got["selection"]["intersect_hits"] == 5
    assert S.compact_selected(MAIN, 4, intersect=panel, B=1)["selected_set"] == {"AAAC", "AACA", "CAAG"}


def test_forbid_is_counted_before_require():
    recs, colors = ["AAACA", "CAAGC", "AAACA"], [0, 1, 2]  # AAAC, AACA: colours 0 and 2; CAAG, AAGC: colour 1
    got = S.compact_selected(recs, 4, 1, colors, 3, forbid=0b001, require=0b010)  # AAAC and AACA fail both: counted under forbid
    assert got["selection"]["rejected_forbid"] == 2 and got["selection"]["rejected_require"] == 0 and got["selection"]["selected"] == 2
    got = S.compact_selected(recs, 4, 1, colors, 3, forbid=0b010, require=0b100)
    assert got["selection"]["rejected_forbid"] == 2 and got["selection"]["selected"] == 2 and got["selection"]["per_color_selected"] == [2, 0, 2]
    got = S.compact_selected(recs, 4, 1, colors, 3, require=0b100)
    assert got["selection"]["rejected_require"] == 2 and got["selection"]["rejected_forbid"] == 0


def test_min_colors_C_is_the_core():
    recs, colors = TC._case(4, 3)
    got = S.compact_selected(recs, 4, 1, colors, 3, min_colors=2)  # (colour 1 has no window: the core of the two that have)
    assert got["selection"]["selected"] == sum(got["colours"]["occupancy"][2:]) > 0
    recs, colors = ["AAACAAG", "AACAAGC", "ACAAGC"], [0, 1, 2]  # all three carry ACAA and CAAG
    got = S.compact_selected(recs, 4, 1, colors, 3, min_colors=3)
    assert got["selection"]["selected"] == got["colours"]["occupancy"][3] == 2 and got["unitigs"] == ["ACAAG"]
    assert got["selection"]["rejected_carriers"] == got["selection"]["input_kmers"] - 2 == 3


def test_a_filter_record_shorter_than_k():
    got = S.compact_selected(MAIN, 4, subtract=["ACA", "", "N"])
    assert got["unitigs"] == MAIN and got["selection"]["subtract_windows"] == 0 and got["selection"]["rejected_subtract"] == 0
    got = S.compact_selected(MAIN, 4, intersect=["ACA"])  # a record is given: the rule applies, and nothing is in it
    assert got["unitigs"] == [] and got["selection"]["rejected_intersect"] == 5 and got["stats"]["distinct_kmers"] == 0
    assert S.compact_selected(MAIN, 4, intersect=["N", ""])["unitigs"] == MAIN  # no record: no rule


def test_arguments_that_are_refused():
    for kw in ({"require": 1, "forbid": 1}, {"min_colors": 3, "max_colors": 2}, {"A_": 0}, {"B": 0}, {"require": 8}, {"max_colors": 65}):
        with pytest.raises(ValueError):
            S.compact_selected(["AAACC"], 4, 1, [0], 3, **kw)
    with pytest.raises(ValueError):
        S.compact_selected(["AAACC"], 4, min_colors=1)  # a colour rule without colours


def test_selection_lines():
    recs, colors = ["AAACA", "CAAGC", "AAACA"], [0, 1, 2]
    got = S.compact_selected(recs, 4, 1, colors, 3, forbid=0b010)
    lines = S.selection_lines(["a.fa", "b.fa", "c.fa"], got["colours"], dict(got["selection"], distinct_all=got["abundance"]["distinct_all"]))
    assert lines == ["input\t4", "abundance_kept\t4", "forbid\t2", "require\t0", "carriers\t0", "subtract\t0", "intersect\t0", "selected\t2",
                     "color\ta.fa\t2\t2", "color\tb.fa\t2\t0", "color\tc.fa\t2\t2"]


def _holds(out, k, recs):
    sel = out["selection"]
    assert sum(sel["rejected_" + r] for r in S.RULES) + sel["selected"] == sel["input_kmers"] == out["abundance"]["distinct_kept"]
    assert sel["selected"] == out["stats"]["distinct_kmers"] == len(out["abundance"]["kmer_counts"])
    assert sum(out["abundance"]["unitig_sums"]) == sel["selected_occurrences"] <= out["abundance"]["kept_occurrences"]
    assert sel["subtract_hits"] <= sel["subtract_windows"] and sel["intersect_hits"] <= sel["intersect_windows"]


@pytest.mark.parametrize("k,C,m,name", SC.grid(), ids=lambda v: str(v))
def test_the_gpu_cases_through_the_restatement(k, C, m, name):
    recs, colors, kwargs, _ = SC.case(k, C, name)
    out = S.compact_selected(recs, k, m, colors, C, **kwargs)
    _holds(out, k, recs)
    sel = out["selection"]
    if name == "trivial" or name == "empty-filter" or name == "no-hit":
        assert sel["selected"] == sel["input_kmers"] > 0
    elif name == "everything-rejected":
        assert sel["selected"] == 0 and sel["rejected_intersect"] == sel["input_kmers"] > 0 and out["unitigs"] == []
    elif name == "all-five" and C == 64 and m == 1 and k > 4:
        assert sum(sel["rejected_" + r] > 0 for r in S.RULES) >= 3 and sel["selected"] > 0, sel  # several rules reject, in their order
    elif k == 4 and name in ("forbid", "all-five"):  # (at k = 4 nearly every k-mer is in every colour)
        assert sel["selected"] < sel["input_kmers"], sel
    elif name.startswith(("subtract", "intersect", "carriers", "alternating")) or C > 1:
        assert 0 < sel["selected"] < sel["input_kmers"], sel
    if name == "alternating":
        assert sel["rejected_subtract"] > 0 and sel["rejected_intersect"] > 0


def test_the_abundance_thresholds_of_the_grid_differ():
    """A = 1, 2, 3 and B = 1, 2 select different sets: the filter shows k-mers once, twice and three times."""
    for k in SC.KS:
        recs, colors = TC._case(k, 3)
        subtract, intersect, _ = SC.filters(k, recs)
        by_a = [S.compact_selected(recs, k, subtract=subtract, A_=a)["selection"]["rejected_subtract"] for a in (1, 2, 3, 4)]
        assert by_a[0] > by_a[1] > by_a[2] > 0, (k, by_a)
        by_b = [S.compact_selected(recs, k, intersect=intersect, B=b)["selection"]["rejected_intersect"] for b in (1, 2)]
        assert 0 < by_b[0] < by_b[1], (k, by_b)


def test_the_collision_and_size_cases():
    k, main, other = SC.collision_case()
    assert S.compact_selected([main], k, subtract=[other])["selection"]["subtract_hits"] == 0
    assert S.compact_selected([main], k, subtract=[main])["selection"]["selected"] == 0
    for k in SC.SIZE_KS:
        recs, colors, subtract, intersect = SC.size_case(k)
        out = S.compact_selected(recs, k, 2, colors, 3, subtract=subtract, A_=3, intersect=intersect, min_colors=2)
        _holds(out, k, recs)
        assert sum(len(s) for s in subtract + intersect) // 64 > 4 * 256  # the filter's positions: more than four workgroups of threads
        if k == 9:
            assert out["selection"]["input_kmers"] > out["selection"]["selected"] > 2048
