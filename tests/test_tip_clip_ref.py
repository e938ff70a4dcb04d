"""The restatement of the cleaned compaction (tip_clip_ref.py) on cases whose outcome follows from the definition by
hand. No GPU."""
import random

import pytest

import compact_ref as R
import tip_clip_ref as T


def _dna(rng):
    return lambda n: "".join(rng.choice("ACGT") for _ in range(n))


@pytest.fixture(scope="module")
def cases():
    rng = random.Random(24)
    return T.hand_cases(rng, _dna(rng))


def _run(cases, name):
    records, k, kw = cases[name]
    return T.compact_cleaned(records, k, **kw)


@pytest.mark.parametrize("k", [11, 21, 31, 32, 40])
def test_planted_tips_give_the_genome_back(k):
    rng = random.Random(1000 + k)
    dna = _dna(rng)
    g = T.genome(rng, 3000, k)
    records, planted = T.plant_tips(rng, g, k, 40, dna)
    want = R.compact([g], k)
    one = T.compact_cleaned(records, k, clip_tips=k, rounds=1)
    assert one[0] == want[0] and one[2] == want[2]
    assert one[6] == {"rounds_run": 1, "tips": 40, "tip_kmers": planted, "isolated": 0, "isolated_kmers": 0,
                      "removed_occurrences": planted}
    assert one[1]["distinct_kmers"] == want[1]["distinct_kmers"] and one[3]["distinct_kept"] == want[1]["distinct_kmers"] + planted
    two = T.compact_cleaned(records, k, clip_tips=k, rounds=2)
    assert two[0] == want[0] and two[6] == dict(one[6], rounds_run=2)
    untouched = T.compact_cleaned(records, k)
    assert untouched[1]["unitigs"] > want[1]["unitigs"] and untouched[6]["rounds_run"] == 0


def test_a_tip_of_six_kmers_stays_at_six_and_goes_at_seven(cases):
    g = cases["_parts"]["g"]
    stays, goes = _run(cases, "tip6_stays"), _run(cases, "tip6_goes")
    assert stays[6]["tips"] == 0 and stays[6]["rounds_run"] == 1 and stays[1]["unitigs"] == 3
    assert goes[6]["tips"] == 1 and goes[6]["tip_kmers"] == 6 and goes[0] == R.compact([g], 11)[0] == [g]


def test_a_y_loses_its_twigs_first_and_its_stem_in_the_next_round(cases):
    p = cases["_parts"]
    one = _run(cases, "y_one_round")
    assert one[6] == {"rounds_run": 1, "tips": 2, "tip_kmers": 7, "isolated": 0, "isolated_kmers": 0, "removed_occurrences": 7}
    assert one[0] == T.compact_cleaned([p["g"], p["stem"]], 11)[0] and len(one[0]) == 3
    two = _run(cases, "y_two_rounds")
    assert two[6] == {"rounds_run": 2, "tips": 3, "tip_kmers": 12, "isolated": 0, "isolated_kmers": 0, "removed_occurrences": 12}
    assert two[0] == [p["g"]]
    many = _run(cases, "y_many_rounds")
    assert many[0] == [p["g"]] and many[6] == dict(two[6], rounds_run=3)


def test_an_isolated_record_goes_below_the_length_and_stays_at_it(cases):
    g = cases["_parts"]["g"]
    goes, stays = _run(cases, "isolated_goes"), _run(cases, "isolated_stays")
    assert goes[0] == [g] and goes[6]["isolated"] == 1 and goes[6]["isolated_kmers"] == 4 and goes[6]["tips"] == 0
    assert len(stays[0]) == 2 and stays[6]["isolated"] == 0


@pytest.mark.parametrize("name", ["stem_kept", "merge_kept"])
def test_the_stem_of_a_fork_and_the_continuation_of_a_merge_are_protected(cases, name):
    records, k, _ = cases[name]
    got = _run(cases, name)
    assert got[0] == R.compact(records, k)[0] and len(got[0]) == 3 and min(len(u) - k + 1 for u in got[0]) == 3
    assert got[6] == {"rounds_run": 1, "tips": 0, "tip_kmers": 0, "isolated": 0, "isolated_kmers": 0, "removed_occurrences": 0}


def test_a_lone_palindromic_kmer_is_anchored_on_both_sides(cases):
    walks, out, into = T.walks_over({"ACGT": "ACGT"})
    assert [T.walk_ends({"ACGT": "ACGT"}, w, out, into) for w, _ in walks] == [(T.ANCHORED, T.ANCHORED)] * 2
    got = _run(cases, "lone_palindrome")
    assert got[0] == ["ACGT"] and got[6]["tips"] == got[6]["isolated"] == 0


def test_a_ring_with_a_tip_closes_again(cases):
    ring_rec = cases["_parts"]["ring_rec"]
    records, k, _ = cases["ring_tip"]
    before = T.compact_cleaned(records, k)
    assert before[1]["closed_walks"] == 0 and before[1]["unitigs"] == 2
    got = _run(cases, "ring_tip")
    want = R.compact([ring_rec], k)
    assert got[0] == want[0] and got[2] == [True] and got[6]["tips"] == 1 and got[6]["tip_kmers"] == 4


def test_end_states_at_a_self_mirror_node():
    # k = 5: the node ACGT is its own mirror. One k-mer that ends in it has a free end there; with a second one both are anchored.
    reading = {R.canonical("GACGT"): "GACGT"}
    walks, out, into = T.walks_over(reading)
    (w,) = [w for w, _ in walks if R.edge_string(reading, w[-1]) == "GACGT"]
    assert T.walk_ends(reading, w, out, into) == (T.FREE, T.FREE)
    reading[R.canonical("CACGT")] = "CACGT"
    walks, out, into = T.walks_over(reading)
    for w, _ in walks:
        if R.edge_string(reading, w[-1]).endswith("ACGT"):
            assert T.walk_ends(reading, w, out, into) == (T.ANCHORED, T.FREE)


def test_bad_arguments():
    for kw in (dict(rounds=0), dict(rounds=65), dict(split=True), dict(m=0)):
        with pytest.raises(ValueError):
            T.compact_cleaned(["ACGTACGT"], 3, **kw)
