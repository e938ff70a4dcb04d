"""The restatement of the simplified compaction (bubble_ref.py) on cases whose outcome follows from the definition by
hand, and what the generator of the GPU fuzz must contain. No GPU."""
import random

import pytest

import bubble_ref as B
import compact_ref as R
import tip_clip_ref as T

K = 11
NONE = {"arms": 0, "arm_kmers": 0, "removed_occurrences": 0}


def _dna(rng):
    return lambda n: "".join(rng.choice("ACGT") for _ in range(n))


@pytest.fixture(scope="module")
def cases():
    rng = random.Random(25)
    return B.hand_cases(rng, _dna(rng), K)


def _run(cases, name, **more):
    records, k, kw = cases[name]
    return B.compact_simplified(records, k, **dict(kw, **more))


def _with(g, p, base):
    return g[:p] + base + g[p + 1:]


def test_a_snp_seen_once_is_a_tie_that_the_creator_settles(cases):
    g = cases["_parts"]["g"]
    short = _run(cases, "snp_short_L")  # the arms have k k-mers: not fewer than L = k
    assert short[7] == NONE and short[6]["rounds_run"] == 1 and short[1]["unitigs"] == 4
    tie = _run(cases, "snp_tie")  # means 1 : 1; g is the first record and holds the smaller creators
    assert tie[7] == {"arms": 1, "arm_kmers": K, "removed_occurrences": K}
    assert tie[0] == [g] and tie[6] == {"rounds_run": 1, "tips": 0, "tip_kmers": 0, "isolated": 0, "isolated_kmers": 0, "removed_occurrences": 0}
    assert tie[3]["distinct_kept"] == tie[1]["distinct_kmers"] + K
    again = _run(cases, "snp_tie", rounds=5)
    assert again[0] == [g] and again[6]["rounds_run"] == 2 and again[7] == tie[7]


def test_the_variant_seen_three_times_wins(cases):
    parts = cases["_parts"]
    out = _run(cases, "snp_variant_wins")
    assert out[7] == {"arms": 1, "arm_kmers": K, "removed_occurrences": K}
    assert out[0] == [_with(parts["g"], parts["p"], parts["snp"][K - 1])]


def test_the_ratio_guards_even_coverage(cases):
    assert _run(cases, "ratio2_even")[7] == NONE  # k k >= 2 k k is false
    weak = _run(cases, "ratio2_3to1")  # 3 k k >= 2 k k
    assert weak[7] == {"arms": 1, "arm_kmers": K, "removed_occurrences": K} and weak[0] == [cases["_parts"]["g"]]
    assert _run(cases, "ratio2_3to1", bubble_ratio=3)[7]["arms"] == 1 and _run(cases, "ratio2_3to1", bubble_ratio=4)[7] == NONE


def test_a_deletion_is_decided_by_the_means(cases):
    parts = cases["_parts"]
    g, p = parts["g"], parts["dp"]
    goes = _run(cases, "deletion_goes")  # g's arm: 2 k over k k-mers; the deletion's: k - 1 over k - 1
    assert goes[7] == {"arms": 1, "arm_kmers": K - 1, "removed_occurrences": K - 1} and goes[0] == [g]
    wins = _run(cases, "deletion_wins")  # g's arm: mean 1; the deletion's: mean 2
    assert wins[7] == {"arms": 1, "arm_kmers": K, "removed_occurrences": K} and wins[0] == [g[:p] + g[p + 1:]]


def test_three_alleles_lose_two_arms_in_one_round(cases):
    out = _run(cases, "three_alleles")
    assert out[7] == {"arms": 2, "arm_kmers": 2 * K, "removed_occurrences": 2 * K} and out[0] == [cases["_parts"]["g"]] and out[6]["rounds_run"] == 1


def test_a_long_arm_is_in_no_bundle_and_one_short_arm_stays(cases):
    info = {}
    out = _run(cases, "long_arm", info=info)
    assert out[7] == {"arms": 1, "arm_kmers": K, "removed_occurrences": K} and info["max_bundle"] == 2
    kmers = {R.canonical(u[i:i + K]) for u in out[0] for i in range(len(u) - K + 1)}
    ins, g, p = cases["_parts"]["insertion"], cases["_parts"]["g"], cases["_parts"]["p"]
    assert all(R.canonical(ins[i:i + K]) in kmers for i in range(len(ins) - K + 1))  # the insertion's K + 7 k-mers stay
    assert all(R.canonical(g[i:i + K]) in kmers for i in range(p - K + 1, p + 1))  # and g's arm
    assert out[1]["unitigs"] == 4
    wider = _run(cases, "long_arm", pop_bubbles=K + 8, info=info)  # K + 7 < K + 8: a bundle of three, all of mean 1, and g's arm is the best
    assert info["max_bundle"] == 3 and wider[7] == {"arms": 2, "arm_kmers": 2 * K + 7, "removed_occurrences": 2 * K + 7} and wider[0] == [g]


def test_a_hairpin_is_never_two_arms(cases):
    info = {}
    out = _run(cases, "hairpin", info=info)
    assert out[7] == NONE and info["turned_away"] >= 1
    records, k, _ = cases["hairpin"]
    assert out[0] == R.compact(records, k)[0]


def test_a_ring_with_a_snp_is_a_closed_walk_again(cases):
    parts = cases["_parts"]
    out = _run(cases, "ring_snp")
    assert out[7] == {"arms": 1, "arm_kmers": K, "removed_occurrences": K}
    assert out[0] == R.compact([parts["ring_rec"]], K)[0] and out[2] == [True] and out[1]["closed_walks"] == 1


def test_a_snp_and_a_tip_go_in_one_round_with_separate_counters(cases):
    out = _run(cases, "snp_and_tip")
    assert out[7] == {"arms": 1, "arm_kmers": K, "removed_occurrences": K}
    assert out[6] == {"rounds_run": 1, "tips": 1, "tip_kmers": 4, "isolated": 0, "isolated_kmers": 0, "removed_occurrences": 4}
    assert out[0] == [cases["_parts"]["g"]]


def test_a_bubble_on_a_bubbles_arm_needs_two_rounds(cases):
    g = cases["_parts"]["g"]
    one = _run(cases, "nested_one_round")  # wide's arm is three walks: only the inner SNP (1 against wide's 2) goes
    assert one[7] == {"arms": 1, "arm_kmers": K, "removed_occurrences": K} and one[6]["rounds_run"] == 1 and one[1]["unitigs"] == 4
    two = _run(cases, "nested_two_rounds")  # then wide (2 K - 1 k-mers seen twice) ties with g's arm and g holds the smaller creator
    assert two[7] == {"arms": 2, "arm_kmers": K + 2 * K - 1, "removed_occurrences": K + 2 * (2 * K - 1)}
    assert two[0] == [g] and two[6]["rounds_run"] == 3


def test_without_popping_the_cleaned_restatement_comes_back(cases):
    rng = random.Random(77)
    g = T.genome(rng, 600, K)
    records, _ = T.plant_tips(rng, g, K, 5, _dna(rng))
    records += B.plant_snps(rng, g, K, 4)[0][1:]
    for kw in (dict(clip_tips=K), dict(clip_tips=K, remove_isolated=K, rounds=3, m=1), dict()):
        assert B.compact_simplified(records, K, **kw)[:7] == T.compact_cleaned(records, K, **kw) and B.compact_simplified(records, K, **kw)[7] == NONE


@pytest.mark.parametrize("k", [11, 31, 32])
def test_planted_snps_give_the_genome_back(k):
    rng = random.Random(2000 + k)
    g = T.genome(rng, 3000, k)
    records, sites = B.plant_snps(rng, g, k, 30)
    assert len(records) == 31 and all(b - a >= 2 * k + 2 for a, b in zip(sites, sites[1:]))
    out = B.compact_simplified([g] + records, k, pop_bubbles=2 * k, rounds=2)
    assert out[0] == [g] and out[7] == {"arms": 30, "arm_kmers": 30 * k, "removed_occurrences": 30 * k} and out[6]["rounds_run"] == 2
    assert B.compact_simplified([g] + records, k, pop_bubbles=2 * k, bubble_ratio=3)[7] == NONE  # 2 : 1 does not reach 3


def test_the_fuzz_generator_reaches_what_it_must():
    """The GPU fuzz (test_gpu_pop_bubbles.py) runs these inputs; here the restatement alone says that they pop arms, hold excluded
    loops or hairpins, and hold bundles of three or more arms, so that the GPU test cannot pass vacuously."""
    cases = B.fuzz_cases()
    assert len(cases) == 300 and {k for _, k, _ in cases} == {4, 5, 6}
    popping = hairpins = wide = 0
    for records, k, kw in cases:
        assert 1 <= kw["rounds"] <= 4 and kw["bubble_ratio"] in (1, 2)
        info = {}
        out = B.compact_simplified(records, k, info=info, **kw)
        popping += out[7]["arms"] > 0
        hairpins += info.get("turned_away", 0) > 0
        wide += info.get("max_bundle", 0) >= 3
    assert popping >= 60 and hairpins >= 10 and wide >= 10, (popping, hairpins, wide)
