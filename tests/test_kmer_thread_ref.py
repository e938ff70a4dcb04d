"""The thread contract's restatement (kmer_thread_ref.py) against walks derived by hand at k = 4 -- a Y, a read across stem and branch,
its reverse complement, reads that start and end inside a unitig, an N, an absent k-mer, a ring taken several times round -- and,
on every case list the GPU tests use, against what a walk means (kmer_thread_ref.check): the lists are built so that the
restatement alone meets every property here, on the CPU."""
import pytest

import compact_ref
import kmer_thread_cases as cases
import kmer_thread_ref as TR
from matchtigs_amd import synth


@pytest.mark.parametrize("name,index,k,queries,want", cases.hand_cases(), ids=lambda x: x if isinstance(x, str) else None)
def test_hand_cases(name, index, k, queries, want):
    got = TR.thread(index, queries, k)
    assert got == want
    TR.check(index, queries, k, got, unitigs=True)


def test_the_y_is_what_compaction_makes_of_its_haplotypes():
    unitigs, _, closed = compact_ref.compact(cases.Y_HAPLOTYPES, 4)
    assert sorted(map(synth.canonical, unitigs)) == sorted(map(synth.canonical, cases.Y_INDEX)) and not any(closed)
    ring, _, closed = compact_ref.compact(["AACTGAACTG"], 4)
    assert len(ring) == 1 and closed == [True] and len(ring[0]) == 8 and ring[0] in "AACTGAACTGAACTG"


def test_reverse_complement_reverses_and_flips_the_steps():
    got = TR.thread(cases.Y_INDEX, cases.Y_QUERIES, 4)
    a, b = got["walks"][0], got["walks"][1]
    assert cases.Y_QUERIES[1] == synth.revcomp(cases.Y_QUERIES[0])
    assert [x ^ 1 for x in reversed(got["steps"][a[5]:a[5] + a[4]])] == got["steps"][b[5]:b[5] + b[4]]
    assert a[3] == b[3] and a[6] == b[6] and b[7] == a[6] - a[8]  # the same path read from its other end


def test_min_kmers_and_gaf():
    got = TR.thread(cases.Y_INDEX, cases.Y_QUERIES, 4)
    names, lengths = [f"r{i}" for i in range(len(cases.Y_QUERIES))], [len(q) for q in cases.Y_QUERIES]
    assert TR.gaf(got, names, lengths) == cases.Y_GAF
    assert TR.gaf(got, names, lengths, ["stem", "b1", "b2"]).splitlines()[2].split(b"\t")[5] == b">stem<b2"
    for min_kmers in (2, 3, 6, 7):
        kept = TR.thread(cases.Y_INDEX, cases.Y_QUERIES, 4, min_kmers)
        assert [w[:5] + w[6:] for w in kept["walks"]] == [w[:5] + w[6:] for w in got["walks"] if w[3] >= min_kmers]
        assert {f: kept[f] for f in ("kmers", "valid", "found")} == cases.Y_COUNTS
        TR.check(cases.Y_INDEX, cases.Y_QUERIES, 4, kept, min_kmers, unitigs=True)


@pytest.mark.parametrize("k", [2, 5, 15, 31, 33])
def test_genome_cases_meet_the_properties(k):
    haps, queries = cases.genome_case(k)
    unitigs = compact_ref.compact(haps, k)[0]
    for min_kmers in (1, 2, k):
        got = TR.thread(unitigs, queries, k, min_kmers)
        TR.check(unitigs, queries, k, got, min_kmers, unitigs=True)
    got = TR.thread(unitigs, queries, k)
    for r in (0, 1):  # a haplotype over its own unitigs: one walk from end to end
        assert [w for w in got["walks"] if w[0] == r] == [got["walks"][r]] and got["walks"][r][3] == got["kmers"][r] == len(haps[r]) - k + 1
    assert any(w[4] > 1 for w in got["walks"]) and len(got["walks"]) > len(queries) - 3  # steps are crossed, substitutions break walks
    # over the haplotypes as they are, not compacted: never wrong, only shorter
    TR.check(haps, queries, k, TR.thread(haps, queries, k))


def test_large_case_meets_the_properties():
    genome, k, queries = cases.large_case()
    unitigs = compact_ref.compact(genome, k)[0]
    assert len({synth.canonical(u[i:i + k]) for u in unitigs for i in range(len(u) - k + 1)}) == 512  # every 5-mer
    got = TR.thread(unitigs, queries, k)
    TR.check(unitigs, queries, k, got, unitigs=True)
    long_walks = [w for w in got["walks"] if w[0] == 1500]
    assert len(long_walks) == 1 and long_walks[0][4] > 4 * 2048 and len(got["walks"]) > 2 * 2048
