"""Threading on the GPU (kmer_walks_device.hpp, api.KmerIndex.thread / api.TigIndex.thread): the counts, the walks and
the steps field for field against the contract's restatement (kmer_thread_ref.py, which steps window by window over strings and
knows no runs), the table index and the sparse index against each other for every m and bucket_limit tried, and the library's own
output held to what a walk means (kmer_thread_ref.check) without the restatement: paths that spell the query, steps that overlap,
walks that ascend and cannot be joined, one walk per stretch of found windows over unitigs. locate() answers as before a call."""
import numpy as np
import pytest

import kmer_thread_cases as cases
import kmer_thread_ref as TR
from matchtigs_amd import api, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(product_lib):
    import torch

    if product_lib.mtg_device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("these tests need a GPU: threading has no CPU path")
    return torch


def _as_ref(result):
    """A KmerThreadResult in the restatement's form."""
    assert result.walks.dtype == api.KMER_WALK_DTYPE and result.steps.dtype == np.uint64
    return {"kmers": result.kmers.tolist(), "valid": result.valid.tolist(), "found": result.found.tolist(),
            "walks": [tuple(int(x) for x in row) for row in result.walks[list(TR.FIELDS)].tolist()], "steps": result.steps.tolist()}


def _sparse_settings(k):
    """(m, bucket_limit): the defaults, a short minimizer with every bucket heavy, the longest minimizer"""
    return [(None, None), (min(k, 3), 1), (min(k, 31), 2)] if k > 3 else [(None, None), (1, 1)]


def _assert_threads(index, queries, k, min_kmers=1, want=None, unitigs=False, what=""):
    """Both indexes over `index`: the restatement's result from each, the properties on the library's own output, locate() untouched."""
    want = TR.thread(index, queries, k, min_kmers) if want is None else want
    with api.KmerIndex(index, k, locate=True) as table:
        before = table.locate(queries)
        result = table.thread(queries, min_kmers)
        got = _as_ref(result)
        for f in ("kmers", "valid", "found", "steps", "walks"):
            assert got[f] == want[f], (what, k, min_kmers, f, got[f][:6], want[f][:6])
        TR.check(index, queries, k, got, min_kmers, unitigs)
        after = table.locate(queries)
        for f in ("offsets", "kmers", "valid", "found", "runs"):
            assert getattr(before, f).tobytes() == getattr(after, f).tobytes(), f
        assert int(before.runs["kmers"].sum()) == sum(want["found"])
    for m, limit in _sparse_settings(k):
        with api.TigIndex(index, k, m, bucket_limit=limit, locate=True) as sparse:
            other = sparse.thread(queries, min_kmers)
            for f in ("offsets", "kmers", "valid", "found", "walks", "steps"):
                assert getattr(other, f).tobytes() == getattr(result, f).tobytes(), (what, k, m, limit, f)
            assert sparse.locate(queries).runs.tobytes() == before.runs.tobytes()
    return result


@pytest.mark.parametrize("name,index,k,queries,want", cases.hand_cases(), ids=lambda x: x if isinstance(x, str) else None)
def test_hand_cases(gpu, name, index, k, queries, want):
    result = _assert_threads(index, queries, k, want=want, unitigs=True, what=name)
    if name == "Y":
        names = [f"r{i}" for i in range(len(queries))]
        assert result.gaf(names) == cases.Y_GAF == TR.gaf(want, names, [len(q) for q in queries])
        assert result.gaf(names, ["stem", "b1", "b2"]) == TR.gaf(want, names, [len(q) for q in queries], ["stem", "b1", "b2"])
        assert result.gaf(names, query_lengths=[100] * len(names)) == TR.gaf(want, names, [100] * len(names))
        with pytest.raises(ValueError):
            result.gaf(names[:-1])
        with pytest.raises(ValueError):
            result.gaf(names, ["stem", "b1"])
    for min_kmers in (2, 4, 6, 7):
        _assert_threads(index, queries, k, min_kmers, unitigs=True, what=name)


@pytest.mark.parametrize("k", [2, 5, 15, 31, 33])
def test_genomes(gpu, k):
    """Two haplotypes of 2 kb compacted on the GPU; the haplotypes and reads of them from both strands, with substitutions and Ns,
    empty records and records shorter than k. 33 takes the probes' path beyond 31, 5 gives many tiny unitigs and repeats."""
    haps, queries = cases.genome_case(k)
    store, _ = api.compact_unitigs(haps, k)
    unitigs = store.sequences()
    for min_kmers in (1, 2, k):
        result = _assert_threads(unitigs, queries, k, min_kmers, unitigs=True, what=f"genome min_kmers={min_kmers}")
        if min_kmers == 1:
            walks = result.walks
            assert walks["q_record"][:2].tolist() == [0, 1] and walks["kmers"][:2].tolist() == [len(h) - k + 1 for h in haps]
            assert int(walks["steps"].max()) > 1 and set((result.steps & np.uint64(1)).tolist()) == {0, 1}
    # the same queries over the haplotypes as they are: repeats between them shorten walks, nothing else
    _assert_threads(haps, queries, k, what="not compacted")


def test_empty_and_short(gpu):
    index = cases.Y_INDEX
    for queries in ([], [""], ["", "AC", "ACC"], ["NNNNNNNN"], ["TTTTTTTT"]):
        result = _assert_threads(index, queries, 4, what=str(queries))
        assert len(result.walks) == 0 and len(result.steps) == 0 and result.gaf([f"r{i}" for i in range(len(queries))]) == b""
    for empty_index in ([], ["", "ACC"]):
        _assert_threads(empty_index, cases.Y_QUERIES, 4, what="an index without windows")
    # k = 1, where a window is a base, W(u) the record's length and steps overlap in no base: AC forwards and then backwards as GT;
    # CA leaves the record at its end and enters it again at its start
    result = _assert_threads(["AC", "G"], ["ACGT", "CA"], 1, what="k = 1")
    assert _as_ref(result)["walks"] == [(0, 0, 4, 4, 2, 0, 4, 0, 4), (1, 0, 2, 2, 2, 2, 4, 1, 3)] and result.steps.tolist() == [0, 1, 0, 0]
    with api.KmerIndex(index, 4) as plain, api.TigIndex(index, 4) as sparse:
        for ix in (plain, sparse):
            with pytest.raises(ValueError) as e:
                ix.thread(cases.Y_QUERIES)
            assert "locate=True" in str(e.value)
    t, s = api.last_kmer_thread_times(), api.last_kmer_thread_times(tig=True)
    assert set(t) == set(s) == {"upload_ms", "pack_ms", "probe_ms", "runs_ms", "walks_ms"} and all(v >= 0 for v in (*t.values(), *s.values()))


def test_runs_and_walks_beyond_one_scan_tile(gpu):
    """200 kb at k = 5 over unitigs of one or two windows: more than 2 048 runs, walks, kept walks and steps, so every scan of the
    stage carries block sums over several tiles (hu::SCAN_CHUNK = 2 048), and record 1 500 is one walk of tens of thousands of steps."""
    genome, k, queries = cases.large_case()
    store, _ = api.compact_unitigs(genome, k)
    unitigs = store.sequences()
    want = TR.thread(unitigs, queries, k)
    result = _assert_threads(unitigs, queries, k, want=want, unitigs=True, what="large")
    long_walk = result.walks[result.walks["q_record"] == 1500]
    assert len(long_walk) == 1 and int(long_walk["steps"][0]) > 4 * 2048 and len(result.walks) > 2 * 2048
    assert int(long_walk["kmers"][0]) == 100_000 - k + 1 and int(long_walk["q_end"][0]) == 100_000
    names = [f"read{i}" for i in range(len(queries))]
    assert result.gaf(names) == TR.gaf(want, names, [len(q) for q in queries])
    kept = _assert_threads(unitigs, queries, k, 12, unitigs=True, what="large, min_kmers = 12")
    assert 2048 < len(kept.walks) < len(result.walks)
    t = api.last_kmer_thread_times()
    assert t["probe_ms"] > 0 and t["runs_ms"] > 0 and t["walks_ms"] > 0
