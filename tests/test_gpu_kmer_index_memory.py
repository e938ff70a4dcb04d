"""A k-mer index and its probe calls give back to the device arena what they took (api.device_arena_stats: live_bytes): build and
free of a plain, a locating, a weighted, a coloured and a weighted-and-coloured index; on live indexes one query with and one without
the bit arrays, one locate call with runs and one with none, one abundance and one colour call with and without per_window, a query
with no bases; and an index with no windows. k = 5 and k = 34: the narrow and the wide table, the index without and with its packed
bases. Every call is warmed once (test_gpu_compact_memory.py's _gives_back) and holds its answer to the restatement that the test
of that call compares it with (test_gpu_kmer_query.py, _locate, _abundance, _color)."""
import random

import pytest

import kmer_abundance_ref as A
import kmer_color_ref as C
import kmer_locate_ref as L
import kmer_query_ref as Q
from matchtigs_amd import api
from test_gpu_compact_memory import _gives_back

pytestmark = pytest.mark.gpu
KS = [5, 34]
N_COLORS = 3
KINDS = {  # what the index is built with beside the records
    "plain": dict(),
    "locating": dict(locate=True),
    "weighted": dict(weights=True),
    "coloured": dict(colors=True),
    "weighted-and-coloured": dict(weights=True, colors=True),
}


@pytest.fixture(scope="module")
def gpu(product_lib):
    import torch

    if product_lib.mtg_device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("these tests need a GPU: the k-mer index has no CPU path")
    return torch


def _case(k):
    """Five index records of about a hundred bases and one shorter than k; a query that shares stretches with them, with an N, a random
    record and one shorter than k; one weight and one colour mask per index window. The restatements' answers are computed here, once."""
    rng = random.Random(4100 + k)
    dna = lambda n: "".join(rng.choices("ACGT", k=n))
    index = [dna(rng.randint(90, 120)) for _ in range(5)] + [dna(k - 1)]
    query = [index[0][10:70] + "N" + index[2][5:60], dna(100), dna(k - 1), index[4][::-1], index[1][20:20 + 2 * k]]
    windows = sum(max(0, len(s) - k + 1) for s in index)
    weights = [rng.choice([0, 1, 7, 0xFFFFFFFF, rng.getrandbits(32)]) for _ in range(windows)]
    masks = [rng.getrandbits(N_COLORS) for _ in range(windows)]
    want = dict(query=Q.query(Q.index_set(index, k), query, k), locate=L.locate(index, query, k), abundance=A.abundance(index, weights, query, k),
                colors=C.color_hits(index, masks, N_COLORS, query, k))
    assert want["locate"]["runs"] and 0 < sum(want["query"]["found"]) < sum(want["query"]["valid"])
    return dict(k=k, index=index, query=query, weights=weights, masks=masks, want=want)


@pytest.fixture(scope="module", params=KS, ids=lambda k: f"k{k}")
def case(request):
    return _case(request.param)


def _build(case, locate=False, weights=False, colors=False, records=None):
    return api.KmerIndex(case["index"] if records is None else records, case["k"], locate=locate, weights=case["weights"] if weights else None,
                         colors=case["masks"] if colors else None, n_colors=N_COLORS if colors else None)


def _check_query(ix, query, want, bits):
    got = ix.query(query, bits=bits)
    for f in ("kmers", "valid", "found") + (("valid_bits", "present_bits") if bits else ()):
        assert getattr(got, f).tolist() == want[f], f
    if not bits:
        assert got.valid_bits is None and got.present_bits is None


def _check_locate(ix, query, want):
    got = ix.locate(query)
    for f in ("kmers", "valid", "found"):
        assert getattr(got, f).tolist() == want[f], f
    assert [tuple(int(x) for x in row) for row in got.runs[list(L.FIELDS)].tolist()] == want["runs"]


def _check_abundance(ix, query, want, per_window):
    got = ix.abundance(query, per_window=per_window)
    for f in ("kmers", "valid", "found", "sum", "min", "max"):
        assert getattr(got, f).tolist() == want[f], f
    assert (got.per_window.tolist() == want["per_window"]) if per_window else got.per_window is None


def _check_colors(ix, query, want, per_window):
    got = ix.color_hits(query, per_window=per_window)
    for f in ("kmers", "valid", "found", "per_color"):
        assert getattr(got, f).tolist() == want[f], f
    assert (got.per_window.tolist() == want["per_window"]) if per_window else got.per_window is None


@pytest.mark.parametrize("kind", KINDS)
def test_build_and_free(gpu, case, kind):
    def check():
        with _build(case, **KINDS[kind]) as ix:
            assert ix.info.device_bytes > 0
            _check_query(ix, case["query"], case["want"]["query"], False)

    _gives_back(lambda: _build(case, **KINDS[kind]).close(), check)


def test_the_probe_calls(gpu, case):
    query, want = case["query"], case["want"]
    no_runs = ["N" * 50, "n" * (case["k"] + 3)]  # bases, but no valid window: the locate call's exit without runs
    want_none = L.locate(case["index"], no_runs, case["k"])
    assert want_none["runs"] == [] and sum(want_none["valid"]) == 0
    with _build(case, locate=True, weights=True, colors=True) as ix:
        for bits in (True, False):
            _gives_back(lambda: ix.query(query, bits=bits), lambda: _check_query(ix, query, want["query"], bits))
        _gives_back(lambda: ix.locate(query), lambda: _check_locate(ix, query, want["locate"]))
        _gives_back(lambda: ix.locate(no_runs), lambda: _check_locate(ix, no_runs, want_none))
        for per_window in (True, False):
            _gives_back(lambda: ix.abundance(query, per_window=per_window), lambda: _check_abundance(ix, query, want["abundance"], per_window))
            _gives_back(lambda: ix.color_hits(query, per_window=per_window), lambda: _check_colors(ix, query, want["colors"], per_window))
        for empty in ([], ["", ""]):  # a query with no bases: no device call at all
            _gives_back(lambda: ix.query(empty, bits=True), lambda: _check_query(ix, empty, Q.query(set(), empty, case["k"]), True))


def test_an_index_with_no_windows(gpu, case):
    k, query = case["k"], case["query"]
    short = [s[:k - 1] for s in case["index"]]
    want = Q.query(set(), query, k)
    assert sum(want["valid"]) > 0 and sum(want["found"]) == 0

    def check():
        with api.KmerIndex(short, k, locate=True, weights=[], colors=[], n_colors=N_COLORS) as ix:
            assert ix.info.occurrences == 0 and ix.info.distinct == 0
            _check_query(ix, query, want, True)
            assert len(ix.locate(query).runs) == 0

    _gives_back(lambda: api.KmerIndex(short, k, locate=True, weights=[], colors=[], n_colors=N_COLORS).close(), check)
