"""Every k-mer stage on the GPU on inputs whose k-mers collide in all 64 bits of the window hash (collision_cases.py): same home slot,
same tag, every pre-filter passes, and only kw::same_class can tell the two classes apart. The set comparison, the plain, counted,
coloured and class compactions, the k-mer index with query, locate, abundance and color_hits, the plain-FASTA join and one pass
through the product, each against its restatement, as exact integers; every call twice with identical results.
test_collision_cases.py shows on the CPU that the cases collide whatever the hash's odd base is, and shares the expectations."""
import dataclasses
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import collision_cases as CC
import compact_ref
import fasta_in_ref as FA
import test_collision_cases as T
from matchtigs_amd import api, synth
from test_gpu_color_split import _assert_classes
from test_gpu_fasta_in import _assert_graph
from test_gpu_kmer_abundance import _assert_equals_ref as _assert_abundance
from test_gpu_kmer_color import _assert_colors_equal_ref, _assert_hits_equal_ref
from test_gpu_kmer_locate import _runs

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CASES = CC.cases()
NONE = 2 ** 64 - 1


@pytest.fixture(scope="module")
def gpu(product_lib):
    import torch

    if product_lib.mtg_device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("these tests need a GPU: the k-mer stages have no CPU path")
    return torch


def _store(result):
    data, off = result[0].arrays()
    return data.tobytes().decode(), [int(x) for x in off]


def _assert_store(result, unitigs, stats):
    """Bytes, offsets and statistics of a compaction call against the restatement's."""
    data, off = _store(result)
    assert dataclasses.asdict(result[1]) == stats
    assert off == [0] + [int(x) for x in np.cumsum([len(u) for u in unitigs])]
    assert data == "".join(unitigs)


@pytest.mark.parametrize("k", CC.KS)
@pytest.mark.parametrize("name", ["pair", "strand"])
def test_compare_kmer_sets(gpu, name, k):
    x, y = CASES[name]
    for both, (a, b) in ((False, ([x], [y])), (True, ([x, y], [y, x]))):
        want = T.compared(name, k, both)
        runs = [dataclasses.asdict(api.compare_kmer_sets(a, b, k)) for _ in range(2)]
        assert runs[0] == want, {f: (runs[0][f], want[f]) for f in want if runs[0][f] != want[f]}
        assert runs[1] == runs[0]
        c = api.KmerComparison(**runs[0])
        if both:
            assert c.equal and c.common == c.distinct_a and c.first_only_in_a_record == c.first_only_in_b_record == NONE
        else:
            assert c.common == 0 and not c.equal and c.only_in_a == c.distinct_a == len(x) - k + 1
            assert (c.first_only_in_a_record, c.first_only_in_a_pos, c.first_only_in_b_record, c.first_only_in_b_pos) == (0, 0, 0, 0)


@pytest.mark.parametrize("name,k", T.WINDOW_CASES + [("nodes", CC.K_NODES)])
def test_compact_unitigs(gpu, name, k):
    unitigs, stats, _ = T.compacted(name, k)
    runs = [api.compact_unitigs(CASES[name], k) for _ in range(2)]
    _assert_store(runs[0], unitigs, stats)
    assert _store(runs[1]) == _store(runs[0]) and runs[1][1] == runs[0][1]
    assert runs[0][1].distinct_kmers == runs[0][1].windows  # no two windows merged
    assert runs[0][1].unitigs == (1 if name == "one_record" else 2)


@pytest.mark.parametrize("m", [1, 2])
@pytest.mark.parametrize("k", CC.KS)
def test_compact_unitigs_counted(gpu, k, m):
    x, y = CASES["pair"]
    W = len(x) - k + 1
    unitigs, stats, _, ab, counts = T.counted(k, m)
    runs = [api.compact_unitigs_counted([x, y, y], k, m, kmer_counts=True) for _ in range(2)]
    _assert_store(runs[0], unitigs, stats)
    a = runs[0][2]
    got = {"distinct_all": a.distinct_all, "distinct_kept": a.distinct_kept, "dropped": a.dropped, "max_abundance": a.max_abundance,
           "kept_occurrences": a.kept_occurrences, "spectrum": a.spectrum.tolist(), "unitig_sums": a.unitig_sums.tolist()}
    assert got == ab
    assert a.kmer_counts.dtype == np.uint32 and a.kmer_counts.tolist() == counts == ([1] * W + [2] * W if m == 1 else [2] * W)  # never 3
    assert a.max_abundance == 2 and a.spectrum[3] == 0
    b = runs[1][2]
    assert _store(runs[1]) == _store(runs[0]) and runs[1][1] == runs[0][1] and np.array_equal(a.kmer_counts, b.kmer_counts)
    assert np.array_equal(a.spectrum, b.spectrum) and np.array_equal(a.unitig_sums, b.unitig_sums)


@pytest.mark.parametrize("k", CC.KS)
def test_compact_unitigs_colored(gpu, k):
    x, y = CASES["pair"]
    unitigs, stats, _, ab, col, _ = T.coloured(k, False)
    runs = [api.compact_unitigs_colored([x, y], k, [0, 1], 2) for _ in range(2)]
    _assert_store(runs[0], unitigs, stats)
    _assert_colors_equal_ref(runs[0][3], col, 2)
    masks = runs[0][3].kmer_colors
    assert set(masks.tolist()) == {1, 2} and int(runs[0][3].shared[0, 1]) == 0 and runs[0][3].occupancy[2] == 0  # no mask is 3
    assert runs[0][2].kmer_counts.tolist() == ab["kmer_counts"] and set(ab["kmer_counts"]) == {1}
    assert _store(runs[1]) == _store(runs[0]) and runs[1][1] == runs[0][1]
    for f in ("kmer_colors", "per_color", "shared", "occupancy"):
        assert np.array_equal(getattr(runs[0][3], f), getattr(runs[1][3], f)), f


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("k", CC.KS)
def test_compact_unitigs_colored_classes(gpu, k, split):
    x, y = CASES["pair"]
    unitigs, stats, _, ab, col, classes = T.coloured(k, split)
    runs = [api.compact_unitigs_colored_classes([x, y], k, [0, 1], 2, split=split) for _ in range(2)]
    store, c, a, co, cc = runs[0]
    _assert_store(runs[0], unitigs, stats)
    _assert_colors_equal_ref(co, col, 2)
    assert a.kmer_counts.tolist() == ab["kmer_counts"]
    _assert_classes(cc, classes, co.kmer_colors, c.unitigs, split)
    assert cc.masks.tolist() == [1, 2] and cc.kmers.tolist() == [len(x) - k + 1] * 2 and int(co.shared[0, 1]) == 0
    assert _store(runs[1]) == _store(runs[0]) and runs[1][1] == c and np.array_equal(runs[1][3].kmer_colors, co.kmer_colors)
    for f in ("masks", "kmers", "runs", "first", "kmer_class"):
        assert np.array_equal(getattr(cc, f), getattr(runs[1][4], f)), f


def _assert_index_answers(ix, want):
    """query, locate, abundance and color_hits of one index (built with everything) against the restatements; each call twice."""
    c, q, loc, ab, col = want
    for again in range(2):
        got = ix.query(c["query"], bits=True)
        for f in ("kmers", "valid", "found", "valid_bits", "present_bits"):
            assert getattr(got, f).dtype == np.uint64 and getattr(got, f).tolist() == q[f], (again, f)
        got = ix.locate(c["query"])
        for f in ("kmers", "valid", "found"):
            assert getattr(got, f).tolist() == loc[f], (again, f)
        assert got.runs.dtype == api.KMER_RUN_DTYPE and _runs(got) == loc["runs"], (again, _runs(got)[:8], loc["runs"][:8])
        _assert_abundance(ix.abundance(c["query"], per_window=True), ab, True)
        _assert_hits_equal_ref(ix.color_hits(c["query"], per_window=True), col, c["n_colors"], True)


@pytest.mark.parametrize("k", CC.KS)
def test_index_lookup_compares_the_query_with_the_index(gpu, k):
    """An index of x asked for y, revcomp(y) and x: nothing of y is there, although every window of y that holds the block has the
    hash of a window of x."""
    want = T.indexed("lookup", k)
    c = want[0]
    W = len(c["index"][0]) - k + 1
    with api.KmerIndex(c["index"], k, locate=True, weights=c["weights"], colors=c["masks"], n_colors=c["n_colors"]) as ix, \
            api.KmerIndex(c["index"], k) as plain:
        assert ix.info.distinct == ix.info.occurrences == plain.info.distinct == W
        _assert_index_answers(ix, want)
        got = plain.query(c["query"], bits=True)
        assert got.found.tolist() == [0, 0, W] and got.present_bits.tolist() == want[1]["present_bits"]


@pytest.mark.parametrize("k", CC.KS)
def test_index_build_keeps_both_classes_of_a_probe_sequence(gpu, k):
    """An index of x and y: every k-mer is found, in its own record, with its own weight and mask."""
    want = T.indexed("claim", k)
    c = want[0]
    W = len(c["index"][0]) - k + 1
    with api.KmerIndex(c["index"], k, locate=True, weights=c["weights"], colors=c["masks"], n_colors=c["n_colors"]) as ix:
        assert ix.info.distinct == ix.info.occurrences == 2 * W
        _assert_index_answers(ix, want)
        got = ix.locate(c["query"])
        assert got.found.tolist() == [W] * 4 and [int(r["t_record"]) for r in got.runs] == [0, 1, 1, 0]
        pw = ix.abundance(c["query"][:2], per_window=True).per_window.tolist()
        assert pw[:W] == c["weights"][:W] and pw[len(c["query"][0]):len(c["query"][0]) + W] == c["weights"][W:]
        assert ix.color_hits(c["query"]).per_color.tolist() == [[W, 0], [0, W], [0, W], [W, 0]]


def test_the_join_keeps_the_two_ends_apart(gpu):
    recs, k = CASES["join"], CC.K_NODES
    want = T.joined()
    runs = [api.Bigraph.from_sequences(recs, k).export() for _ in range(2)]
    _assert_graph(runs[0], want, "join")
    assert len(runs[0]["mirror"]) == 14
    for f in runs[0]:
        assert np.array_equal(runs[0][f], runs[1][f]), f
    # the compaction's nodes on the same records: the unitigs that end in X or Y stay unitigs
    unitigs, stats, _ = compact_ref.compact(recs, k)
    _assert_store(api.compact_unitigs(recs, k), unitigs, stats)


def _cli(*a):
    return subprocess.run([sys.executable, "-m", "matchtigs_amd", *a], capture_output=True, text=True, cwd=str(ROOT), timeout=600)


def test_one_pass_through_the_product(gpu, tmp_path):
    k = 1031
    x, y = CASES["pair"]
    p = {n: str(tmp_path / n) for n in ("pair.fa", "x.fa", "y.fa", "u.fa", "g.fa")}
    Path(p["pair.fa"]).write_text(FA.fasta_text([x, y], width=70))
    Path(p["x.fa"]).write_text(FA.fasta_text([x]))
    Path(p["y.fa"]).write_text(FA.fasta_text([y]))
    r = _cli("--seq-in", p["pair.fa"], "-k", str(k), "--unitigs-fa-out", p["u.fa"], "--greedytigs-fa-out", p["g.fa"], "--verify")
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stderr.splitlines() if l.startswith("Verifying ")]
    assert len(lines) == 1 and "k-mer sets equal" in lines[0] and f"{2 * (len(x) - k + 1)} distinct k-mers" in lines[0], r.stderr[-3000:]
    assert Path(p["u.fa"]).read_text().split("\n")[1::2] == T.compacted("pair", k)[0] == [x, y]
    tigs = Path(p["g.fa"]).read_text().split("\n")[1::2]
    assert sorted(synth.canonical(t) for t in tigs) == sorted(synth.canonical(t) for t in (x, y))
    # x's file against y's sequence: nothing in common, and the report names a k-mer of either side
    r = _cli("--seq-in", p["y.fa"], "-k", str(k), "--verify-fa", p["x.fa"])
    lines = [l for l in r.stderr.splitlines() if l.startswith("Verifying ")]
    assert r.returncode == 1 and len(lines) == 1 and "DIFFER" in lines[0], r.stderr[-3000:]
    missing = lines[0].split("first missing k-mer: ")[1].split(";")[0].split()[-1]
    foreign = lines[0].split("first foreign k-mer: ")[1].split(";")[0].split()[-1]
    assert missing == y[:k] and foreign == x[:k]
