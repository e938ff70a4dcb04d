"""What of the k-mer tally (mtg_kmer_tally_*, api.KmerTally, `--count-fa`) can be checked without a GPU: the
restatement (kmer_tally_ref.py) on cases derived by hand, the C-ABI's declarations, the result's fields, the closed tally and the
flag rules of the command line."""
import ctypes as C
import dataclasses
import subprocess
import sys
import types
from pathlib import Path

import numpy as np
import pytest

import kmer_query_ref as Q
import kmer_tally_ref as T
from matchtigs_amd import _lib, api, synth

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = ("mtg_kmer_tally_create", "mtg_kmer_tally_device_bytes", "mtg_kmer_tally_add", "mtg_kmer_tally_coverage",
                "mtg_kmer_tally_reset", "mtg_kmer_tally_free", "mtg_last_kmer_tally_times", "mtg_kmer_tally_add_store",
                "mtg_kmer_tally_coverage_store")


def test_both_strands_land_on_one_counter():
    k, index = 3, ["AAC"]  # rc(AAC) = GTT; canonical AAC
    ix = Q.index_set(index, k)
    assert ix == {"AAC"}
    counts = T.tally(ix, [["AAC", "gtt", "GTTAAC"]], k)  # GTTAAC: GTT, TTA, TAA, AAC
    assert counts == {"AAC": 4}
    cov = T.coverage(ix, counts, ["AAC", "GTT", "ACG"], k)
    assert cov["found"] == [1, 1, 0] and cov["covered"] == [1, 1, 0] and cov["sum"] == [4, 4, 0] and cov["max"] == [4, 4, 0]
    assert cov["per_window"] == [4, 0, 0, 4, 0, 0, 0, 0, 0]


def test_a_palindromic_kmer_counts_once_per_window():
    k = 4
    assert synth.revcomp("ACGT") == "ACGT"
    ix = Q.index_set(["ACGTT"], k)  # ACGT (its own reverse complement), CGTT -> canonical AACG
    assert ix == {"ACGT", "AACG"}
    counts = T.tally(ix, [["ACGT", "acgt"], ["AACGT"]], k)  # two adds; AACGT: AACG, ACGT
    assert counts == {"ACGT": 3, "AACG": 1}
    cov = T.coverage(ix, counts, ["ACGTT"], k)
    assert (cov["covered"], cov["sum"], cov["max"], cov["per_window"]) == ([2], [4], [3], [3, 1, 0, 0, 0])


def test_a_repeat_inside_one_read_counts_twice():
    k = 3
    ix = Q.index_set(["ACGA"], k)  # ACG (< CGT), CGA (< TCG)
    assert ix == {"ACG", "CGA"}
    counts = T.tally(ix, [["ACGTACG"]], k)  # ACG, CGT (= ACG), GTA, TAC (= GTA), ACG
    assert counts == {"ACG": 3}
    cov = T.coverage(ix, counts, ["ACGA", "ACGACG"], k)  # a k-mer asked twice contributes to each of its windows
    # ACGACG: ACG (3), CGA (in the index, never added), GAC (= GTC: not in the index), ACG (3)
    assert cov["found"] == [2, 3] and cov["covered"] == [1, 2] and cov["sum"] == [3, 6] and cov["max"] == [3, 3]
    assert cov["per_window"] == [3, 0, 0, 0, 3, 0, 0, 3, 0, 0]


def test_an_n_costs_the_k_windows_over_it():
    k = 3
    s = "ACGTACGTAC"
    ix = Q.index_set([s], k)
    whole = T.tally(ix, [[s]], k)
    masked = T.tally(ix, [[s[:4] + "N" + s[5:]]], k)  # the windows that start at 2, 3, 4 hold the N
    assert sum(whole.values()) == 8 and sum(masked.values()) == 8 - k
    lost = whole - masked
    assert lost == T.tally(ix, [[s[2:7]]], k) and sum(lost.values()) == k
    # junk bytes and lower case: only ACGTacgt make a window valid
    assert T.tally(ix, [["acgRacg", "AC-GT", "acg"]], k) == {"ACG": 3}


def test_a_record_shorter_than_k_adds_and_shows_nothing():
    k = 5
    ix = Q.index_set(["ACGTAGG", "ACGT"], k)  # the second record has no window
    assert len(ix) == 3
    assert T.tally(ix, [["ACGT", "", "A"]], k) == {}
    cov = T.coverage(ix, T.tally(ix, [["ACGTAGG"]], k), ["ACGT", "", "ACGTAGG"], k)
    assert cov["kmers"] == [0, 0, 3] and cov["found"] == [0, 0, 3] and cov["covered"] == [0, 0, 3] and cov["sum"] == [0, 0, 3]
    assert cov["max"] == [0, 0, 1] and len(cov["per_window"]) == 11


def test_count_tsv_bytes():
    k = 3
    unitigs = ["ACGA", "TTT"]
    got = T.count_tsv(unitigs, [["ACGTACG", "AAA"], ["NNNN"]], ["a.fq", "dir/b.fa.gz"], k)
    assert got == (b"unitig\tkmers\ta.fq:covered\ta.fq:sum\tdir/b.fa.gz:covered\tdir/b.fa.gz:sum\n"
                   b"0\t2\t1\t3\t0\t0\n"
                   b"1\t1\t1\t1\t0\t0\n")


def test_entry_points_declared_and_exported(product_lib):
    names = _lib.declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for n in ENTRY_POINTS:
        assert n in names and n in syms, n  # unmangled => extern "C"
        f = getattr(product_lib, n)
        assert f.argtypes is not None, n
    u64, vp = C.c_uint64, C.c_void_p
    assert product_lib.mtg_kmer_tally_create.restype is vp and product_lib.mtg_kmer_tally_create.argtypes == [vp]
    assert product_lib.mtg_kmer_tally_device_bytes.restype is u64
    assert product_lib.mtg_kmer_tally_add.argtypes == [vp, vp, vp, u64, vp, vp, vp] and product_lib.mtg_kmer_tally_add.restype is None
    assert product_lib.mtg_kmer_tally_coverage.argtypes == [vp, vp, vp, u64] + [vp] * 7
    assert product_lib.mtg_kmer_tally_add_store.argtypes == [vp] * 5 and product_lib.mtg_kmer_tally_coverage_store.argtypes == [vp] * 9
    assert product_lib.mtg_last_kmer_tally_times.argtypes == [C.POINTER(C.c_double)]
    product_lib.mtg_kmer_tally_free(None)  # NULL is fine, and touches no device
    assert set(api.last_kmer_tally_times()) == {"upload_ms", "pack_ms", "probe_ms", "download_ms"}


def test_headers_compile_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "mtg_engine.h"\n#include "matchtigs.h"\n'
                   "int main(void) {\n    uint64_t off[2] = {0, 4}, kmers[1], valid[1], found[1], covered[1], sum[1], max[1], per_window[4];\n"
                   "    double t[4];\n    mtg_unitigs *store = 0;\n"
                   "    mtg_kmer_index *ix = mtg_kmer_index_build(\"ACGT\", off, 1, 3, 0);\n"
                   "    mtg_kmer_tally *tally = mtg_kmer_tally_create(ix);\n"
                   "    uint64_t bytes = mtg_kmer_tally_device_bytes(tally);\n"
                   "    mtg_kmer_tally_add(tally, \"ACGT\", off, 1, kmers, valid, found);\n"
                   "    mtg_kmer_tally_add_store(tally, store, kmers, valid, found);\n"
                   "    mtg_kmer_tally_coverage(tally, \"ACGT\", off, 1, kmers, valid, found, covered, sum, max, per_window);\n"
                   "    mtg_kmer_tally_coverage_store(tally, store, kmers, valid, found, covered, sum, max, 0);\n"
                   "    mtg_kmer_tally_reset(tally);\n    mtg_last_kmer_tally_times(t);\n    mtg_kmer_tally_free(tally);\n"
                   "    mtg_kmer_index_free(ix);\n    return (int)(bytes + sum[0]);\n}\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", str(ROOT / "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_coverage_result_fields():
    fields = ["k", "offsets", "kmers", "valid", "found", "covered", "sum", "max", "per_window"]
    assert [f.name for f in dataclasses.fields(api.KmerCoverageResult)] == fields
    z = np.zeros(1, np.uint64)
    r = api.KmerCoverageResult(3, np.zeros(2, np.uint64), z, z, z, z, z, z)
    assert r.per_window is None
    with pytest.raises(dataclasses.FrozenInstanceError):
        r.sum = z


def _fake(tally_open, index_open):
    """A KmerTally and its KmerIndex without a library behind them: any call that reached it would raise AttributeError."""
    ix = api.KmerIndex.__new__(api.KmerIndex)
    ix._L = types.SimpleNamespace(mtg_kmer_index_free=lambda h: None)
    ix._h = 1 if index_open else None
    t = api.KmerTally.__new__(api.KmerTally)
    t._L = types.SimpleNamespace(mtg_kmer_tally_free=lambda h: None)
    t._h = 1 if tally_open else None
    t.index = ix
    return t, ix


def test_a_closed_tally_refuses():
    for tally_open, index_open, message in ((False, True, "the tally is closed"), (False, False, "the tally is closed"),
                                            (True, False, "the index is closed")):
        t, ix = _fake(tally_open, index_open)
        for call in (lambda: t.add(["ACGT"]), lambda: t.coverage(["ACGT"]), lambda: t.coverage(["ACGT"], per_window=True), t.reset):
            with pytest.raises(ValueError) as e:
                call()
            assert str(e.value) == message
        t.close()
        t.close()
        ix._h = None
    t, ix = _fake(True, False)
    with pytest.raises(ValueError) as e:
        api.KmerTally(ix)  # no tally on a closed index
    assert str(e.value) == "the index is closed"
    with pytest.raises(TypeError):
        api.KmerTally(["ACGT"])
    t.close()
    # a context manager that holds its index
    t, ix = _fake(True, True)
    with t as same:
        assert same is t and t.index is ix
    assert t._h is None


def _cli(*a):
    return subprocess.run([sys.executable, "-m", "matchtigs_amd", *a], capture_output=True, text=True, cwd=str(ROOT), timeout=300)


BASE = ("--fa-in", "no_such.fa", "-k", "21")
COUNT = ("--count-fa", "c.fa", "--count-out", "d.tsv")
REFUSED = [
    (("--count-fa", "c.fa"), ["--count-fa needs --count-out"]),
    (("--count-fa", "c.fa", "--count-fa", "d.fq", "--greedytigs-fa-out", "g.fa"), ["--count-fa needs --count-out"]),
    (("--count-out", "d.tsv"), ["--count-out needs --count-fa"]),
    (("--count-out", "d.tsv", "--query-fa", "q.fa", "--query-out", "r.tsv"), ["--count-out needs --count-fa"]),
    (("--count-min-base-quality", "20", "--greedytigs-fa-out", "g.fa"), ["--count-min-base-quality needs --count-fa"]),
    (("--count-min-base-quality", "20", "--query-fa", "q.fq", "--query-out", "r.tsv"), ["--count-min-base-quality needs --count-fa"]),
    (COUNT + ("--count-min-base-quality", "94"), ["--count-min-base-quality must be in 0..93"]),
    (COUNT + ("--count-min-base-quality", "-1"), ["--count-min-base-quality must be in 0..93"]),
    (COUNT + ("--count-min-base-quality", "x"), ["--count-min-base-quality", "invalid int value"]),
    # the older quality flags say what they said
    (COUNT + ("--min-base-quality", "94"), ["--min-base-quality must be in 0..93"]),
    (COUNT + ("--query-min-base-quality", "94"), ["--query-min-base-quality must be in 0..93"]),
]


@pytest.mark.parametrize("i", range(len(REFUSED)))
def test_flag_rules(i):
    """Each refusal is argparse's own (exit status 2, `error:`): it comes before the library is loaded, let alone a GPU used."""
    given, parts = REFUSED[i]
    r = _cli(*(BASE + given))
    assert r.returncode == 2 and "error:" in r.stderr, (given, r.stderr[-500:])
    last = r.stderr.strip().splitlines()[-1]
    for part in parts:
        assert part in last, (given, last)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("kmer_tally_cli")
    (d / "reads.fa").write_text(">a\nACGTACGTACGTACGTACGTACGTACGT\n")
    (d / "reads.fq").write_text("@a\nACGTACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIII\n")
    return d


def test_quality_flags_need_a_fastq_file_of_their_own(product_lib, files):
    """After format detection (the content decides, not the name), still argparse's error and before any input is read."""
    fa, fq, out = str(files / "reads.fa"), str(files / "reads.fq"), str(files / "d.tsv")
    for given, message in (
            (("--count-fa", fa, "--count-out", out, "--count-min-base-quality", "20"), "--count-min-base-quality needs a fastq file among --count-fa"),
            (("--count-fa", fa, "--count-fa", fa, "--count-out", out, "--count-min-base-quality", "0", "--query-fa", fq, "--query-out", "r.tsv"),
             "--count-min-base-quality needs a fastq file among --count-fa"),
            # a fastq count file does not serve the older flags: their messages are the ones they always gave
            (("--count-fa", fq, "--count-out", out, "--min-base-quality", "20"), "--min-base-quality needs a fastq file among --seq-in / --query-fa"),
            (("--count-fa", fq, "--count-out", out, "--query-fa", fa, "--query-out", "r.tsv", "--query-min-base-quality", "20"),
             "--query-min-base-quality needs a fastq file among --query-fa")):
        r = _cli(*BASE, *given)
        assert r.returncode == 2 and "error:" in r.stderr, (given, r.stderr[-500:])
        assert r.stderr.strip().splitlines()[-1].endswith(message), (given, r.stderr[-500:])
        assert not (files / "d.tsv").exists()


def test_accepted_flags_get_as_far_as_the_input(product_lib, files, tmp_path):
    fa, fq, out = str(files / "reads.fa"), str(files / "reads.fq"), str(tmp_path / "d.tsv.gz")
    for route in ("--fa-in", "--bcalm-in", "--seq-in"):
        for extra in (("--count-fa", fa, "--count-out", out),
                      ("--count-fa", fq, "--count-fa", fa, "--count-out", out, "--count-min-base-quality", "20"),
                      ("--count-fa", fq, "--count-out", out, "--count-min-base-quality", "0", "--query-fa", fa, "--query-out", str(tmp_path / "r.tsv")),
                      ("--count-fa", fa, "--count-out", out, "--greedytigs-fa-out", str(tmp_path / "g.fa"), "--unitigs-fa-out", str(tmp_path / "u.fa"))):
            r = _cli(route, str(tmp_path / "no_such.fa"), "-k", "21", *extra)
            assert r.returncode != 0 and "error:" not in r.stderr and "cannot open" in r.stderr, (route, extra, r.stderr[-1000:])
            assert not (tmp_path / "d.tsv.gz").exists()
    # a count file that is not there is found out at format detection
    r = _cli("--fa-in", fa, "-k", "21", "--count-fa", str(tmp_path / "no_such.fq"), "--count-out", out)
    assert r.returncode != 0 and "error:" not in r.stderr and "cannot open" in r.stderr and "no_such.fq" in r.stderr
    r = _cli("--help")
    for flag in ("--count-fa", "--count-out", "--count-min-base-quality"):
        assert flag in r.stdout
