"""What of locating k-mers (`--query-locate-out`, mtg_kmer_index_locate) can be checked without a GPU: the C-ABI's
declarations, the flag rules of the command line, and the restatement the GPU tests compare against, on cases derived by hand."""
import subprocess
import sys
from pathlib import Path

import kmer_locate_ref as R
from matchtigs_amd import _lib, synth

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = ("mtg_kmer_index_build_locating", "mtg_kmer_index_build_locating_store", "mtg_kmer_index_is_locating",
                "mtg_kmer_index_locate", "mtg_kmer_runs_count", "mtg_kmer_runs_arrays", "mtg_kmer_runs_free",
                "mtg_last_kmer_locate_times")


def _cli(*a):
    return subprocess.run([sys.executable, "-m", "matchtigs_amd", *a], capture_output=True, text=True, cwd=str(ROOT), timeout=300)


def test_entry_points_declared_and_exported(product_lib):
    names = _lib.declared_symbols()
    for n in ENTRY_POINTS:
        assert n in names and hasattr(product_lib, n), n


def test_help_lists_the_flag():
    r = _cli("--help")
    assert r.returncode == 0 and "--query-locate-out" in r.stdout


def test_flag_rules(tmp_path):
    missing = str(tmp_path / "no_such.fa")
    for extra in ((), ("--query-fa", "q.fa"), ("--query-out", "r.tsv"), ("--greedytigs-fa-out", "g.fa")):
        r = _cli("--fa-in", missing, "-k", "5", "--query-locate-out", "l.tsv", *extra)
        assert r.returncode == 2 and "--query-locate-out needs --query-fa and --query-out" in r.stderr, (extra, r.stderr[-500:])
    # with both, the run gets as far as opening the input
    r = _cli("--fa-in", missing, "-k", "5", "--query-fa", "q.fa", "--query-out", str(tmp_path / "r.tsv"),
             "--query-locate-out", str(tmp_path / "l.tsv"))
    assert r.returncode != 0 and "needs" not in r.stderr and "cannot open" in r.stderr, r.stderr[-2000:]


def test_adjacent_records_at_k1():
    # the windows of adjacent records are adjacent at k = 1, and still two runs: the locations lie in two index records
    r = R.locate(["A", "C"], ["AC"], 1)
    assert r["runs"] == [(0, 0, 1, 0, 0, 0), (0, 1, 1, 0, 1, 0)] and r["found"] == [2]
    # ... one record: one run; the query cut in two records: two runs
    assert R.locate(["AC"], ["AC"], 1)["runs"] == [(0, 0, 2, 0, 0, 0)]
    assert R.locate(["AC"], ["A", "C"], 1)["runs"] == [(0, 0, 1, 0, 0, 0), (1, 0, 1, 0, 0, 1)]
    # G is C's class, found at C's place on the reverse strand; GT = rc(AC) is one - run
    assert R.locate(["AC"], ["GT"], 1)["runs"] == [(0, 0, 2, 1, 0, 0)]


def test_homopolymer_repeats_break_runs():
    r = R.locate(["AAAAAA"], ["AAAAA"], 3)
    assert r["runs"] == [(0, 0, 1, 0, 0, 0), (0, 1, 1, 0, 0, 0), (0, 2, 1, 0, 0, 0)]
    r = R.locate(["AAAAAA"], ["TTTTT"], 3)
    assert r["runs"] == [(0, 0, 1, 1, 0, 0), (0, 1, 1, 1, 0, 0), (0, 2, 1, 1, 0, 0)]
    assert r["kmers"] == r["valid"] == r["found"] == [3]


def test_palindrome_is_forward():
    assert synth.revcomp("ACGT") == "ACGT"
    assert R.locate(["ACGT"], ["acgt"], 4)["runs"] == [(0, 0, 1, 0, 0, 0)]
    # inside a forward copy it is one of the run; inside a reverse-complemented copy it is still +, and cuts the - run in two
    assert R.locate(["GGACGTAA"], ["GACGTA"], 4)["runs"] == [(0, 0, 3, 0, 0, 1)]
    assert R.locate(["GGACGTAA"], ["TACGTC"], 4)["runs"] == [(0, 0, 1, 1, 0, 3), (0, 1, 1, 0, 0, 2), (0, 2, 1, 1, 0, 1)]


def test_copy_and_reverse_complement_share_t_start():
    index = ["GGGGGGG", "ACCGATTGCAT", ""]  # (k = 5: no palindromes, and no k-mer of the second record repeats)
    assert R.locate(index, [index[1]], 5)["runs"] == [(0, 0, 7, 0, 1, 0)]
    assert R.locate(index, [synth.revcomp(index[1])], 5)["runs"] == [(0, 0, 7, 1, 1, 0)]
    # a piece from the middle, lower case, behind an N: offsets on both sides
    assert R.locate(index, ["", "tNcgattg"], 5)["runs"] == [(1, 2, 2, 0, 1, 2)]
    r = R.locate(index, ["caatcgNN"], 5)
    assert r["runs"] == [(0, 0, 2, 1, 1, 2)]
    assert r["kmers"] == [4] and r["valid"] == [2] and r["found"] == [2]


def test_spelling_invariant_on_g_seq():
    k = 5
    g = synth.g_seq(300, seed=3, k=k)
    index = g.unitigs
    query = [index[0].lower(), synth.revcomp(index[1]), "ACGTTGCAAACCGGTT", "", "AC", index[2][:9] + "N" + index[2][10:],
             index[3] + synth.revcomp(index[4])]
    r = R.locate(index, query, k)
    assert r["kmers"] == [max(0, len(s) - k + 1) for s in query]
    assert sum(n for _, _, n, _, _, _ in r["runs"]) == sum(r["found"])
    assert all(R.spells(index, query, run, k) for run in r["runs"])
    # unitigs hold every k-mer once, so a copy of a unitig is one run over all of it, on either strand
    assert r["runs"][0] == (0, 0, len(index[0]) - k + 1, 0, 0, 0)
    assert r["runs"][1] == (1, 0, len(index[1]) - k + 1, 1, 1, 0)
    assert r["runs"] == sorted(r["runs"], key=lambda x: (x[0], x[1]))
