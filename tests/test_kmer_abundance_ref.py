"""What of the k-mer abundance query (`--query-abundance-out`, mtg_kmer_index_abundance) can be checked without a GPU:
the restatement the GPU tests compare against (kmer_abundance_ref.py) on cases derived by hand, the flag rules of the command line,
and the C-ABI's declarations."""
import pytest

import kmer_abundance_ref as R
import kmer_query_ref as Q
from matchtigs_amd import _lib, synth
from matchtigs_amd.__main__ import _integer_lines, main

ENTRY_POINTS = ("mtg_compact_unitigs_counted_kmers", "mtg_compact_unitigs_counted_kmers_store", "mtg_kmer_counts_count",
                "mtg_kmer_counts_array", "mtg_kmer_counts_free", "mtg_kmer_index_build_weighted", "mtg_kmer_index_build_weighted_store",
                "mtg_kmer_index_is_weighted", "mtg_kmer_index_abundance", "mtg_last_kmer_abundance_times")


def test_palindrome_counts_once_per_window():
    assert synth.revcomp("ACGT") == "ACGT"
    assert R.window_counts(["ACGT"], ["ACGT"], 4) == [1]
    assert R.window_counts(["ACGT"], ["ACGT", "acgt", "ACGTA"], 4) == [3]
    # as a weight it answers for both readings of the query, which are one
    r = R.abundance(["ACGT"], [7], ["ACGT", "acgt"], 4)
    assert r["found"] == [1, 1] and r["sum"] == r["min"] == r["max"] == [7, 7]


def test_kmer_seen_on_both_strands():
    assert synth.canonical("GTT") == "AAC"
    assert R.window_counts(["GTT"], ["AAC", "GTT"], 3) == [2]
    assert R.window_counts(["AACC"], ["AAC", "GTT", "GGTT"], 3) == [3, 1]  # AAC, GTT, GTT of GGTT; ACC = rc(GGT)
    assert R.window_counts(["AAC", "TTT"], ["AAC"], 3) == [1, 0]  # a window the reads do not show


def test_repeated_kmer_takes_the_weight_of_its_first_occurrence():
    # windows AC CG GA AC: the second AC comes too late
    assert R.class_weights(["ACGAC"], [5, 6, 7, 9], 2) == {"AC": 5, "CG": 6, "GA": 7}
    r = R.abundance(["ACGAC"], [5, 6, 7, 9], ["AC", "GT", "TCG", "TT"], 2)  # GT = rc(AC); TC = rc(GA), CG its own
    assert r["kmers"] == r["valid"] == [1, 1, 2, 1] and r["found"] == [1, 1, 2, 0]
    assert r["sum"] == [5, 5, 13, 0] and r["min"] == [5, 5, 6, 0] and r["max"] == [5, 5, 7, 0]
    # ... also when the second occurrence is the reverse complement, in another record
    assert R.class_weights(["AC", "GT"], [3, 4], 2) == {"AC": 3}
    assert R.class_weights(["GT", "AC"], [3, 4], 2) == {"AC": 3}
    # a weight of 0 is a weight: found, with sum 0
    r = R.abundance(["AC"], [0], ["ACAC"], 2)  # AC, CA (absent), AC
    assert r["found"] == [2] and r["sum"] == r["min"] == r["max"] == [0]


def test_short_record_shifts_no_ordinal():
    # records ACG, A, TTT at k = 3: two windows, the record between them has none
    assert R.windows(["ACG", "A", "TTT"], 3) == ["ACG", "TTT"]
    assert R.class_weights(["ACG", "A", "TTT"], [10, 20], 3) == {"ACG": 10, "AAA": 20}
    assert R.abundance(["ACG", "A", "", "TTT"], [10, 20], ["AAAA", "CGT"], 3)["sum"] == [40, 10]
    with pytest.raises(ValueError):
        R.class_weights(["ACG", "A", "TTT"], [10, 20, 30], 3)
    with pytest.raises(ValueError):
        R.class_weights(["ACG", "A", "TTT"], [10], 3)


def test_per_window_and_profile_lines():
    query = ["ACGNACG", "AC", "acg", ""]
    r = R.abundance(["ACG"], [4], query, 3)
    assert r["kmers"] == [5, 0, 1, 0] and r["valid"] == r["found"] == [2, 0, 1, 0]
    assert r["sum"] == [8, 0, 4, 0] and r["min"] == r["max"] == [4, 0, 4, 0]
    assert r["per_window"] == [4, 0, 0, 0, 4, 0, 0] + [0, 0] + [4, 0, 0]
    bits = Q.query({"ACG"}, query, 3)["valid_bits"]
    assert [R.profile_line(r, query, bits, i, 3) for i in range(4)] == ["4 - - - 4", "", "4", ""]
    # an absent window is 0, not -
    r = R.abundance(["ACG"], [4], ["ACGG"], 3)
    assert R.profile_line(r, ["ACGG"], Q.query({"ACG"}, ["ACGG"], 3)["valid_bits"], 0, 3) == "4 0"


def test_integer_lines():
    assert _integer_lines([4, 0, 4294967295, 10], [0, 3, 0, 0, 1, 0]) == b"\n4 0 4294967295\n\n\n10\n\n"
    assert _integer_lines([4, 0, 9, 100], [4], [False, True, False, True]) == b"4 - 9 -\n"
    assert _integer_lines([], []) == b"" and _integer_lines([], [0, 0]) == b"\n\n"


@pytest.mark.parametrize("argv, message", [
    (["--fa-in", "u.fa", "-k", "5", "--query-fa", "q.fa", "--query-out", "r.tsv", "--query-abundance-out", "a.tsv"],
     "--query-abundance-out needs --seq-in, --query-fa and --query-out"),
    (["--seq-in", "s.fa", "-k", "5", "--query-abundance-out", "a.tsv"], "--query-abundance-out needs --seq-in, --query-fa and --query-out"),
    (["--seq-in", "s.fa", "-k", "5", "--query-abundance-out", "a.tsv", "--unitigs-fa-out", "u.fa"],
     "--query-abundance-out needs --seq-in, --query-fa and --query-out"),
    (["--seq-in", "s.fa", "-k", "5", "--query-fa", "q.fa", "--query-out", "r.tsv", "--query-abundance-profile-out", "p.txt"],
     "--query-abundance-profile-out needs --query-abundance-out"),
    (["--fa-in", "u.fa", "-k", "5", "--unitig-kmer-abundance-out", "kc.txt"], "--unitig-kmer-abundance-out needs --seq-in"),
    (["--bcalm-in", "u.fa", "-k", "5", "--unitig-kmer-abundance-out", "kc.txt", "--greedytigs-fa-out", "g.fa"],
     "--unitig-kmer-abundance-out needs --seq-in"),
])
def test_flag_rules(capsys, argv, message):
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert e.value.code == 2 and message in capsys.readouterr().err


def test_unitig_kmer_abundance_out_is_something_to_do(capsys, tmp_path):
    """Alone with --seq-in it passes the flag rules: the run gets as far as opening the input."""
    with pytest.raises(SystemExit) as e:
        main(["--seq-in", str(tmp_path / "s.fa"), "-k", "5"])
    assert e.value.code == 2 and "nothing to do" in capsys.readouterr().err
    import subprocess
    import sys

    r = subprocess.run([sys.executable, "-m", "matchtigs_amd", "--seq-in", str(tmp_path / "no_such.fa"), "-k", "5",
                        "--unitig-kmer-abundance-out", str(tmp_path / "kc.txt")], capture_output=True, text=True, cwd=str(_lib.REPO_DIR), timeout=300)
    assert r.returncode != 0 and "nothing to do" not in r.stderr and "needs" not in r.stderr and "cannot open" in r.stderr, r.stderr[-2000:]


def test_help_lists_the_flags(capsys):
    with pytest.raises(SystemExit):
        main(["--help"])
    out = capsys.readouterr().out
    assert all(f in out for f in ("--query-abundance-out", "--query-abundance-profile-out", "--unitig-kmer-abundance-out"))


def test_entry_points_declared_and_exported(product_lib):
    names = _lib.declared_symbols()
    for n in ENTRY_POINTS:
        assert n in names and hasattr(product_lib, n), n
