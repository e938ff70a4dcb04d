"""The counted unitig compaction (`--min-abundance`, mtg_compact_unitigs_counted), the part that needs no GPU: hand cases
for the restatement the GPU tests compare against (abundance_ref.py), its agreement with compact_ref at m = 1, the flag rules (each in
a child process, refused before any GPU use) and the new C entry points, declared and exported."""
import ctypes as C
import random
import re
import subprocess
import sys
from pathlib import Path

import abundance_ref as A
import compact_ref as R

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = ("mtg_compact_unitigs_counted", "mtg_compact_unitigs_counted_store", "mtg_abundance_sums_count", "mtg_abundance_sums_array",
                "mtg_abundance_sums_free")


def test_both_strands_and_repeats_count():
    count = A.abundances(["AAAA", "TTT"], 3)
    assert count == {"AAA": 3}  # two windows of the first record, one of the second on the other strand


def test_a_palindromic_window_counts_once():
    assert A.abundances(["ACGT"], 4) == {"ACGT": 1}
    assert A.abundances(["ACGT", "acgt"], 4) == {"ACGT": 2}


def test_spectrum_bins():
    s = A.spectrum_of({"a": 1, "b": 1, "c": 254, "d": 255, "e": 256, "f": 100000})
    assert s[0] == 0 and s[1] == 2 and s[254] == 1 and s[255] == 3 and sum(s) == 6 and len(s) == 256


def test_statistics_of_a_hand_case():
    # k = 3: AAA x3 (AAAA, TTT), AAC x1 = GTT, ACG x1 = CGT
    u, stats, closed, ab = A.compact_counted(["AAAACG", "TTT"], 3, 2)
    assert u == ["AAA"] and closed == [True]
    assert stats["windows"] == 5 and stats["distinct_kmers"] == 1 and stats["unitigs"] == 1
    assert (ab["distinct_all"], ab["distinct_kept"], ab["dropped"], ab["max_abundance"], ab["kept_occurrences"]) == (3, 1, 2, 3, 3)
    assert ab["spectrum"][1] == 2 and ab["spectrum"][3] == 1 and ab["unitig_sums"] == [3]
    u, stats, _, ab = A.compact_counted(["AAAACG", "TTT"], 3, 4)  # nothing reaches the threshold
    assert u == [] and stats["unitigs"] == 0 and stats["windows"] == 5 and ab["distinct_kept"] == 0 and sum(ab["spectrum"]) == 3


def test_creators_come_from_all_windows():
    """The first window of a kept k-mer may lie in a record whose other k-mers are dropped: its reading is taken there."""
    g = "ACGGTCATTGGA"
    bad = R.revcomp(g[:6] + "T" + g[7:])  # one substitution, given on the other strand, in front
    u1, _, _, ab = A.compact_counted([bad, g, g], 5, 2)
    u2, _, _ = R.compact([g], 5)
    assert sorted(R.canonical(x) for x in u1) == sorted(R.canonical(x) for x in u2)
    assert u1 != u2  # the readings follow `bad`, which shows the kept k-mers first and reversed
    assert ab["dropped"] == len(A.abundances([bad], 5).keys() - A.abundances([g], 5).keys())


def test_m_1_equals_the_plain_restatement():
    rng = random.Random(11)
    for case in range(50):
        alphabet = "ACGT" if case % 2 else "AC"
        records = ["".join(rng.choice(alphabet) for _ in range(rng.randrange(0, 40))) for _ in range(rng.randrange(1, 5))]
        k = rng.choice([2, 3, 4, 5, 8])
        u, stats, closed, ab = A.compact_counted(records, k, 1)
        assert (u, stats, closed) == R.compact(records, k)
        assert ab["distinct_all"] == ab["distinct_kept"] == stats["distinct_kmers"] and ab["kept_occurrences"] == stats["windows"]
        assert sum(c * n for c, n in enumerate(ab["spectrum"])) == stats["windows"]


def _run(*a):
    return subprocess.run([sys.executable, "-m", "matchtigs_amd", *a], capture_output=True, text=True, cwd=str(ROOT), timeout=300)


def test_flag_rules(tmp_path, product_lib):
    s, out = str(tmp_path / "s.fa"), str(tmp_path / "u.fa")
    (tmp_path / "s.fa").write_text(">0\nACGTACGT\n")
    r = _run("--fa-in", s, "-k", "5", "--unitigs-fa-out", out, "--min-abundance", "2")
    assert r.returncode == 2 and "--min-abundance needs --seq-in" in r.stderr, r.stderr[-500:]
    r = _run("--seq-in", s, "-k", "5", "--unitigs-fa-out", out, "--min-abundance", "0")
    assert r.returncode == 2 and "--min-abundance must be >= 1" in r.stderr, r.stderr[-500:]
    r = _run("--fa-in", s, "-k", "5", "--kmer-spectrum-out", str(tmp_path / "spec.tsv"))
    assert r.returncode == 2 and "--kmer-spectrum-out needs --seq-in" in r.stderr, r.stderr[-500:]
    r = _run("--bcalm-in", s, "-k", "5", "--unitigs-fa-out", out, "--unitig-abundance-out", str(tmp_path / "ab.tsv"))
    assert r.returncode == 2 and "--unitig-abundance-out needs --seq-in" in r.stderr, r.stderr[-500:]
    assert not (tmp_path / "u.fa").exists() and not (tmp_path / "spec.tsv").exists()


def test_an_output_flag_counts_as_something_to_do(tmp_path, product_lib):
    """`--kmer-spectrum-out` alone passes the "nothing to do" rule: the run gets as far as opening the (missing) input."""
    r = _run("--seq-in", str(tmp_path / "missing.fa"), "-k", "5", "--kmer-spectrum-out", str(tmp_path / "spec.tsv"))
    assert r.returncode != 0 and "cannot open" in r.stderr and "nothing to do" not in r.stderr, r.stderr[-500:]
    r = _run("--seq-in", str(tmp_path / "missing.fa"), "-k", "5", "--min-abundance", "2")
    assert r.returncode == 2 and "nothing to do" in r.stderr


def test_help_lists_the_flags(product_lib):
    r = _run("--help")
    assert r.returncode == 0 and all(f in r.stdout for f in ("--min-abundance", "--kmer-spectrum-out", "--unitig-abundance-out"))


def test_entry_points_declared_and_exported(product_lib):
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mtg_engine.h").read_text(), flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in include/mtg_engine.h"
        assert hasattr(product_lib, name), f"{name} is not exported"
    from matchtigs_amd import _lib, api

    assert "mtg_abundance" in header and C.sizeof(_lib.MtgAbundance) == 8 * (4 + 256)
    assert callable(api.compact_unitigs_counted)
    syms = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert all(re.search(rf"\b{name}$", syms, flags=re.M) for name in ENTRY_POINTS)  # unmangled: extern "C"


def test_python_refuses_a_zero_threshold(product_lib):
    import pytest

    from matchtigs_amd import api

    with pytest.raises(ValueError, match="min_abundance must be >= 1"):
        api.compact_unitigs_counted(["ACGT"], 3, 0)
