"""The k-mer set verification (`--verify`, `--verify-fa`), the part that needs no GPU: the C entry points are declared
and exported, the flag rules (each in a child process), the graph-free FASTA reader, and the restatement the GPU tests
(test_gpu_kmer_compare.py) compare against agrees with the two k-mer set helpers the suite already had."""
import ctypes as C
import gzip
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import kmer_compare_ref as R
from matchtigs_amd import synth

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = ("mtg_compare_kmer_sets", "mtg_compare_kmer_sets_stores", "mtg_read_sequences", "mtg_last_kmer_compare_times")


def _run(*a):
    return subprocess.run([sys.executable, "-m", "matchtigs_amd", *a], capture_output=True, text=True, cwd=str(ROOT), timeout=300)


def _py(code, *a):
    return subprocess.run([sys.executable, "-c", code, *a], capture_output=True, text=True, cwd=str(ROOT), timeout=300)


def test_entry_points_declared_and_exported(product_lib):
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mtg_engine.h").read_text(), flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in include/mtg_engine.h"
        assert hasattr(product_lib, name), f"{name} is not exported"
    assert "mtg_kmer_comparison" in header
    from matchtigs_amd import _lib

    assert C.sizeof(_lib.MtgKmerComparison) == 15 * 8


def test_help_lists_both_flags(product_lib):
    r = _run("--help")
    assert r.returncode == 0 and "--verify " in r.stdout and "--verify-fa" in r.stdout


def test_verify_is_accepted_with_an_output(tmp_path, product_lib):
    """The flags parse: the run gets as far as opening the (missing) input."""
    r = _run("--bcalm-in", str(tmp_path / "missing.fa"), "-k", "5", "--eulertigs-fa-out", str(tmp_path / "o.fa"), "--verify")
    assert r.returncode != 0 and "cannot open" in r.stderr and "unrecognized arguments" not in r.stderr, r.stderr[-500:]


def test_verify_alone_is_nothing_to_do(tmp_path, product_lib):
    r = _run("--bcalm-in", str(tmp_path / "u.fa"), "-k", "5", "--verify")
    assert r.returncode != 0 and "nothing to do" in r.stderr


def test_verify_fa_without_input(tmp_path, product_lib):
    r = _run("--verify-fa", str(tmp_path / "t.fa"))
    assert r.returncode != 0 and "Missing input argument" in r.stderr


def test_verify_fa_requires_k(tmp_path, product_lib):
    (tmp_path / "u.fa").write_text(">0\nACGTACGT\n")
    r = _run("--verify-fa", str(tmp_path / "t.fa"), "--fa-in", str(tmp_path / "u.fa"))
    assert r.returncode != 0 and "--fa-in requires -k" in r.stderr


def test_verify_fa_counts_as_something_to_do(tmp_path, product_lib):
    """`--verify-fa` alone passes the "nothing to do" rule: the run gets as far as opening the (missing) input."""
    r = _run("--verify-fa", str(tmp_path / "t.fa"), "--verify-fa", str(tmp_path / "t2.fa"), "--bcalm-in", str(tmp_path / "missing.fa"), "-k", "5")
    assert r.returncode != 0 and "cannot open" in r.stderr and "nothing to do" not in r.stderr, r.stderr[-500:]


RECORDS = ["ACGTTGCA", "AC", "", "GGGTTTAAACCC", "T"]
TEXT = ">first record, any text L:+:1:-\nacgt\nTGca\n\n>2\nAC\n>empty\n>4 multi\nGGG\r\nttt\nAAAccc\n>5\nT"


@pytest.mark.parametrize("gz", [False, True])
def test_read_sequences(tmp_path, product_lib, gz):
    """Multi-line, mixed case, CRLF, an empty record and records shorter than any k, plain and gzipped, against the literal strings."""
    from matchtigs_amd import api

    p = tmp_path / ("t.fa.gz" if gz else "t.fa")
    p.write_bytes(gzip.compress(TEXT.encode()) if gz else TEXT.encode())
    st = api.read_sequences(str(p))
    assert len(st) == len(RECORDS) and st.sequences() == RECORDS


def test_read_sequences_empty_file(tmp_path, product_lib):
    from matchtigs_amd import api

    (tmp_path / "e.fa").write_text("")
    assert api.read_sequences(str(tmp_path / "e.fa")).sequences() == []


def test_read_sequences_rejects_non_acgt(tmp_path, product_lib):
    (tmp_path / "n.fa").write_text(">0\nACGT\nACNT\n")
    r = _py("import sys; from matchtigs_amd import api; api.read_sequences(sys.argv[1])", str(tmp_path / "n.fa"))
    assert r.returncode != 0 and "character 'N' is not in the DNA alphabet" in r.stderr, r.stderr[-500:]


def test_read_fasta_keeps_its_length_rule(tmp_path, product_lib):
    (tmp_path / "s.fa").write_text(">0\nACGTACGT\n>1\nACG\n")
    r = _py("import sys; from matchtigs_amd import api; api.read_fasta(sys.argv[1], 5)", str(tmp_path / "s.fa"))
    assert r.returncode != 0 and "record 1 has length 3 < k = 5" in r.stderr, r.stderr[-500:]


def test_comparison_properties():
    from matchtigs_amd import api

    c = api.KmerComparison(**R.compare(["ACGTT", "AACGT"], ["ACGTA"], 4))
    assert (c.occurrences_a, c.distinct_a, c.repeated_a, c.repeated_b) == (4, 2, 2, 0)  # AACG == rc(CGTT), ACGT twice
    assert not c.equal and (c.only_in_a, c.only_in_b, c.common) == (1, 1, 1)
    assert (c.first_only_in_a_record, c.first_only_in_a_pos, c.first_only_in_b_record, c.first_only_in_b_pos) == (0, 1, 0, 1)
    assert "1 missing" in c.describe() and "1 foreign" in c.describe()
    e = api.KmerComparison(**R.compare(["ACGTT"], ["AACGT"], 4))
    assert e.equal and e.first_only_in_a_record == R.NONE and "equal" in e.describe()
    assert api.kmer_at(["ACGTT", "aacgt"], 1, 1, 4) == "ACGT"


@pytest.mark.parametrize("k", [9, 12, 21, 31, 32, 41])
def test_restatement_agrees_with_the_helpers(k):
    ug = synth.g_seq(4000, seed=k, k=min(k, 31), haplotypes=3, sub_rate=0.03)
    a = ug.unitigs + ["ACGT" * 12, "acgt" * 12, "A" * k, "T" * (k - 1), ""]
    b = [synth.revcomp(s) for s in a[::2]] + ["G" * (k + 3)]
    r = R.compare(a, b, k)
    sa, sb = synth.kmer_set_of_tigs([s.upper() for s in a], k), synth.kmer_set_of_tigs([s.upper() for s in b], k)
    assert r["distinct_a"] == len(sa) and r["distinct_b"] == len(sb)
    assert (r["common"], r["only_in_a"], r["only_in_b"]) == (len(sa & sb), len(sa - sb), len(sb - sa))
    assert r["occurrences_a"] == sum(max(0, len(s) - k + 1) for s in a)
    assert r["only_in_a"] > 0 and r["only_in_b"] > 0
    ra, pa = r["first_only_in_a_record"], r["first_only_in_a_pos"]
    assert synth.canonical(a[ra].upper()[pa:pa + k]) in sa - sb
    assert all(x in sb for rr, pp, x in R.windows(a, k) if (rr, pp) < (ra, pa))
    if k % 2 == 1 and k <= 31:
        for seqs, n in ((a, r["distinct_a"]), (b, r["distinct_b"])):
            seqs = [s for s in seqs if len(s) >= k]  # (the numpy helper takes no shorter record)
            data = np.frombuffer("".join(seqs).upper().encode(), np.uint8)
            off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
            assert len(synth.kmer_codes_of_sequences(data, off, k)) == n
