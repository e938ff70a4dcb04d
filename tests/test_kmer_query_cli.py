"""What of the k-mer index (`--query-fa`, mtg_kmer_index_*) can be checked without a GPU: the C-ABI's declarations, the
flag rules of the command line, the reader without an alphabet rule, and the restatement the GPU tests compare against."""
import ctypes as C
import gzip
import subprocess
import sys
from pathlib import Path

import kmer_query_ref as R
from matchtigs_amd import _lib, api, synth

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = ("mtg_kmer_index_build", "mtg_kmer_index_build_store", "mtg_kmer_index_get_info", "mtg_kmer_index_query",
                "mtg_kmer_index_free", "mtg_last_kmer_query_times", "mtg_read_sequences_named")


def _cli(*a):
    return subprocess.run([sys.executable, "-m", "matchtigs_amd", *a], capture_output=True, text=True, cwd=str(ROOT), timeout=300)


def test_entry_points_declared_and_exported(product_lib):
    names = _lib.declared_symbols()
    for n in ENTRY_POINTS:
        assert n in names and hasattr(product_lib, n), n
    assert C.sizeof(_lib.MtgKmerIndexInfo) == 7 * 8
    assert [f for f, _ in _lib.MtgKmerIndexInfo._fields_] == ["k", "records", "characters", "occurrences", "distinct", "slots", "device_bytes"]


def test_help_lists_the_flags():
    r = _cli("--help")
    assert r.returncode == 0
    for flag in ("--query-fa", "--query-out", "--query-presence-out"):
        assert flag in r.stdout


def test_flag_rules(tmp_path):
    missing = str(tmp_path / "no_such.fa")
    r = _cli("--fa-in", missing, "-k", "5", "--query-fa", "q.fa")
    assert r.returncode == 2 and "--query-fa needs --query-out" in r.stderr
    r = _cli("--fa-in", missing, "-k", "5", "--query-out", "r.tsv")
    assert r.returncode == 2 and "--query-out needs --query-fa" in r.stderr
    r = _cli("--fa-in", missing, "-k", "5", "--query-presence-out", "p.txt")
    assert r.returncode == 2 and "--query-presence-out needs" in r.stderr
    r = _cli("--fa-in", missing, "--query-fa", "q.fa", "--query-out", "r.tsv")
    assert r.returncode == 2 and "--fa-in requires -k" in r.stderr
    # the pair is something to do: the run gets as far as opening the input
    r = _cli("--fa-in", missing, "-k", "5", "--query-fa", "q.fa", "--query-out", str(tmp_path / "r.tsv"))
    assert r.returncode != 0 and "nothing to do" not in r.stderr and "cannot open" in r.stderr, r.stderr[-2000:]
    r = _cli("--fa-in", missing, "-k", "5")
    assert r.returncode == 2 and "nothing to do" in r.stderr


FASTA = (b">first one  more text\nACGTN\nnnacgt\n"
         b">second\tx\r\nacgtRYKM\r\n\r\nAC-GT*\r\n"
         b">\n"
         b">empty\n"
         b">last|7 \nA\n")
WANT_NAMES = ["first", "second", "", "empty", "last|7"]
WANT_SEQS = ["ACGTNnnacgt", "acgtRYKMAC-GT*", "", "", "A"]


def test_read_sequences_named(product_lib, tmp_path):
    plain, gz = tmp_path / "q.fa", tmp_path / "q.fa.gz"
    plain.write_bytes(FASTA)
    gz.write_bytes(gzip.compress(FASTA))
    for path in (plain, gz):
        store, names = api.read_sequences_named(str(path))
        assert names == WANT_NAMES
        assert store.sequences() == WANT_SEQS and len(store) == 5
        data, off = store.arrays()
        assert off.tolist() == [0, 11, 25, 25, 25, 26] and bytes(data) == "".join(WANT_SEQS).encode()


def test_read_sequences_still_rejects_n(product_lib, tmp_path):
    p = tmp_path / "n.fa"
    p.write_text(">a\nACGTNACGT\n")
    r = subprocess.run([sys.executable, "-c", f"from matchtigs_amd import api; api.read_sequences({str(p)!r}); print('read')"],
                       capture_output=True, text=True, cwd=str(ROOT), timeout=300)
    assert r.returncode != 0 and "read" not in r.stdout and "not in the DNA alphabet" in r.stderr


def test_restatement_agrees_with_synth():
    k = 5
    g = synth.g_seq(300, seed=3, k=k)
    index = R.index_set(g.unitigs, k)
    assert index == synth.kmer_set_of_tigs(g.unitigs, k) == g.kmers
    foreign = "ACGTTGCAAACCGGTT"
    seqs = [g.unitigs[0].lower(), synth.revcomp(g.unitigs[1]), foreign, "", "AC"]
    r = R.query(index, seqs, k)
    assert r["kmers"] == [max(0, len(s) - k + 1) for s in seqs] and r["valid"] == r["kmers"]
    assert r["found"][0] == r["kmers"][0] and r["found"][1] == r["kmers"][1]
    assert r["found"][2] == sum(synth.canonical(foreign[i:i + k]) in g.kmers for i in range(len(foreign) - k + 1))
    assert r["valid_bits"] == r["present_bits"] or r["found"][2] < r["kmers"][2]
    assert sum(bin(w).count("1") for w in r["valid_bits"]) == sum(r["valid"])
    assert sum(bin(w).count("1") for w in r["present_bits"]) == sum(r["found"])
    assert R.presence(r, seqs, 0) == "1" * r["kmers"][0] and R.presence(r, seqs, 3) == ""
    # an N costs exactly the windows that cover it
    s = g.unitigs[0]
    rn = R.query(index, [s[:7] + "N" + s[8:]], k)
    assert rn["valid"][0] == rn["found"][0] == len(s) - k + 1 - (min(7, len(s) - k) - max(0, 7 - k + 1) + 1)
