"""`--query-abundance-out`, `--query-abundance-profile-out`, `--unitig-kmer-abundance-out` through the CLI on the GPU:
every row and line against the restatement (kmer_abundance_ref.py), the three older query files byte for byte those of a run without
the new flags, the abundance output alone (m = 1 implied), and a threshold nothing reaches."""
import gzip
import subprocess
import sys
from pathlib import Path

import pytest

import kmer_abundance_ref as R
import kmer_query_ref as Q
from matchtigs_amd import synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
K = 21


def _cli(*a):
    return subprocess.run([sys.executable, "-m", "matchtigs_amd", *a], capture_output=True, text=True, cwd=str(ROOT), timeout=600)


def _fasta(path):
    return [l for l in Path(path).read_text().splitlines() if not l.startswith(">")]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    genome, reads = R.reads_case()
    query = [genome, synth.revcomp(genome).lower(), genome[:100] + "N" + genome[101:200] + "ryK" + genome[203:260], "ACGT", "",
             reads[3], "ACCGTTAGC" * 5, "T" * 40]
    d = tmp_path_factory.mktemp("kmer_abundance_cli")
    (d / "reads.fa").write_text("".join(f">r{i}\n{r[:80]}\n{r[80:]}\n" for i, r in enumerate(reads)))
    (d / "q.fa").write_text("".join(f">q{i} some text\n{s}\n" for i, s in enumerate(query)))
    return d, reads, query


def _rows(names, want):
    return [f"{name}\t{n}\t{v}\t{f}\t{s}\t{lo}\t{hi}\t{f'{s / f:.3f}' if f else '-'}" for name, n, v, f, s, lo, hi in zip(
        names, want["kmers"], want["valid"], want["found"], want["sum"], want["min"], want["max"])]


def test_all_three_outputs_beside_the_older_ones(product_lib, inputs):
    d, reads, query = inputs
    p = {n: str(d / n) for n in ("reads.fa", "q.fa", "u.fa", "r.tsv", "p.txt", "l.tsv", "ab.tsv.gz", "prof.txt", "kc.txt", "g.fa",
                                 "r0.tsv", "p0.txt", "l0.tsv")}
    r = _cli("--seq-in", p["reads.fa"], "-k", str(K), "--min-abundance", "2", "--unitigs-fa-out", p["u.fa"], "--greedytigs-fa-out", p["g.fa"],
             "--verify", "--query-fa", p["q.fa"], "--query-out", p["r.tsv"], "--query-presence-out", p["p.txt"], "--query-locate-out", p["l.tsv"],
             "--query-abundance-out", p["ab.tsv.gz"], "--query-abundance-profile-out", p["prof.txt"], "--unitig-kmer-abundance-out", p["kc.txt"])
    print(r.stderr[-3000:])
    assert r.returncode == 0, r.stderr[-3000:]
    assert "Verifying abundance filter: " in r.stderr and "as counted" in r.stderr and "k-mer sets equal" in r.stderr
    unitigs = _fasta(p["u.fa"])
    counts = R.window_counts(unitigs, reads, K)
    assert min(counts) >= 2
    # the k-mer abundances of the unitigs: line i = the windows of fasta record i
    lines = Path(p["kc.txt"]).read_text().split("\n")
    assert lines.pop() == "" and len(lines) == len(unitigs)
    at = 0
    for line, u in zip(lines, unitigs):
        n = len(u) - K + 1
        assert line == " ".join(map(str, counts[at:at + n]))
        at += n
    # one abundance row per query record
    want = R.abundance(unitigs, counts, query, K)
    rows = gzip.open(p["ab.tsv.gz"], "rt").read().split("\n")
    assert rows.pop() == "" and rows[0] == "record\tkmers\tvalid\tfound\tsum\tmin\tmax\tmean"
    assert rows[1:] == _rows([f"q{i}" for i in range(len(query))], want)
    assert want["found"][0] == want["found"][1] > 100 and want["found"][4] == 0 and rows[5].endswith("\t0\t0\t0\t-")
    assert [x.split("\t")[0] for x in rows[1:]] == [x.split("\t")[0] for x in Path(p["r.tsv"]).read_text().splitlines()[1:]]
    # one profile line per query record
    bits = Q.query(set(R.class_weights(unitigs, counts, K)), query, K)["valid_bits"]
    lines = Path(p["prof.txt"]).read_text().split("\n")
    assert lines.pop() == "" and lines == [R.profile_line(want, query, bits, i, K) for i in range(len(query))]
    assert "-" in lines[2].split(" ") and "0" in lines[0].split(" ") and lines[3] == lines[4] == ""
    # the older query files do not notice
    r = _cli("--seq-in", p["reads.fa"], "-k", str(K), "--min-abundance", "2", "--query-fa", p["q.fa"], "--query-out", p["r0.tsv"],
             "--query-presence-out", p["p0.txt"], "--query-locate-out", p["l0.tsv"])
    assert r.returncode == 0, r.stderr[-3000:]
    for a, b in (("r.tsv", "r0.tsv"), ("p.txt", "p0.txt"), ("l.tsv", "l0.tsv")):
        assert Path(p[a]).read_bytes() == Path(p[b]).read_bytes() and Path(p[a]).stat().st_size > 0, a


def test_the_abundance_output_alone_counts_without_filtering(product_lib, inputs):
    d, reads, query = inputs
    r = _cli("--seq-in", str(d / "reads.fa"), "-k", str(K), "--query-fa", str(d / "q.fa"), "--query-out", str(d / "r1.tsv"),
             "--query-abundance-out", str(d / "ab1.tsv"), "--unitigs-fa-out", str(d / "u1.fa"))
    assert r.returncode == 0 and ", 0 dropped; " in r.stderr, r.stderr[-3000:]
    unitigs = _fasta(d / "u1.fa")
    counts = R.window_counts(unitigs, reads, K)
    assert 1 in counts
    rows = (d / "ab1.tsv").read_text().split("\n")
    assert rows.pop() == "" and rows[1:] == _rows([f"q{i}" for i in range(len(query))], R.abundance(unitigs, counts, query, K))
    assert rows[6].split("\t")[1:4] == [str(150 - K + 1)] * 3  # a read: every window is in the set


def test_no_kmer_reaches_the_threshold(product_lib, inputs):
    d, _, _ = inputs
    ab, kc, tsv = d / "ab99.tsv", d / "kc99.txt", d / "r99.tsv"
    r = _cli("--seq-in", str(d / "reads.fa"), "-k", str(K), "--min-abundance", "99", "--query-fa", str(d / "q.fa"), "--query-out", str(tsv),
             "--query-abundance-out", str(ab), "--unitig-kmer-abundance-out", str(kc))
    assert r.returncode == 1 and "no k-mer reaches --min-abundance 99" in r.stderr, r.stderr[-3000:]
    assert not ab.exists() and not kc.exists() and not tsv.exists()


def test_profile_without_the_presence_output(product_lib, inputs):
    """The profile needs the valid bits, which the run then has to ask for itself: beside `--query-locate-out`, gzip-compressed."""
    d, reads, query = inputs
    r = _cli("--seq-in", str(d / "reads.fa"), "-k", str(K), "--min-abundance", "3", "--unitigs-fa-out", str(d / "u3.fa"), "--query-fa", str(d / "q.fa"),
             "--query-out", str(d / "r3.tsv"), "--query-locate-out", str(d / "l3.tsv"), "--query-abundance-out", str(d / "ab3.tsv"),
             "--query-abundance-profile-out", str(d / "prof3.txt.gz"))
    assert r.returncode == 0, r.stderr[-3000:]
    unitigs = _fasta(d / "u3.fa")
    counts = R.window_counts(unitigs, reads, K)
    want = R.abundance(unitigs, counts, query, K)
    bits = Q.query(set(R.class_weights(unitigs, counts, K)), query, K)["valid_bits"]
    lines = gzip.open(d / "prof3.txt.gz", "rt").read().split("\n")
    assert lines.pop() == "" and lines == [R.profile_line(want, query, bits, i, K) for i in range(len(query))]
    assert (d / "ab3.tsv").read_text().split("\n")[1:-1] == _rows([f"q{i}" for i in range(len(query))], want)
