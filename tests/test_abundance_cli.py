"""`--min-abundance`, `--kmer-spectrum-out`, `--unitig-abundance-out` through the CLI on the GPU: the files against the
API and the restatement (abundance_ref.py), both verification lines, greedytigs that equal those of `--fa-in` on the written unitigs,
a threshold nothing reaches, and a run without the new flags."""
import gzip
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import abundance_ref as A
from matchtigs_amd import synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
K = 21


def _cli(*a):
    return subprocess.run([sys.executable, "-m", "matchtigs_amd", *a], capture_output=True, text=True, cwd=str(ROOT), timeout=600)


def _fasta(path):
    return [l for l in Path(path).read_text().splitlines() if not l.startswith(">")]


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    """40 reads of 150 bases from a 600-base genome (10x), either strand, about 1 % substitutions, lower case here and there."""
    rng = np.random.default_rng(3)
    genome = synth.random_genome(600, seed=77, haplotypes=1)[0]
    out = []
    for i in range(40):
        at = int(rng.integers(0, 600 - 150 + 1))
        r = list(genome[at:at + 150])
        for j in np.flatnonzero(rng.random(150) < 0.01):
            r[j] = "ACGT"[("ACGT".index(r[j]) + int(rng.integers(1, 4))) % 4]
        r = "".join(r)
        r = synth.revcomp(r) if rng.random() < 0.5 else r
        out.append(r.lower() if i % 7 == 0 else r)
    d = tmp_path_factory.mktemp("abundance_cli")
    (d / "reads.fa").write_text("".join(f">r{i}\n{r[:80]}\n{r[80:]}\n" for i, r in enumerate(out)))
    return d, out


def test_filtered_run(product_lib, reads):
    from matchtigs_amd import api

    d, seqs = reads
    p = {n: str(d / n) for n in ("reads.fa", "u.fa", "spec.tsv", "ab.tsv.gz", "g.fa", "g2.fa")}
    r = _cli("--seq-in", p["reads.fa"], "-k", str(K), "--min-abundance", "2", "--unitigs-fa-out", p["u.fa"], "--kmer-spectrum-out", p["spec.tsv"],
             "--unitig-abundance-out", p["ab.tsv.gz"], "--greedytigs-fa-out", p["g.fa"], "--verify")
    print(r.stderr[-3000:])
    assert r.returncode == 0, r.stderr[-3000:]
    unitigs, stats, _, ab = A.compact_counted(seqs, K, 2)
    assert ab["dropped"] > 0 and ab["distinct_kept"] > 0
    # the unitig file is the API's store
    store, c, a = api.compact_unitigs_counted(seqs, K, 2)
    assert _fasta(p["u.fa"]) == store.sequences() == unitigs
    # the spectrum rows are the restatement's
    rows = Path(p["spec.tsv"]).read_text().splitlines()
    assert rows[0] == "abundance\tkmers"
    want = [f"{c_}{'+' if c_ == 255 else ''}\t{n}" for c_, n in enumerate(ab["spectrum"]) if n]
    assert rows[1:] == want and len(want) >= 2
    # abundance row i describes fasta record i: k-mers and sum recomputed from the record's own string
    count = A.abundances(seqs, K)
    rows = gzip.open(p["ab.tsv.gz"], "rt").read().splitlines()
    assert rows[0] == "unitig\tkmers\tabundance\tmean" and len(rows) == 1 + len(unitigs)
    for i, (row, rec) in enumerate(zip(rows[1:], _fasta(p["u.fa"]))):
        n = len(rec) - K + 1
        total = sum(count[synth.canonical(rec[j:j + K])] for j in range(n))
        assert row == f"{i}\t{n}\t{total}\t{total / n:.3f}"
    # both verification lines, and the Loaded line tells what the filter did
    assert "Verifying abundance filter: " in r.stderr and "as counted" in r.stderr and "MISMATCH" not in r.stderr
    assert re.search(r"Verifying greedytigs .*k-mer sets equal", r.stderr)
    assert f"{ab['distinct_all']} distinct k-mers -> {ab['distinct_kept']} kept, {ab['dropped']} dropped; max abundance {ab['max_abundance']}" in r.stderr
    line = re.search(r"Verifying abundance filter: .*", r.stderr).group(0)
    assert f"{ab['dropped']} are not ({ab['dropped']} dropped by the filter), 0 foreign" in line
    # the greedytigs equal those of --fa-in on the written unitigs, byte for byte
    r = _cli("--fa-in", p["u.fa"], "-k", str(K), "--greedytigs-fa-out", p["g2.fa"])
    assert r.returncode == 0, r.stderr[-3000:]
    assert Path(p["g.fa"]).read_bytes() == Path(p["g2.fa"]).read_bytes()


def test_no_kmer_reaches_the_threshold(product_lib, reads):
    d, seqs = reads
    spec, u = d / "spec99.tsv", d / "u99.fa"
    r = _cli("--seq-in", str(d / "reads.fa"), "-k", str(K), "--min-abundance", "99", "--unitigs-fa-out", str(u), "--kmer-spectrum-out", str(spec))
    assert r.returncode == 1 and "no k-mer reaches --min-abundance 99" in r.stderr, r.stderr[-3000:]
    ab = A.compact_counted(seqs, K, 99)[3]
    assert ab["distinct_kept"] == 0
    assert spec.read_text().splitlines()[1:] == [f"{c}\t{n}" for c, n in enumerate(ab["spectrum"]) if n]
    assert not u.exists() and "Loaded" not in r.stderr


def test_an_output_flag_alone_counts_without_filtering(product_lib, reads):
    d, seqs = reads
    r = _cli("--seq-in", str(d / "reads.fa"), "-k", str(K), "--unitig-abundance-out", str(d / "ab1.tsv"), "--unitigs-fa-out", str(d / "u1.fa"))
    assert r.returncode == 0, r.stderr[-3000:]
    unitigs, _, _, ab = A.compact_counted(seqs, K, 1)
    assert _fasta(d / "u1.fa") == unitigs and ", 0 dropped; " in r.stderr
    rows = (d / "ab1.tsv").read_text().splitlines()[1:]
    assert [int(x.split("\t")[2]) for x in rows] == ab["unitig_sums"]


def test_without_the_new_flags(product_lib, reads):
    """The plain route: the same bytes as the API's plain compaction and the "Loaded" line in its old shape."""
    from matchtigs_amd import api

    d, seqs = reads
    r = _cli("--seq-in", str(d / "reads.fa"), "-k", str(K), "--unitigs-fa-out", str(d / "u0.fa"))
    assert r.returncode == 0, r.stderr[-3000:]
    store, c = api.compact_unitigs(seqs, K)
    assert _fasta(d / "u0.fa") == store.sequences()
    loaded = re.search(r"Loaded .*", r.stderr).group(0)
    assert re.fullmatch(r"Loaded \d+ unitigs: \d+ nodes, \d+ edges in [\d.]+s \(compacted from " + re.escape(c.describe())
                        + r"; 0 non-ACGT runs cut\)", loaded), loaded
    assert "abundance filter" not in r.stderr and "dropped" not in r.stderr
