"""`--unitigs-bcalm-out` and `--unitigs-gfa-out` through the CLI on the GPU: a counted and cleaned `--seq-in` run whose
BCALM2 file carries the abundances, the sequences of `--unitigs-fa-out` and the links of the GFA file; that file read back by
`--bcalm-in` with verified greedytigs; the link route's graph against the `--fa-in` join of the same unitigs; both flags on the
other two inputs."""
import gzip
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import fasta_in_ref as F
import unitig_links_ref as R
from matchtigs_amd import synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
K = 21


def _cli(*a):
    return subprocess.run([sys.executable, "-m", "matchtigs_amd", *a], capture_output=True, text=True, cwd=str(ROOT), timeout=600)


def _fasta(path):
    return [l for l in Path(path).read_text().splitlines() if not l.startswith(">")]


def _gfa_links(path):
    """The L lines of a GFA file as link tuples in file order, each checked to follow the S line of its unitig."""
    links, last = [], None
    for line in Path(path).read_text().splitlines()[1:]:
        f = line.split("\t")
        if f[0] == "S":
            last = int(f[1])
        else:
            assert f[0] == "L" and int(f[1]) == last and f[5] == f"{K - 1}M", line
            links.append((int(f[1]), f[2] == "+", int(f[3]), f[4] == "+"))
    return links


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """One `--seq-in` run with every unitig output: 40 reads of 150 bases from a 600-base genome, either strand, about 1 %
    substitutions, plus 6 reads given once per strand with one substitution near an end (tips above --min-abundance 2)."""
    rng = np.random.default_rng(3)
    genome = synth.random_genome(600, seed=77, haplotypes=1)[0]
    out = []
    for i in range(40):
        at = int(rng.integers(0, 600 - 150 + 1))
        r = list(genome[at:at + 150])
        for j in np.flatnonzero(rng.random(150) < 0.01):
            r[j] = "ACGT"[("ACGT".index(r[j]) + int(rng.integers(1, 4))) % 4]
        r = "".join(r)
        out.append(synth.revcomp(r) if rng.random() < 0.5 else r)
    for i in range(6):
        at = int(rng.integers(0, 600 - 150 + 1))
        r, j = list(genome[at:at + 150]), (4 + i if i % 2 else 145 - i)
        r[j] = "ACGT"[("ACGT".index(r[j]) + 1 + i % 3) % 4]
        out += ["".join(r), synth.revcomp("".join(r))]
    d = tmp_path_factory.mktemp("unitig_links_cli")
    (d / "reads.fa").write_text("".join(f">r{i}\n{r}\n" for i, r in enumerate(out)))
    r = _cli("--seq-in", str(d / "reads.fa"), "-k", str(K), "--min-abundance", "2", "--clip-tips", str(K), "--unitigs-bcalm-out",
             str(d / "u.bcalm.fa.gz"), "--unitigs-gfa-out", str(d / "u.gfa"), "--unitigs-fa-out", str(d / "u.fa"), "--unitig-abundance-out",
             str(d / "ab.tsv"))
    print(r.stderr[-3000:])
    assert r.returncode == 0, r.stderr[-3000:]
    return d, r.stderr


def test_the_files_of_a_counted_run(product_lib, run):
    d, stderr = run
    text = gzip.decompress((d / "u.bcalm.fa.gz").read_bytes()).decode()
    recs = R.parse_bcalm(text)
    unitigs = _fasta(d / "u.fa")
    assert [r["seq"] for r in recs] == unitigs and [r["id"] for r in recs] == list(range(len(unitigs))) and len(unitigs) > 1
    rows = [l.split("\t") for l in (d / "ab.tsv").read_text().splitlines()[1:]]
    assert [r["KC"] for r in recs] == [int(x[2]) for x in rows] and [r["LN"] - K + 1 for r in recs] == [int(x[1]) for x in rows]
    assert any(r["KC"] > r["LN"] - K + 1 for r in recs)  # abundances, not k-mer counts
    assert [r["km"] for r in recs] == [R.km_text(r["KC"], r["LN"] - K + 1) for r in recs]
    links = [l for r in recs for l in r["links"]]
    assert _gfa_links(d / "u.gfa") == links and len(links) > 0
    off, to = R.links_of_sequences(unitigs, K)
    assert links == R.link_tuples(off, to)
    kc = [r["KC"] for r in recs]
    assert text == R.bcalm_text(unitigs, K, off, to, kc) and (d / "u.gfa").read_text() == R.gfa_text(unitigs, K, off, to, kc)
    lines = re.findall(r"Writing unitig graph took [\d.]+s \((\d+) unitigs, (\d+) links, (\d+) bytes\)", stderr)
    assert lines == [(str(len(unitigs)), str(len(links)), str(len(text))),
                     (str(len(unitigs)), str(len(links)), str(len((d / "u.gfa").read_bytes())))]


def test_the_file_feeds_bcalm_in(product_lib, run):
    from matchtigs_amd import api

    d, _ = run
    r = _cli("--bcalm-in", str(d / "u.bcalm.fa.gz"), "-k", str(K), "--greedytigs-fa-out", str(d / "t.fa"), "--verify")
    assert r.returncode == 0, r.stderr[-3000:]
    assert re.search(r"Verifying greedytigs .*k-mer sets equal", r.stderr)
    # the link route against the join of the same unitigs: the same edges, and a node partition that refines the join's
    gl, sl = api.read_bcalm2(str(d / "u.bcalm.fa.gz"), K)
    gf, sf = api.read_fasta(str(d / "u.fa"), K)
    assert sl.sequences() == sf.sequences()
    assert gl.edge_count() == gf.edge_count() and gf.node_count() <= gl.node_count()
    ok, predicted = F.end_partitions_agree(gl.export(), gf.export())
    assert ok and predicted == gl.node_count()


@pytest.mark.parametrize("flag, name", [("--bcalm-in", "u.bcalm.fa.gz"), ("--fa-in", "u.fa")])
def test_both_flags_on_the_other_inputs(product_lib, run, flag, name):
    d, _ = run
    b, g = d / f"again{flag}.fa", d / f"again{flag}.gfa.gz"
    r = _cli(flag, str(d / name), "-k", str(K), "--unitigs-bcalm-out", str(b), "--unitigs-gfa-out", str(g))
    assert r.returncode == 0, r.stderr[-3000:]
    unitigs = _fasta(d / "u.fa")
    off, to = R.links_of_sequences(unitigs, K)
    assert b.read_text() == R.bcalm_text(unitigs, K, off, to)  # nothing was counted: KC is the number of k-mers
    assert gzip.decompress(g.read_bytes()).decode() == R.gfa_text(unitigs, K, off, to)
    assert len(re.findall(r"Writing unitig graph took", r.stderr)) == 2
