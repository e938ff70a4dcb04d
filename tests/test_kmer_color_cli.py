"""`--color-matrix-out`, `--unitig-colors-out`, `--query-colors-out` through the CLI on the GPU: three `--seq-in` files
-- a FASTA with an `N`, a gzipped FASTQ cut by `--min-base-quality`, a second FASTA -- are three colours; every file is checked line
for line against the restatement (kmer_color_ref.py), the older outputs are byte for byte those of the run without the colour flags,
and the matrix alone is something to do."""
import gzip
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import fastq_ref as F
import kmer_abundance_ref as KA
import kmer_color_ref as R
from matchtigs_amd import synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
K, Q = 21, 20


def _cli(*a):
    return subprocess.run([sys.executable, "-m", "matchtigs_amd", *map(str, a)], capture_output=True, text=True, cwd=str(ROOT), timeout=600)


def _fasta(path):
    return [l for l in Path(path).read_text().splitlines() if not l.startswith(">")]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """-> (directory, the records the three files hold once cut, their colours, the query records and their names)."""
    d = tmp_path_factory.mktemp("kmer_color_cli")
    rng = np.random.default_rng(8)
    genome = synth.random_genome(600, seed=31, haplotypes=1)[0]
    other = synth.random_genome(200, seed=32, haplotypes=1)[0]
    a = [genome[:180] + "NN" + genome[182:350], genome[300:420].lower()]
    (d / "a.fa").write_text("".join(f">a{i} x\n{s[:70]}\n{s[70:]}\n" for i, s in enumerate(a)))
    reads = []
    for i in range(30):
        at = int(rng.integers(200, 600 - 100 + 1))
        r, q = genome[at:at + 100], [40] * 100
        for j in np.flatnonzero(rng.random(100) < 0.03):
            q[j] = 5
        if i % 2:
            r, q = synth.revcomp(r), q[::-1]
        reads.append((f"r{i}".encode(), r.encode(), bytes(x + 33 for x in q)))
    text = F.fastq_text(reads)
    (d / "b.fq.gz").write_bytes(gzip.compress(text))
    c = [synth.revcomp(genome[100:260]), other, "ACGT"]
    (d / "c.fa").write_text("".join(f">c{i}\n{s}\n" for i, s in enumerate(c)))
    data, off, _ = F.split(text, Q)
    pieces = [[p for s in a for p in re.split("[^ACGT]+", s.upper()) if p], [data[off[i]:off[i + 1]].decode() for i in range(len(off) - 1)], c]
    assert len(pieces[0]) == 3 and len(pieces[1]) > 30  # the N and the low qualities cut
    records = [p for f in pieces for p in f]
    colors = [i for i, f in enumerate(pieces) for _ in f]
    query = [genome, synth.revcomp(other).lower(), genome[:50] + "N" + genome[51:120], "ACGT", "", synth.random_genome(80, seed=33, haplotypes=1)[0]]
    (d / "q.fa").write_text("".join(f">q{i} text\n{s}\n" for i, s in enumerate(query)))
    return d, records, colors, query, [f"q{i}" for i in range(len(query))]


def _lines(path):
    raw = Path(path).read_bytes()
    text = (gzip.decompress(raw) if str(path).endswith(".gz") else raw).decode()
    assert text.endswith("\n")
    return text[:-1].split("\n")


def test_all_three_outputs_beside_the_older_ones(product_lib, inputs):
    d, records, colors, query, qnames = inputs
    names = [str(d / n) for n in ("a.fa", "b.fq.gz", "c.fa")]
    p = {n: str(d / n) for n in ("m.tsv", "uc.txt.gz", "qc.tsv.gz", "u.fa", "hits.tsv", "t.fa", "u0.fa", "hits0.tsv", "t0.fa", "q.fa")}
    common = ["--seq-in", names[0], "--seq-in", names[1], "--seq-in", names[2], "-k", K, "--min-base-quality", Q, "--query-fa", p["q.fa"], "--verify"]
    r = _cli(*common, "--color-matrix-out", p["m.tsv"], "--unitig-colors-out", p["uc.txt.gz"], "--unitigs-fa-out", p["u.fa"], "--query-out", p["hits.tsv"],
             "--query-colors-out", p["qc.tsv.gz"], "--greedytigs-fa-out", p["t.fa"])
    print(r.stderr[-3000:])
    assert r.returncode == 0, r.stderr[-3000:]
    assert "k-mer sets equal" in r.stderr and "DIFFER" not in r.stderr
    r0 = _cli(*common, "--unitigs-fa-out", p["u0.fa"], "--query-out", p["hits0.tsv"], "--greedytigs-fa-out", p["t0.fa"])
    assert r0.returncode == 0, r0.stderr[-3000:]
    for x, y in (("u.fa", "u0.fa"), ("hits.tsv", "hits0.tsv"), ("t.fa", "t0.fa")):
        assert Path(p[x]).read_bytes() == Path(p[y]).read_bytes() and Path(p[x]).stat().st_size > 0, x
    loaded = [l for l in r.stderr.splitlines() if l.startswith("Loaded ")], [l for l in r0.stderr.splitlines() if l.startswith("Loaded ")]
    assert len(loaded[0]) == 1 and re.sub(r" in [0-9.]+s", "", loaded[0][0]) == re.sub(r" in [0-9.]+s", "", loaded[1][0])
    assert "Colours:" not in r0.stderr
    # the restatement on the records the files hold
    unitigs, _, _, ab, want = R.compact_colored(records, colors, 3, K)
    assert _fasta(p["u.fa"]) == unitigs
    assert min(want["occupancy"][1:4]) > 0 and want["per_color"][2] > want["shared"][2][0] > 0  # private, pairs, core; c.fa has k-mers of its own
    assert _lines(p["m.tsv"]) == R.matrix_lines(names, want)
    assert _lines(p["uc.txt.gz"]) == R.unitig_color_lines(unitigs, want["kmer_colors"], K)
    assert any(" " in l for l in _lines(p["uc.txt.gz"]))  # a unitig whose colours change
    hits = R.color_hits(unitigs, want["kmer_colors"], 3, query, K)
    assert _lines(p["qc.tsv.gz"]) == R.query_color_lines(names, qnames, hits)
    assert 0 < sum(hits["found"]) < sum(hits["valid"]) < sum(hits["kmers"])
    line = [l for l in r.stderr.splitlines() if l.startswith("Colours: ")]
    assert len(line) == 1 and line[0].startswith(
        f"Colours: {ab['distinct_kept']} k-mers kept in 3 colours, {want['occupancy'][3]} core, {want['occupancy'][1]} private; closest pair ")
    jac = R.jaccard(want["per_color"], want["shared"])
    pairs = {(i, j): jac[i][j] for i in range(3) for j in range(i + 1, 3)}
    hi, lo = max(pairs, key=pairs.get), min(pairs, key=pairs.get)
    assert f"closest pair {names[hi[0]]} / {names[hi[1]]} (Jaccard {pairs[hi]:.4f}), most distant {names[lo[0]]} / {names[lo[1]]} (Jaccard {pairs[lo]:.4f})" in line[0]


def test_the_matrix_alone_is_something_to_do(product_lib, inputs):
    d, records, colors, _, _ = inputs
    names = [str(d / n) for n in ("c.fa", "a.fa")]  # another order: colour 0 is c.fa
    recs = [r for r, c in zip(records, colors) if c == 2] + [r for r, c in zip(records, colors) if c == 0]
    cols = [0] * colors.count(2) + [1] * colors.count(0)
    out = d / "alone.tsv.gz"
    r = _cli("--seq-in", names[0], "--seq-in", names[1], "-k", K, "--min-abundance", 2, "--color-matrix-out", out)
    assert r.returncode == 0, r.stderr[-3000:]
    want = R.compact_colored(recs, cols, 2, K, 2)
    assert want[3]["distinct_kept"] > 0 and want[3]["dropped"] > 0
    assert _lines(out) == R.matrix_lines(names, want[4])
    one = d / "one.tsv"
    r = _cli("--seq-in", names[1], "-k", K, "--color-matrix-out", one, "--unitig-colors-out", d / "one.txt")  # one file: one colour
    assert r.returncode == 0, r.stderr[-3000:]
    n = len({synth.canonical(w) for w in KA.windows([x for x, c in zip(records, colors) if c == 0], K)})
    assert _lines(one) == [f"color\tkmers\t{names[1]}", f"{names[1]}\t{n}\t{n}", f"#occupancy\t{n}"]
    assert all(re.fullmatch(r"\d+:1", l) for l in _lines(d / "one.txt")) and "closest pair" not in r.stderr
