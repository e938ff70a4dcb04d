"""FASTQ through the CLI on the GPU: `--seq-in reads.fq --min-base-quality` equals the run on a FASTA twin whose bad
bases were masked by the restatement (fastq_ref.py), two `--seq-in` files equal one concatenated file, `--query-fa reads.fq` equals
its FASTA twin row for row, and the error exits."""
import gzip
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import abundance_ref as A
import fastq_ref as F
from matchtigs_amd import synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
K, Q = 7, 20


def _cli(*a):
    return subprocess.run([sys.executable, "-m", "matchtigs_amd", *map(str, a)], capture_output=True, text=True, cwd=str(ROOT), timeout=600)


def _reads(seed: int, n: int, length: int, genome_bases: int):
    """Reads from one random genome, either strand, about 2 % substitutions which mostly carry a low quality, a few `N`, low qualities
    here and there on correct bases too, lower case now and then."""
    rng = np.random.default_rng(seed)
    genome = synth.random_genome(genome_bases, seed=seed + 1, haplotypes=1)[0]
    out = []
    for i in range(n):
        at = int(rng.integers(0, genome_bases - length + 1))
        r = list(genome[at:at + length])
        q = [40] * length
        for j in np.flatnonzero(rng.random(length) < 0.02):
            r[j] = "ACGT"[("ACGT".index(r[j]) + int(rng.integers(1, 4))) % 4]
            q[j] = 8 if rng.random() < 0.7 else 40
        for j in np.flatnonzero(rng.random(length) < 0.01):
            q[j] = int(rng.integers(0, Q))
        for j in np.flatnonzero(rng.random(length) < 0.005):
            r[j] = "N"
        r = "".join(r)
        if rng.random() < 0.5:
            r, q = synth.revcomp(r), q[::-1]
        r = r.lower() if i % 7 == 0 else r
        out.append((f"read{i}/1 lane {i % 3}".encode(), r.encode(), bytes(x + 33 for x in q)))
    return out


def _pieces(text: bytes, q: int):
    data, off, _ = F.split(text, q)
    return [data[off[i]:off[i + 1]].decode() for i in range(len(off) - 1)]


def test_twin_equivalence(product_lib, tmp_path):
    text = F.fastq_text(_reads(21, 60, 60, 300))
    # what the restatement alone says about these reads: the mask and the abundance filter both remove k-mers, and some are kept
    masked, plain = A.abundances(_pieces(text, Q), K), A.abundances(_pieces(text, 0), K)
    kept = {x for x, c in masked.items() if c >= 2}
    assert any(c >= 2 and x not in kept for x, c in plain.items())  # kept with Q = 0, removed by the mask
    assert any(c < 2 for c in masked.values())                      # removed by --min-abundance 2
    assert kept
    (tmp_path / "r.fq").write_bytes(text)
    (tmp_path / "twin.fa").write_bytes(F.fasta_twin(text, Q))
    outs = {}
    for tag, inp, extra in (("fq", "r.fq", ("--min-base-quality", Q)), ("fa", "twin.fa", ())):
        o = {n: tmp_path / f"{tag}_{n}" for n in ("u.fa", "t.fa", "s.tsv")}
        r = _cli("--seq-in", tmp_path / inp, "-k", K, "--min-abundance", 2, *extra, "--unitigs-fa-out", o["u.fa"], "--greedytigs-fa-out", o["t.fa"],
                 "--kmer-spectrum-out", o["s.tsv"], "--verify")
        print(r.stderr[-3000:])
        assert r.returncode == 0, r.stderr[-3000:]
        assert re.search(r"Verifying greedytigs .*k-mer sets equal", r.stderr) and "as counted" in r.stderr and "MISMATCH" not in r.stderr
        outs[tag] = {n: p.read_bytes() for n, p in o.items()}
        if tag == "fq":
            st = F.split(text, Q)[2]
            assert (f"Read {tmp_path / inp}: {st['records']} records, {st['bases']} bases, {st['non_acgt_bases']} non-ACGT bases, "
                    f"{st['masked_bases']} bases masked by quality -> {st['pieces']} pieces of {st['bases_kept']} bases") in r.stderr
            assert f"{st['pieces_cut']} non-ACGT runs cut)" in r.stderr
    assert outs["fq"] == outs["fa"] and all(outs["fq"].values())
    # the unitigs spell exactly the kept set
    unitigs = [l for l in outs["fq"]["u.fa"].decode().splitlines() if not l.startswith(">")]
    assert set(A.abundances(unitigs, K)) == kept


def test_two_input_files_equal_one_concatenated(product_lib, tmp_path):
    """The README's example as written: R1.fq.gz and R2.fq.gz, k = 31; and a FASTA file mixed in."""
    r1, r2 = F.fastq_text(_reads(31, 40, 100, 500)), F.fastq_text(_reads(32, 40, 100, 500), eol=b"\r\n")
    for name, text in (("R1.fq.gz", r1), ("R2.fq.gz", r2), ("both.fq.gz", r1 + r2)):
        with gzip.open(tmp_path / name, "wb") as f:
            f.write(text)
    (tmp_path / "R2.fa").write_bytes(F.fasta_twin(r2, Q))
    outs = {}
    for tag, inputs in (("two", ("R1.fq.gz", "R2.fq.gz")), ("one", ("both.fq.gz",)), ("mixed", ("R1.fq.gz", "R2.fa"))):
        u, t = tmp_path / f"{tag}_u.fa", tmp_path / f"{tag}_t.fa"
        r = _cli(*(x for i in inputs for x in ("--seq-in", tmp_path / i)), "-k", 31, "--min-abundance", 2, "--min-base-quality", Q,
                 "--unitigs-fa-out", u, "--greedytigs-fa-out", t, "--verify")
        assert r.returncode == 0, r.stderr[-3000:]
        assert re.search(r"Verifying greedytigs .*k-mer sets equal", r.stderr) and "as counted" in r.stderr
        outs[tag] = (u.read_bytes(), t.read_bytes())
    assert outs["two"] == outs["one"] == outs["mixed"] and all(outs["two"])


def test_query_outputs_equal_the_fasta_twin(product_lib, tmp_path):
    reads = F.fastq_text(_reads(41, 40, 60, 300))
    queries = F.fastq_text(_reads(41, 12, 60, 300)[:8] + _reads(43, 4, 60, 300) + [(b"empty", b"", b""), (b"", b"ACGTNNACGTACGT", b"IIIIIIII!!IIII")])
    (tmp_path / "r.fq").write_bytes(reads)
    (tmp_path / "q.fq").write_bytes(queries)
    rows = {}
    for tag, qfile, extra, qq in (("fq", "q.fq", (), 0), ("fa", "q.fa", (), 0), ("fq_masked", "q.fq", ("--query-min-base-quality", Q), Q),
                                  ("fa_masked", "q.fa", (), Q)):
        (tmp_path / "q.fa").write_bytes(F.fasta_twin(queries, qq, names=True))
        out = tmp_path / f"{tag}.tsv"
        r = _cli("--seq-in", tmp_path / "r.fq", "-k", K, "--query-fa", tmp_path / qfile, "--query-out", out, *extra)
        assert r.returncode == 0, r.stderr[-3000:]
        rows[tag] = out.read_text().splitlines()
    assert rows["fq"] == rows["fa"] and rows["fq_masked"] == rows["fa_masked"] and len(rows["fq"]) == 1 + 14
    assert rows["fq"] != rows["fq_masked"]  # masking a query changes its `valid` column
    assert rows["fq"][1].split("\t")[0] == "read0/1"


def test_error_exits(product_lib, tmp_path):
    (tmp_path / "twin.fa").write_bytes(b">r\nACGTACGTACGT\n")
    r = _cli("--seq-in", tmp_path / "twin.fa", "-k", K, "--min-base-quality", Q, "--unitigs-fa-out", tmp_path / "u.fa")
    assert r.returncode == 2 and "--min-base-quality needs a fastq file" in r.stderr, r.stderr[-2000:]
    bad = tmp_path / "bad.fq"
    bad.write_bytes(b"@r\nACGTACGTACGT\n+\nIIIIIIIIIIII\n@s\nACGTACGTACGT\n+\nIIII\n")
    r = _cli("--seq-in", bad, "-k", K, "--unitigs-fa-out", tmp_path / "u.fa")
    assert r.returncode == 2 and F.error_message(bad, 1, 8, F.BAD_LENGTH) in r.stderr, r.stderr[-2000:]
    assert not (tmp_path / "u.fa").exists()
    r = _cli("--seq-in", tmp_path / "twin.fa", "-k", K, "--query-fa", bad, "--query-out", tmp_path / "q.tsv")
    assert r.returncode == 2 and F.error_message(bad, 1, 8, F.BAD_LENGTH) in r.stderr, r.stderr[-2000:]
