"""`--bubbles-out` and `--bubbles-max-kmers` through the CLI on the GPU: the reads of two haplotypes that differ in three
SNPs and a two-base deletion, as two `--seq-in` files, counted, cleaned and popped with `--bubble-ratio 4`, so that an error seen
twice goes and the variation stays and is called with its carriers; the same on `--fa-in`; and a run without the new flags, byte
for byte."""
import gzip
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import unitig_bubbles_ref as UB
from matchtigs_amd import synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
K = 21
SNPS = (300, 600, 900)
HEAD = "bubble\tarm\tunitig\tstrand\tkmers\tabundance\tmean\ttype\tpos\tref\talt\tdifferences"


def _cli(*a):
    return subprocess.run([sys.executable, "-m", "matchtigs_amd", *a], capture_output=True, text=True, cwd=str(ROOT), timeout=600)


def _other(c, step=1):
    return "ACGT"[("ACGT".index(c) + step) % 4]


def _haplotypes():
    """(a, b, d): b is a with the bases at SNPS changed and the two bases at d gone, d chosen where the deletion can be placed in one
    way only (a[d - 1] != a[d + 1] and a[d] != a[d + 2])."""
    a = synth.random_genome(1500, seed=41, haplotypes=1)[0]
    d = next(i for i in range(1200, 1300) if a[i - 1] != a[i + 1] and a[i] != a[i + 2])
    b = list(a)
    for p in SNPS:
        b[p] = _other(a[p])
    return a, "".join(b[:d] + b[d + 2:]), d


def _tiled(genome, starts):
    return [r for at in starts for r in (genome[at:at + 100], synth.revcomp(genome[at:at + 100]))]


def _reads():
    """File a: reads of 100 bases of haplotype a every 5 bases, on both strands, plus one read with a substitution in its middle,
    once per strand (an error seen twice: it passes --min-abundance 2 and is a bubble of mean 2 beside some 30). File b: haplotype b
    every 10 bases, so that a's arm of a site has about twice the mean of b's: a is the reference allele, and 2 < 4 keeps b's."""
    a, b, _ = _haplotypes()
    reads_a = _tiled(a, range(0, len(a) - 99, 5))
    wrong = list(a[100:200])
    wrong[50] = _other(wrong[50], 2)
    reads_a += ["".join(wrong), synth.revcomp("".join(wrong))]
    return reads_a, _tiled(b, range(0, len(b) - 99, 10))


def _fasta(path):
    return [l for l in Path(path).read_text().splitlines() if not l.startswith(">")]


def _stderr_less_timings(text, d):
    text = text.replace(str(d), "DIR")
    return re.sub(r"\d+\.\d+ ?s\b", "Ts", text)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Two `--seq-in` runs of the same two files: `plain` without the new flags, `called` with `--bubbles-out`."""
    d = tmp_path_factory.mktemp("unitig_bubbles_cli")
    for name, reads in zip(("a.fa", "b.fa"), _reads()):
        (d / name).write_text("".join(f">r{i}\n{r}\n" for i, r in enumerate(reads)))
    base = ["--seq-in", str(d / "a.fa"), "--seq-in", str(d / "b.fa"), "-k", str(K), "--min-abundance", "2", "--clip-tips", str(K), "--pop-bubbles",
            str(2 * K), "--bubble-ratio", "4"]
    err = {}
    for name, extra in (("plain", []), ("called", ["--bubbles-out", "calls.tsv"])):
        sub = d / name
        sub.mkdir()
        args = base + ["--unitigs-fa-out", str(sub / "u.fa"), "--unitig-abundance-out", str(sub / "ab.tsv"), "--unitig-colors-out", str(sub / "col.txt"),
                       "--unitigs-gfa-out", str(sub / "u.gfa")]
        args += [str(sub / x) if x.endswith(".tsv") else x for x in extra]
        r = _cli(*args)
        print(r.stderr[-3000:])
        assert r.returncode == 0, r.stderr[-3000:]
        err[name] = _stderr_less_timings(r.stderr, sub)
    return d, err


def _masks(path):
    """The per-k-mer masks of `--unitig-colors-out`: runs `count:hexmask` per unitig."""
    return [int(m, 16) for line in Path(path).read_text().splitlines() for run in line.split() for n, m in [run.split(":")] for _ in range(int(n))]


def test_the_four_sites_are_called_with_their_carriers(product_lib, runs):
    d, err = runs
    a, b, at = _haplotypes()
    text = (d / "called" / "calls.tsv").read_text()
    rows = [l.split("\t") for l in text.splitlines()]
    assert rows[0] == HEAD.split("\t") + ["a.fa", "b.fa"] and len(rows) == 1 + 2 * 4
    unitigs = _fasta(d / "called" / "u.fa")
    want = {("snp", a[p], _other(a[p])) for p in SNPS} | {("del", a[at:at + 2], "-")}
    got = set()
    for ref_row, alt_row in zip(rows[1::2], rows[2::2]):
        assert ref_row[1] == "0" and ref_row[7:12] == ["ref", ".", ".", ".", "0"] and alt_row[1] == "1" and ref_row[0] == alt_row[0]
        kind, pos, ref, alt = alt_row[7], int(alt_row[8]), alt_row[9], alt_row[10]
        record = unitigs[int(ref_row[2])]
        assert ref == "-" or record[pos:pos + len(ref)] == ref  # pos is 0-based on the reference arm's record as written
        if record not in a:  # the record is written on the other strand: read the call on a's
            assert synth.revcomp(record) in a
            ref, alt = ("-" if x == "-" else synth.revcomp(x) for x in (ref, alt))
        got.add((kind, ref, alt))
        # every k-mer of a's allele is in file a alone, every k-mer of b's in file b alone
        assert ref_row[12:] == [ref_row[4], "0"] and alt_row[12:] == ["0", alt_row[4]], (ref_row, alt_row)
        assert alt_row[11] == ("1" if kind == "snp" else "0")
        assert float(ref_row[6]) > float(alt_row[6]) > float(ref_row[6]) / 4  # the reference weighs more, and not four times more
    assert got == want
    assert sorted(int(r[4]) for r in rows[1:]) == [K - 1] + [K] * 6 + [K + 1]  # a SNP's arms have k k-mers, the deletion's k + 1 and k - 1
    line, = [l for l in err["called"].splitlines() if l.startswith("Bubbles: ")]
    assert line.startswith("Bubbles: 4 bubbles, 8 arms: 3 snp, 0 mnp, 0 ins, 1 del, 0 complex; the largest has 2 arms")


def test_the_error_is_popped_and_the_file_is_the_apis(product_lib, runs):
    from matchtigs_amd import api

    d, _ = runs
    unitigs = _fasta(d / "called" / "u.fa")
    wrong = _reads()[0][-2]
    assert not any(wrong[50 - K + 1:50 + K] in u or synth.revcomp(wrong[50 - K + 1:50 + K]) in u for u in unitigs)
    kc = [int(l.split("\t")[2]) for l in (d / "called" / "ab.tsv").read_text().splitlines()[1:]]
    masks = _masks(d / "called" / "col.txt")
    assert len(kc) == len(unitigs) and len(masks) == sum(len(u) - K + 1 for u in unitigs)
    graph = api.Bigraph.from_sequences(unitigs, K)
    found = api.unitig_bubbles(graph, unitigs, K, 2 * K, kc=kc, kmer_colors=np.array(masks, np.uint64), n_colors=2)
    text = (d / "called" / "calls.tsv").read_text()
    assert text == found.tsv(unitigs, K, ["a.fa", "b.fa"])
    assert text == UB.bubbles_tsv(UB.bubbles_of_sequences(unitigs, K, 2 * K, kc, masks, 2), ["a.fa", "b.fa"])


def test_the_limit_and_gzip(product_lib, runs):
    d, _ = runs
    base = ["--seq-in", str(d / "a.fa"), "--seq-in", str(d / "b.fa"), "-k", str(K), "--min-abundance", "2", "--clip-tips", str(K), "--pop-bubbles",
            str(2 * K), "--bubble-ratio", "4"]
    r = _cli(*base, "--bubbles-out", str(d / "short.tsv.gz"), "--bubbles-max-kmers", str(K))  # fewer than k k-mers: only the deletion's arm
    assert r.returncode == 0, r.stderr[-3000:]
    assert gzip.decompress((d / "short.tsv.gz").read_bytes()).decode() == HEAD + "\ta.fa\tb.fa\n"
    assert "Bubbles: 0 bubbles, 0 arms" in r.stderr
    r = _cli(*base, "--bubbles-out", str(d / "next.tsv"), "--bubbles-max-kmers", str(K + 2))  # the longest arm has k + 1
    assert r.returncode == 0 and (d / "next.tsv").read_text() == (d / "called" / "calls.tsv").read_text()


def test_fa_in_takes_the_flag_without_carriers(product_lib, runs):
    d, _ = runs
    r = _cli("--fa-in", str(d / "called" / "u.fa"), "-k", str(K), "--bubbles-out", str(d / "fa.tsv"))
    assert r.returncode == 0, r.stderr[-3000:]
    unitigs = _fasta(d / "called" / "u.fa")
    text = (d / "fa.tsv").read_text()
    assert text == UB.bubbles_tsv(UB.bubbles_of_sequences(unitigs, K, 2 * K))  # nothing counted: abundance = k-mers
    rows = [l.split("\t") for l in text.splitlines()]
    assert rows[0] == HEAD.split("\t") and len(rows) == 9 and all(r[4] == r[5] and r[6] == "1.0" for r in rows[1:])
    kinds = [r[7] for r in rows[1:]]  # (all means are 1.0: the smaller unitig of a site is its reference, so the deletion may read as an insertion)
    assert kinds.count("ref") == 4 and kinds.count("snp") == 3 and kinds.count("del") + kinds.count("ins") == 1
    assert "Bubbles: 4 bubbles, 8 arms" in r.stderr


def test_with_the_component_filter_the_masks_follow_the_kept_unitigs(product_lib, runs):
    """Three ring-with-tail clusters of 110 k-mers in front of file a's reads: `--min-component-kmers 200` removes them, the unitigs
    behind them move up, and the calls -- the carriers among them, which come from the per-k-mer masks of the unfiltered store --
    are those of the run without the filter, row for row once the unitig's number is replaced by its record."""
    d, _ = runs
    dust = []
    for i in range(3):  # tail + ring + the ring's first k - 1 bases again, once per strand (tests/test_unitig_components_cli.py)
        tail, ring = synth.random_genome(50, seed=70 + i, haplotypes=1)[0], synth.random_genome(60, seed=80 + i, haplotypes=1)[0]
        s = tail[:-1] + _other(ring[-1]) + ring + ring[:K - 1]
        dust += [s, synth.revcomp(s)]
    (d / "c.fa").write_text("".join(f">r{i}\n{r}\n" for i, r in enumerate(dust + _reads()[0])))
    base = ["--seq-in", str(d / "c.fa"), "--seq-in", str(d / "b.fa"), "-k", str(K), "--min-abundance", "2", "--clip-tips", str(K), "--pop-bubbles",
            str(2 * K), "--bubble-ratio", "4"]
    rows, unitigs = {}, {}
    for name, extra in (("whole", []), ("cut", ["--min-component-kmers", "200"])):
        r = _cli(*base, *extra, "--unitigs-fa-out", str(d / f"{name}.fa"), "--bubbles-out", str(d / f"{name}.tsv"))
        assert r.returncode == 0, r.stderr[-3000:]
        unitigs[name] = _fasta(d / f"{name}.fa")
        rows[name] = [l.split("\t") for l in (d / f"{name}.tsv").read_text().splitlines()]
        assert rows[name][0] == HEAD.split("\t") + ["c.fa", "b.fa"] and len(rows[name]) == 9
    assert "Component filter: 3 of 4 components have fewer than 200 k-mers: 6 unitigs, 330 k-mers removed" in r.stderr
    gone = [i for i, u in enumerate(unitigs["whole"]) if u not in unitigs["cut"]]
    assert len(gone) == 6 and unitigs["cut"] == [u for u in unitigs["whole"] if u in unitigs["cut"]]
    arms = [int(r[2]) for r in rows["whole"][1:]]
    assert min(gone) < min(arms)  # every arm's number, and the place of its masks, changes
    named = {name: [r[:2] + [unitigs[name][int(r[2])]] + r[3:] for r in rows[name][1:]] for name in rows}
    assert named["cut"] == named["whole"] and [int(r[2]) for r in rows["cut"][1:]] != arms
    assert all(r[12:] in ([r[4], "0"], ["0", r[4]]) for r in rows["cut"][1:])


def test_a_run_without_the_new_flags_is_unchanged(product_lib, runs):
    """`plain` and `called` differ only in `--bubbles-out`: the same files, byte for byte, and the same stderr less the timings and the
    one line that reports the bubbles."""
    d, err = runs
    for name in ("u.fa", "ab.tsv", "col.txt", "u.gfa"):
        assert (d / "plain" / name).read_bytes() == (d / "called" / name).read_bytes(), name
    called = [l for l in err["called"].splitlines() if not l.startswith("Bubbles: ")]
    assert err["plain"].splitlines() == called and len(called) + 1 == len(err["called"].splitlines())
    assert "Bubbles: " not in err["plain"] and not (d / "plain" / "calls.tsv").exists()
