"""`--components-out`, `--unitig-components-out` and `--min-component-kmers` through the CLI on the GPU: a counted and
cleaned `--seq-in` run over the reads of two unrelated genomes plus planted two-unitig clusters that are neither tip nor isolated
nor bubble; the same run with the filter, verified; its BCALM2 file read back; the same flags on `--fa-in`; and a run without the
new flags, byte for byte."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import unitig_components_ref as R
from matchtigs_amd import synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
K = 21
N = 200          # the threshold: above a planted cluster (110 k-mers), below a genome (about 480)
DUST = 3         # planted clusters: a ring of 60 k-mers with a tail of 50, each read twice
HEADER = "component\tfirst_unitig\tunitigs\tkmers\tbases\tabundance\tmean\tlinks\tdead_ends\tcircular\n"


def _cli(*a):
    return subprocess.run([sys.executable, "-m", "matchtigs_amd", *a], capture_output=True, text=True, cwd=str(ROOT), timeout=600)


def _fasta(path):
    return [l for l in Path(path).read_text().splitlines() if not l.startswith(">")]


def _reads():
    rng = np.random.default_rng(6)
    out = []
    for g in range(2):  # two genomes of 500 bases, tiled by reads of 100 every 10 bases, each given on both strands: abundance >= 2
        genome = synth.random_genome(500, seed=90 + g, haplotypes=1)[0]
        for at in range(0, 401, 10):
            out += [genome[at:at + 100], synth.revcomp(genome[at:at + 100])]
        for i in range(3):  # a read with one substitution near an end, once per strand: a tip above --min-abundance 2
            at = int(rng.integers(0, 401))
            r, j = list(genome[at:at + 100]), (4 + i if i % 2 else 95 - i)
            r[j] = "ACGT"[("ACGT".index(r[j]) + 1 + i % 3) % 4]
            out += ["".join(r), synth.revcomp("".join(r))]
        r = list(genome[200:300])  # and one seen once: its k-mers fall to --min-abundance 2
        r[50] = "ACGT"[("ACGT".index(r[50]) + 1) % 4]
        out.append("".join(r))
    for d in range(DUST):  # tail + ring + the ring's first k - 1 bases again: the ring closes, the tail hangs into it
        tail, ring = synth.random_genome(50, seed=70 + d, haplotypes=1)[0], synth.random_genome(60, seed=80 + d, haplotypes=1)[0]
        tail = tail[:-1] + "ACGT"[("ACGT".index(ring[-1]) + 1) % 4]  # the tail enters the ring by a k-mer of its own: 50 + 60 k-mers
        s = tail + ring + ring[:K - 1]
        out += [s, synth.revcomp(s)]
    return out


def _stderr_less_timings(text, d):
    text = text.replace(str(d), "DIR")
    return re.sub(r"\d+\.\d+ ?s\b", "Ts", text)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Three `--seq-in` runs of the same reads: `plain` without any new flag, `seen` with the two component outputs, `cut` with the
    filter, every output and `--verify`."""
    d = tmp_path_factory.mktemp("unitig_components_cli")
    (d / "reads.fa").write_text("".join(f">r{i}\n{r}\n" for i, r in enumerate(_reads())))
    base = ["--seq-in", str(d / "reads.fa"), "-k", str(K), "--min-abundance", "2", "--clip-tips", str(K), "--remove-isolated", str(K)]
    err = {}
    for name, extra in (("plain", []),
                        ("seen", ["--components-out", "c.tsv", "--unitig-components-out", "uc.txt"]),
                        ("cut", ["--components-out", "c.tsv.gz", "--unitig-components-out", "uc.txt", "--min-component-kmers", str(N), "--verify",
                                 "--greedytigs-fa-out", "g.fa"])):
        sub = d / name
        sub.mkdir()
        args = base + ["--unitigs-fa-out", str(sub / "u.fa"), "--unitigs-bcalm-out", str(sub / "u.bcalm.fa"), "--unitig-abundance-out",
                       str(sub / "ab.tsv"), "--unitig-kmer-abundance-out", str(sub / "kab.txt")]
        args += [str(sub / x) if x.endswith((".tsv", ".txt", ".gz", ".fa")) else x for x in extra]
        r = _cli(*args)
        print(r.stderr[-3000:])
        assert r.returncode == 0, r.stderr[-3000:]
        err[name] = _stderr_less_timings(r.stderr, sub)
    return d, err


def _kc(path):
    return [int(l.split("\t")[2]) for l in Path(path).read_text().splitlines()[1:]]


def test_without_the_filter_the_clusters_are_in_the_table(product_lib, runs):
    d, err = runs
    unitigs = _fasta(d / "seen" / "u.fa")
    want = R.components_of_sequences(unitigs, K, _kc(d / "seen" / "ab.tsv"))
    text = (d / "seen" / "c.tsv").read_text()
    assert text == R.components_tsv(want, K) and text.startswith(HEADER)
    rows = [l.split("\t") for l in text.splitlines()[1:]]
    dust = [r for r in rows if r[2] == "2" and r[3] == "110"]  # ring + tail: 60 + 50 k-mers
    assert len(dust) == DUST and all(r[8] == "1" and r[9] == "0" and r[4] == str(110 + 2 * (K - 1)) for r in dust)
    assert all(int(r[5]) == 2 * 110 for r in dust)  # every k-mer of a cluster was seen twice: abundance, not k-mers
    assert sum(1 for r in rows if int(r[3]) >= N) == 2  # the two genomes
    lines = (d / "seen" / "uc.txt").read_text().splitlines()
    assert len(lines) == len(unitigs) and [int(x) for x in lines] == want["component_of"]
    assert re.search(rf"Writing components took Ts \({len(rows)} components, largest ", err["seen"])


def test_with_the_filter_they_are_gone_and_verify_counts_them(product_lib, runs):
    import gzip

    d, err = runs
    before = _fasta(d / "seen" / "u.fa")
    kept, keep = R.filtered_sequences(before, K, N)
    unitigs = _fasta(d / "cut" / "u.fa")
    assert unitigs == kept and len(before) - len(kept) == 2 * DUST
    kc = [v for v, f in zip(_kc(d / "seen" / "ab.tsv"), keep) if f]
    assert _kc(d / "cut" / "ab.tsv") == kc  # the abundance files are written after the filter
    kab_before = (d / "seen" / "kab.txt").read_text().splitlines()
    assert (d / "cut" / "kab.txt").read_text().splitlines() == [l for l, f in zip(kab_before, keep) if f]
    want = R.components_of_sequences(unitigs, K, kc)
    assert gzip.decompress((d / "cut" / "c.tsv.gz").read_bytes()).decode() == R.components_tsv(want, K)
    assert all(m >= N for m in want["kmers"]) and len(want["kmers"]) == 2
    assert [int(x) for x in (d / "cut" / "uc.txt").read_text().splitlines()] == want["component_of"]
    m = re.search(r"Component filter: (\d+) of (\d+) components have fewer than 200 k-mers: (\d+) unitigs, (\d+) k-mers removed, (\d+) unitigs left", err["cut"])
    assert m and [int(x) for x in m.groups()] == [DUST, DUST + 2, 2 * DUST, 110 * DUST, len(kept)]
    v = re.search(r"Verifying component filter: (\d+) of the input's (\d+) distinct k-mers are in the unitigs, (\d+) are not \((\d+) dropped by the "
                  r"abundance filter, (\d+) cleaned away, (\d+) in components of fewer than 200 k-mers\), 0 foreign: as counted", err["cut"])
    assert v, err["cut"][-3000:]
    inside, total, missing, dropped, cleaned, small = [int(x) for x in v.groups()]
    assert small == 110 * DUST and dropped > 0 and cleaned > 0 and missing == dropped + cleaned + small and inside + missing == total
    assert inside == sum(want["kmers"])
    assert "MISMATCH" not in err["cut"] and re.search(r"Verifying greedytigs .*k-mer sets equal", err["cut"])
    # KC of the filtered BCALM2 file: the kept unitigs' sums
    heads = [l for l in (d / "cut" / "u.bcalm.fa").read_text().splitlines() if l.startswith(">")]
    assert [int(re.search(r"KC:i:(\d+)", h).group(1)) for h in heads] == kc


def test_the_filtered_file_feeds_bcalm_in(product_lib, runs):
    d, _ = runs
    r = _cli("--bcalm-in", str(d / "cut" / "u.bcalm.fa"), "-k", str(K), "--greedytigs-fa-out", str(d / "t.fa"), "--verify", "--components-out",
             str(d / "again.tsv"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert re.search(r"Verifying greedytigs .*k-mer sets equal", r.stderr)
    unitigs = _fasta(d / "cut" / "u.fa")
    assert (d / "again.tsv").read_text() == R.components_tsv(R.components_of_sequences(unitigs, K), K)  # nothing counted: abundance = k-mers


def test_fa_in_takes_the_same_flags(product_lib, runs):
    d, _ = runs
    r = _cli("--fa-in", str(d / "seen" / "u.fa"), "-k", str(K), "--min-component-kmers", str(N), "--components-out", str(d / "fa.tsv"),
             "--unitig-components-out", str(d / "fa.txt"), "--unitigs-fa-out", str(d / "fa.fa"), "--greedytigs-fa-out", str(d / "fa.g.fa"), "--verify")
    assert r.returncode == 0, r.stderr[-3000:]
    kept, _ = R.filtered_sequences(_fasta(d / "seen" / "u.fa"), K, N)
    assert _fasta(d / "fa.fa") == kept
    want = R.components_of_sequences(kept, K)
    assert (d / "fa.tsv").read_text() == R.components_tsv(want, K)
    assert [int(x) for x in (d / "fa.txt").read_text().splitlines()] == want["component_of"]
    assert re.search(rf"Verifying component filter: .*\(0 dropped by the abundance filter, 0 cleaned away, {110 * DUST} in components of fewer than "
                     r"200 k-mers\), 0 foreign: as counted", r.stderr), r.stderr[-3000:]
    assert re.search(r"Verifying greedytigs .*k-mer sets equal", r.stderr)
    none = _cli("--fa-in", str(d / "seen" / "u.fa"), "-k", str(K), "--min-component-kmers", "100000", "--unitigs-fa-out", str(d / "none.fa"))
    assert none.returncode == 1 and "nothing is left after the component filter" in none.stderr


def test_a_run_without_the_new_flags_is_unchanged(product_lib, runs):
    """`plain` and `seen` differ only in the two component outputs: the same files, byte for byte, and the same stderr less the
    timings and the one line that reports the components."""
    d, err = runs
    for name in ("u.fa", "u.bcalm.fa", "ab.tsv", "kab.txt"):
        assert (d / "plain" / name).read_bytes() == (d / "seen" / name).read_bytes(), name
    seen = [l for l in err["seen"].splitlines() if not l.startswith("Writing components took")]
    assert err["plain"].splitlines() == seen and len(seen) + 1 == len(err["seen"].splitlines())
    assert "omponent" not in err["plain"]
