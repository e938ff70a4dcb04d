"""`--clip-tips`, `--remove-isolated`, `--clean-rounds` through the CLI on the GPU: the unitig file against the API and
the restatement (tip_clip_ref.py), both verification lines, greedytigs that equal those of `--fa-in` on the written unitigs, fewer
unitigs than without the flags, the flags' argument rules, a run that cleans everything away, and a run without the new flags."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import tip_clip_ref as T
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
    """test_abundance_cli.py's reads -- 40 of 150 bases from a 600-base genome (10x), either strand, about 1 % substitutions, lower
    case here and there -- plus 6 reads given twice, once per strand, with one substitution 5 .. 10 bases from an end."""
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
    for i in range(6):  # an error near a read end that is seen twice: it passes --min-abundance 2 and stays as a tip
        at = int(rng.integers(0, 600 - 150 + 1))
        r, j = list(genome[at:at + 150]), (4 + i if i % 2 else 145 - i)
        r[j] = "ACGT"[("ACGT".index(r[j]) + 1 + i % 3) % 4]
        out += ["".join(r), synth.revcomp("".join(r))]
    d = tmp_path_factory.mktemp("clip_tips_cli")
    (d / "reads.fa").write_text("".join(f">r{i}\n{r[:80]}\n{r[80:]}\n" for i, r in enumerate(out)))
    (d / "short.fa").write_text(f">s\n{genome[:K + 5]}\n")
    return d, out


def test_cleaned_run(product_lib, reads):
    from matchtigs_amd import api

    d, seqs = reads
    p = {n: str(d / n) for n in ("reads.fa", "u.fa", "g.fa", "g2.fa", "u_plain.fa")}
    r = _cli("--seq-in", p["reads.fa"], "-k", str(K), "--min-abundance", "2", "--clip-tips", str(K), "--remove-isolated", str(K), "--clean-rounds", "3",
             "--unitigs-fa-out", p["u.fa"], "--greedytigs-fa-out", p["g.fa"], "--verify")
    print(r.stderr[-3000:])
    assert r.returncode == 0, r.stderr[-3000:]
    unitigs, stats, _, ab, _, _, cleaning = T.compact_cleaned(seqs, K, clip_tips=K, remove_isolated=K, rounds=3, m=2)
    assert cleaning["tips"] > 0 and ab["dropped"] > 0
    # the unitig file is the API's store and the restatement's
    store, c, a, _, _, cl = api.compact_unitigs_cleaned(seqs, K, K, K, 3, 2)
    assert _fasta(p["u.fa"]) == store.sequences() == unitigs and cl == api.Cleaning(**cleaning)
    # both verification lines say what was counted, and the Loaded line tells what the cleaning did
    gone = cleaning["tip_kmers"] + cleaning["isolated_kmers"]
    filt = re.search(r"Verifying abundance filter: .*", r.stderr).group(0)
    clean = re.search(r"Verifying cleaning: .*", r.stderr).group(0)
    assert filt.endswith("as counted") and clean.endswith("as counted") and "MISMATCH" not in r.stderr
    assert f"{ab['dropped']} are not ({ab['dropped']} dropped by the filter), 0 foreign" in filt
    assert (f"{ab['dropped'] + gone} are not ({ab['dropped']} dropped by the filter, {cleaning['tip_kmers']} in tips, "
            f"{cleaning['isolated_kmers']} in isolated unitigs), 0 foreign") in clean
    assert re.search(r"Verifying greedytigs .*k-mer sets equal", r.stderr)
    loaded = re.search(r"Loaded .*", r.stderr).group(0)
    assert cl.describe() in loaded and c.describe() in loaded and a.describe() in loaded
    # the greedytigs equal those of --fa-in on the written unitigs, byte for byte
    r = _cli("--fa-in", p["u.fa"], "-k", str(K), "--greedytigs-fa-out", p["g2.fa"])
    assert r.returncode == 0, r.stderr[-3000:]
    assert Path(p["g.fa"]).read_bytes() == Path(p["g2.fa"]).read_bytes()
    # fewer unitigs than without the flags
    r = _cli("--seq-in", p["reads.fa"], "-k", str(K), "--min-abundance", "2", "--unitigs-fa-out", p["u_plain.fa"])
    assert r.returncode == 0 and len(_fasta(p["u_plain.fa"])) > len(unitigs)
    assert "Verifying cleaning" not in r.stderr and " tips of " not in r.stderr


def test_cleaning_alone_verifies_against_the_unitigs(product_lib, reads):
    d, seqs = reads
    r = _cli("--seq-in", str(d / "reads.fa"), "-k", str(K), "--clip-tips", str(K), "--unitigs-fa-out", str(d / "u1.fa"), "--eulertigs-fa-out",
             str(d / "e1.fa"), "--verify")
    assert r.returncode == 0, r.stderr[-3000:]
    unitigs, _, _, _, _, _, cleaning = T.compact_cleaned(seqs, K, clip_tips=K)
    assert _fasta(d / "u1.fa") == unitigs and cleaning["rounds_run"] == 1
    assert "Verifying abundance filter" not in r.stderr and re.search(r"Verifying cleaning: .*as counted", r.stderr)
    assert f"(0 dropped by the filter, {cleaning['tip_kmers']} in tips, 0 in isolated unitigs)" in r.stderr
    assert re.search(r"Verifying eulertigs .*k-mer sets equal", r.stderr)


@pytest.mark.parametrize("flags, message", [
    (("--clip-tips", "21"), "--clip-tips needs --seq-in"),
    (("--remove-isolated", "21"), "--remove-isolated needs --seq-in"),
    (("--clean-rounds", "2", "--clip-tips", "21"), "needs --seq-in"),
])
def test_the_flags_need_seq_in(product_lib, reads, flags, message):
    d, _ = reads
    r = _cli("--fa-in", str(d / "reads.fa"), "-k", str(K), "--unitigs-fa-out", str(d / "x.fa"), *flags)
    assert r.returncode == 2 and message in r.stderr, r.stderr[-2000:]


@pytest.mark.parametrize("flags, message", [
    (("--clean-rounds", "2"), "--clean-rounds needs --clip-tips or --remove-isolated"),
    (("--clip-tips", "1"), "--clip-tips must be >= 2"),
    (("--remove-isolated", "0"), "--remove-isolated must be >= 1"),
    (("--clip-tips", "21", "--clean-rounds", "65"), "--clean-rounds must be in 1..64"),
])
def test_the_flags_rules(product_lib, reads, flags, message):
    d, _ = reads
    r = _cli("--seq-in", str(d / "reads.fa"), "-k", str(K), "--unitigs-fa-out", str(d / "x.fa"), *flags)
    assert r.returncode == 2 and message in r.stderr, r.stderr[-2000:]


def test_everything_is_cleaned_away(product_lib, reads):
    d, _ = reads
    spec, u = d / "spec_s.tsv", d / "u_s.fa"
    r = _cli("--seq-in", str(d / "short.fa"), "-k", str(K), "--remove-isolated", "100", "--unitigs-fa-out", str(u), "--kmer-spectrum-out", str(spec))
    assert r.returncode == 1 and "nothing is left after cleaning" in r.stderr, r.stderr[-3000:]
    assert "0 tips of 0 k-mers and 1 isolated unitigs of 6 k-mers removed in 1 rounds" in r.stderr
    assert spec.read_text().splitlines() == ["abundance\tkmers", "1\t6"]
    assert not u.exists() and "Loaded" not in r.stderr


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
    assert "cleaning" not in r.stderr and "tips" not in r.stderr
