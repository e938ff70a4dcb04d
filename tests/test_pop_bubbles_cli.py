"""`--pop-bubbles` and `--bubble-ratio`: the entry points and structs of the C-ABI, the flags' argument rules in a child
process, and on the GPU a run through the CLI against the API, with the cleaning's verification line naming the arms' k-mers, and the
same input without the flag."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from matchtigs_amd import _lib, synth

ROOT = Path(__file__).resolve().parent.parent
K = 21
ENTRY_POINTS = ("mtg_compact_unitigs_simplified", "mtg_compact_unitigs_simplified_store", "mtg_last_bubble_times")


def _cli(*a):
    return subprocess.run([sys.executable, "-m", "matchtigs_amd", *a], capture_output=True, text=True, cwd=str(ROOT), timeout=600)


def _fasta(path):
    return [l for l in Path(path).read_text().splitlines() if not l.startswith(">")]


def test_entry_points_are_declared_and_exported(product_lib):
    names = _lib.declared_symbols()
    for n in ENTRY_POINTS:
        assert n in names and hasattr(product_lib, n), n
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert set(ENTRY_POINTS) <= {l.split()[-1] for l in out.splitlines() if l.strip()}  # unmangled => extern "C"
    from matchtigs_amd import api

    for n in ("compact_unitigs_simplified", "Bubbles", "last_bubble_times"):
        assert hasattr(api, n), n
    assert api.Bubbles(2, 42, 50).describe() == "2 bubble arms of 42 k-mers popped"


def test_struct_sizes(tmp_path):
    assert C.sizeof(_lib.MtgBubbleParams) == 16 and C.sizeof(_lib.MtgBubbles) == 24
    assert [f for f, _ in _lib.MtgBubbleParams._fields_] == ["max_arm_kmers", "min_ratio"]
    assert [f for f, _ in _lib.MtgBubbles._fields_] == ["arms", "arm_kmers", "removed_occurrences"]
    assert C.sizeof(_lib.MtgCleaningParams) == 24 and C.sizeof(_lib.MtgCleaning) == 48  # (as they were)
    src = tmp_path / "t.c"
    src.write_text('#include "mtg_engine.h"\n'
                   "int main(void){return sizeof(mtg_bubble_params) == 16 && sizeof(mtg_bubbles) == 24 && sizeof(mtg_cleaning) == 48 ? 0 : 1;}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", str(ROOT / "include"), str(src), "-o", str(tmp_path / "t")], check=True)
    subprocess.run([str(tmp_path / "t")], check=True)


@pytest.mark.parametrize("route, flags, message", [
    ("--fa-in", ("--pop-bubbles", "42"), "--pop-bubbles needs --seq-in"),
    ("--fa-in", ("--pop-bubbles", "42", "--bubble-ratio", "2"), "needs --seq-in"),
    ("--seq-in", ("--pop-bubbles", "1"), "--pop-bubbles must be >= 2"),
    ("--seq-in", ("--bubble-ratio", "2"), "--bubble-ratio needs --pop-bubbles"),
    ("--seq-in", ("--pop-bubbles", "42", "--bubble-ratio", "0"), "--bubble-ratio must be in 1..255"),
    ("--seq-in", ("--pop-bubbles", "42", "--bubble-ratio", "256"), "--bubble-ratio must be in 1..255"),
    ("--seq-in", ("--clean-rounds", "2"), "--clean-rounds needs --clip-tips or --remove-isolated"),
    ("--seq-in", ("--clean-rounds", "65", "--pop-bubbles", "22"), "--clean-rounds must be in 1..64"),
])
def test_the_flags_rules(tmp_path, route, flags, message):
    r = _cli(route, str(tmp_path / "none.fa"), "-k", str(K), "--unitigs-fa-out", str(tmp_path / "x.fa"), *flags)
    assert r.returncode == 2 and message in r.stderr, r.stderr[-2000:]


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    """40 reads of 150 bases from a 600-base genome (10x), either strand, about 1 % substitutions, plus 6 reads given twice, once per
    strand, with one substitution in the middle (a bubble that passes --min-abundance 2) and 4 with one near an end (a tip)."""
    rng = np.random.default_rng(5)
    genome = synth.random_genome(600, seed=78, haplotypes=1)[0]
    out = []
    for i in range(40):
        at = int(rng.integers(0, 600 - 150 + 1))
        r = list(genome[at:at + 150])
        for j in np.flatnonzero(rng.random(150) < 0.01):
            r[j] = "ACGT"[("ACGT".index(r[j]) + int(rng.integers(1, 4))) % 4]
        r = "".join(r)
        out.append(synth.revcomp(r) if rng.random() < 0.5 else r)
    for i in range(10):
        at = int(rng.integers(0, 600 - 150 + 1))
        r, j = list(genome[at:at + 150]), (60 + 5 * i if i < 6 else (5 if i % 2 else 144))
        r[j] = "ACGT"[("ACGT".index(r[j]) + 1 + i % 3) % 4]
        out += ["".join(r), synth.revcomp("".join(r))]
    d = tmp_path_factory.mktemp("pop_bubbles_cli")
    (d / "reads.fa").write_text("".join(f">r{i}\n{r[:80]}\n{r[80:]}\n" for i, r in enumerate(out)))
    return d, out


@pytest.mark.gpu
def test_clean_rounds_go_with_pop_bubbles(product_lib, reads):
    d, _ = reads
    r = _cli("--seq-in", str(d / "reads.fa"), "-k", str(K), "--clean-rounds", "2", "--pop-bubbles", "22", "--unitigs-fa-out", str(d / "u2.fa"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert " bubble arms of " in re.search(r"Loaded .*", r.stderr).group(0)


@pytest.mark.gpu
def test_simplified_run(product_lib, reads):
    import bubble_ref as B
    from matchtigs_amd import api

    d, seqs = reads
    r = _cli("--seq-in", str(d / "reads.fa"), "-k", str(K), "--min-abundance", "2", "--clip-tips", str(K), "--pop-bubbles", str(2 * K), "--clean-rounds", "3",
             "--unitigs-fa-out", str(d / "u.fa"), "--verify")
    print(r.stderr[-3000:])
    assert r.returncode == 0, r.stderr[-3000:]
    want = B.compact_simplified(seqs, K, pop_bubbles=2 * K, clip_tips=K, rounds=3, m=2)
    store, c, a, _, _, cl, bu = api.compact_unitigs_simplified(seqs, K, 2 * K, 1, K, 0, 3, 2)
    assert _fasta(d / "u.fa") == store.sequences() == want[0] and cl == api.Cleaning(**want[6]) and bu == api.Bubbles(**want[7])
    assert bu.arms > 0 and cl.tips > 0 and a.dropped > 0
    clean = re.search(r"Verifying cleaning: .*", r.stderr).group(0)
    assert clean.endswith("as counted") and "MISMATCH" not in r.stderr
    assert (f"{a.dropped + cl.removed_kmers + bu.arm_kmers} are not ({a.dropped} dropped by the filter, {cl.tip_kmers} in tips, "
            f"{cl.isolated_kmers} in isolated unitigs, {bu.arm_kmers} in bubble arms), 0 foreign") in clean
    loaded = re.search(r"Loaded .*", r.stderr).group(0)
    assert cl.describe() + "; " + bu.describe() in loaded and c.describe() in loaded
    # the same input without the flag: no word of bubbles, the cleaning line in its old shape, more unitigs
    r = _cli("--seq-in", str(d / "reads.fa"), "-k", str(K), "--min-abundance", "2", "--clip-tips", str(K), "--clean-rounds", "3",
             "--unitigs-fa-out", str(d / "u_tips.fa"), "--verify")
    assert r.returncode == 0, r.stderr[-3000:]
    assert "bubble" not in r.stderr
    old = api.compact_unitigs_cleaned(seqs, K, K, 0, 3, 2)
    assert _fasta(d / "u_tips.fa") == old[0].sequences() and len(old[0]) > len(store)
    assert (f"{old[2].dropped + old[5].removed_kmers} are not ({old[2].dropped} dropped by the filter, {old[5].tip_kmers} in tips, "
            f"{old[5].isolated_kmers} in isolated unitigs), 0 foreign: as counted") in r.stderr
