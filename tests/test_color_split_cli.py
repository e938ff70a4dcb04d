"""`--monochromatic-unitigs`, `--color-classes-out`, `--unitig-color-classes-out` through the CLI on the GPU, on the
files of test_kmer_color_cli.py: three `--seq-in` files (FASTA, gzipped FASTQ cut by `--min-base-quality`, FASTA) and two; every file
written is checked line for line against the restatement (color_split_ref.py); the tig algorithms take the split unitigs and
`--verify` holds them to the input; a run without the new flags writes what the restatement of DESIGN.md 22 says; and the flags
without `--seq-in`, or with 65 files, are errors of the command line."""
import re
from pathlib import Path

import pytest

import color_split_ref as S
import kmer_color_ref as KC
from matchtigs_amd import api
from test_kmer_color_cli import K, Q, _cli, _fasta, _lines, inputs  # noqa: F401 (inputs: the fixture)

pytestmark = pytest.mark.gpu


def _classes_line(stderr):
    line = [l for l in stderr.splitlines() if l.startswith("Colour classes: ")]
    assert len(line) == 1
    return line[0]


def _want_line(classes):
    top = max(range(len(classes["masks"])), key=lambda c: (classes["kmers"][c], -c))
    return (f"Colour classes: {len(classes['masks'])} classes in {classes['n_runs']} runs, the largest class {top} (mask {classes['masks'][top]:x}, "
            f"{bin(classes['masks'][top]).count('1')} carriers) with {classes['kmers'][top]} of {sum(classes['kmers'])} k-mers")


def test_three_files_unsplit_and_split(product_lib, inputs):
    d, records, colors, _, _ = inputs
    names = [str(d / n) for n in ("a.fa", "b.fq.gz", "c.fa")]
    common = ["--seq-in", names[0], "--seq-in", names[1], "--seq-in", names[2], "-k", K, "--min-base-quality", Q]
    p = {n: str(d / ("split_" + n)) for n in ("cl.tsv", "ucc.txt", "uc.txt", "u.fa", "cl1.tsv.gz", "ucc1.txt.gz", "uc1.txt", "u1.fa", "ab1.tsv")}
    r = _cli(*common, "--color-classes-out", p["cl.tsv"], "--unitig-color-classes-out", p["ucc.txt"], "--unitig-colors-out", p["uc.txt"],
             "--unitigs-fa-out", p["u.fa"])
    print(r.stderr[-3000:])
    assert r.returncode == 0, r.stderr[-3000:]
    unitigs, stats, _, ab, col, classes = S.compact_classes(records, colors, 3, K)
    assert _fasta(p["u.fa"]) == unitigs and _lines(p["cl.tsv"]) == S.class_lines(classes) and len(classes["masks"]) >= 4
    assert _lines(p["ucc.txt"]) == S.unitig_class_lines(unitigs, classes["kmer_class"], K) and any(" " in l for l in _lines(p["ucc.txt"]))
    assert _lines(p["uc.txt"]) == KC.unitig_color_lines(unitigs, col["kmer_colors"], K)
    assert sum(len(l.split()) for l in _lines(p["uc.txt"])) == classes["n_runs"] == sum(classes["runs"])
    assert _classes_line(r.stderr) == _want_line(classes) and "monochromatic" not in r.stderr
    # the split: every output sees the split unitigs
    r1 = _cli(*common, "--monochromatic-unitigs", "--color-classes-out", p["cl1.tsv.gz"], "--unitig-color-classes-out", p["ucc1.txt.gz"],
              "--unitig-colors-out", p["uc1.txt"], "--unitigs-fa-out", p["u1.fa"], "--unitig-abundance-out", p["ab1.tsv"])
    print(r1.stderr[-3000:])
    assert r1.returncode == 0, r1.stderr[-3000:]
    s_unitigs, s_stats, _, s_ab, s_col, s_classes = S.compact_classes(records, colors, 3, K, 1, True)
    assert len(s_unitigs) > len(unitigs) and _fasta(p["u1.fa"]) == s_unitigs
    assert _lines(p["cl1.tsv.gz"]) == S.class_lines(s_classes) and sum(s_classes["runs"]) == len(s_unitigs)
    assert _lines(p["ucc1.txt.gz"]) == S.unitig_class_lines(s_unitigs, s_classes["kmer_class"], K)
    assert all(re.fullmatch(r"\d+:\d+", l) for l in _lines(p["ucc1.txt.gz"])) and all(re.fullmatch(r"\d+:[0-9a-f]+", l) for l in _lines(p["uc1.txt"]))
    assert _lines(p["uc1.txt"]) == KC.unitig_color_lines(s_unitigs, s_col["kmer_colors"], K)
    assert _lines(p["ab1.tsv"]) == ["unitig\tkmers\tabundance\tmean"] + [
        f"{i}\t{len(u) - K + 1}\t{a}\t{a / (len(u) - K + 1):.3f}" for i, (u, a) in enumerate(zip(s_unitigs, s_ab["unitig_sums"]))]
    assert _classes_line(r1.stderr) == _want_line(s_classes)
    loaded = [l for l in r1.stderr.splitlines() if l.startswith("Loaded ")]
    assert len(loaded) == 1 and loaded[0].startswith(f"Loaded {len(s_unitigs)} unitigs: ")
    assert f"(compacted from {api.Compaction(**s_stats).describe()}; cut into {len(s_unitigs)} monochromatic unitigs; " in loaded[0]
    assert sorted(zip(s_classes["masks"], s_classes["kmers"])) == sorted(zip(classes["masks"], classes["kmers"]))  # the same classes, another order at most


def test_two_files_with_a_threshold(product_lib, inputs):
    d, records, colors, _, _ = inputs
    names = [str(d / n) for n in ("c.fa", "a.fa")]  # another order: colour 0 is c.fa
    recs = [r for r, c in zip(records, colors) if c == 2] + [r for r, c in zip(records, colors) if c == 0]
    cols = [0] * colors.count(2) + [1] * colors.count(0)
    for split, m in ((False, 1), (True, 2)):
        cl, ucc = d / f"two{split}.tsv", d / f"two{split}.txt.gz"
        r = _cli("--seq-in", names[0], "--seq-in", names[1], "-k", K, "--color-classes-out", cl, "--unitig-color-classes-out", ucc,
                 *(["--monochromatic-unitigs", "--min-abundance", m] if split else []))
        assert r.returncode == 0, r.stderr[-3000:]
        unitigs, _, _, ab, _, classes = S.compact_classes(recs, cols, 2, K, m, split)
        assert _lines(cl) == S.class_lines(classes) and _lines(ucc) == S.unitig_class_lines(unitigs, classes["kmer_class"], K)
        assert _classes_line(r.stderr) == _want_line(classes) and (ab["dropped"] > 0) == split
        if not split:
            assert {int(l.split("\t")[1], 16) for l in _lines(cl)[1:]} == {1, 2, 3}


def test_the_tig_algorithms_take_the_split_unitigs(product_lib, inputs):
    """The (k-1)-mer join is fed unitigs that are not maximal, as it is by a `--min-abundance` run."""
    d, records, colors, _, _ = inputs
    names = [str(d / n) for n in ("a.fa", "b.fq.gz", "c.fa")]
    p = {n: str(d / ("tigs_" + n)) for n in ("u.fa", "t.fa", "e.fa", "t2.fa", "e2.fa")}
    r = _cli("--seq-in", names[0], "--seq-in", names[1], "--seq-in", names[2], "-k", K, "--min-base-quality", Q, "--monochromatic-unitigs",
             "--unitigs-fa-out", p["u.fa"], "--greedytigs-fa-out", p["t.fa"], "--eulertigs-fa-out", p["e.fa"], "--verify")
    print(r.stderr[-3000:])
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stderr.count("k-mer sets equal") >= 2 and "DIFFER" not in r.stderr
    assert _fasta(p["u.fa"]) == S.compact_classes(records, colors, 3, K, 1, True)[0]
    r2 = _cli("--fa-in", p["u.fa"], "-k", K, "--greedytigs-fa-out", p["t2.fa"], "--eulertigs-fa-out", p["e2.fa"], "--verify")
    assert r2.returncode == 0, r2.stderr[-3000:]
    for x, y in (("t.fa", "t2.fa"), ("e.fa", "e2.fa")):
        assert Path(p[x]).read_bytes() == Path(p[y]).read_bytes() and Path(p[x]).stat().st_size > 0, x


def test_without_the_new_flags_nothing_changes(product_lib, inputs):
    """Held to expectations recomputed from the restatement of DESIGN.md 22, not to stored output."""
    d, records, colors, _, _ = inputs
    names = [str(d / n) for n in ("a.fa", "b.fq.gz", "c.fa")]
    p = {n: str(d / ("plain_" + n)) for n in ("m.tsv", "uc.txt", "u.fa")}
    r = _cli("--seq-in", names[0], "--seq-in", names[1], "--seq-in", names[2], "-k", K, "--min-base-quality", Q, "--color-matrix-out", p["m.tsv"],
             "--unitig-colors-out", p["uc.txt"], "--unitigs-fa-out", p["u.fa"])
    assert r.returncode == 0, r.stderr[-3000:]
    unitigs, stats, _, ab, want = KC.compact_colored(records, colors, 3, K)
    assert _fasta(p["u.fa"]) == unitigs and _lines(p["m.tsv"]) == KC.matrix_lines(names, want)
    assert _lines(p["uc.txt"]) == KC.unitig_color_lines(unitigs, want["kmer_colors"], K)
    own = [l for l in r.stderr.splitlines() if re.match(r"(Read|Colours?|Loaded|Writing|Computing|Verifying|Querying)\b", l)]  # (the program's lines)
    assert [l.split(" ")[0] for l in own] == ["Read", "Colours:", "Loaded", "Writing"] and "monochromatic" not in r.stderr, r.stderr
    loaded = own[2]
    assert re.fullmatch(re.escape(f"Loaded {len(unitigs)} unitigs: ") + r"\d+ nodes, \d+ edges in [0-9.]+s "
                        + re.escape(f"(compacted from {api.Compaction(**stats).describe()}; ") + r"\d+ non-ACGT runs cut\)", loaded), loaded


def test_the_flags_need_seq_in_and_at_most_64_files(inputs):
    d = inputs[0]
    for flag in (["--monochromatic-unitigs"], ["--color-classes-out", d / "x.tsv"], ["--unitig-color-classes-out", d / "x.txt"]):
        r = _cli("--fa-in", d / "a.fa", "-k", K, "--unitigs-fa-out", d / "x.fa", *flag)
        assert r.returncode == 2 and f"{flag[0]} needs --seq-in" in r.stderr and "Traceback" not in r.stderr, r.stderr
    many = [x for _ in range(65) for x in ("--seq-in", d / "a.fa")]
    for flag in (["--monochromatic-unitigs", "--unitigs-fa-out", d / "x.fa"], ["--color-classes-out", d / "x.tsv"],
                 ["--unitig-color-classes-out", d / "x.txt"]):
        r = _cli(*many, "-k", K, *flag)
        assert r.returncode == 2 and "65 --seq-in files: at most 64" in r.stderr and "Traceback" not in r.stderr, r.stderr
    assert not (d / "x.fa").exists() and not (d / "x.tsv").exists()
