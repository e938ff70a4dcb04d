"""The command line of the k-mer selection on the GPU: tumour less normal, the core of three haplotypes, a gene panel,
every argument error, a run that selects nothing, the flags in an index file's metadata, and runs without the flags."""
import random
from pathlib import Path

import pytest

import kmer_color_ref as KC
import kmer_select_ref as S
from matchtigs_amd import synth
from matchtigs_amd.__main__ import main

pytestmark = pytest.mark.gpu
K = 31


@pytest.fixture(scope="module")
def gpu(product_lib):
    import torch

    if product_lib.mtg_device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("these tests need a GPU: the compaction has no CPU path")
    return torch


def _dna(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _fasta(path, records):
    Path(path).write_text("".join(f">r{i}\n{s}\n" for i, s in enumerate(records)))
    return str(path)


def _records(path):
    return [line for line in Path(path).read_text().splitlines() if not line.startswith(">")]


def _run(capsys, *argv):
    rc = main([str(a) for a in argv])
    return rc, capsys.readouterr().err


def _error(capsys, *argv):
    with pytest.raises(SystemExit) as e:
        main([str(a) for a in argv])
    assert e.value.code == 2
    return capsys.readouterr().err.strip().splitlines()[-1]


def test_tumour_less_normal(gpu, tmp_path, capsys):
    rng = random.Random(1)
    normal = _dna(rng, 600)
    at = 300
    tumour = normal[:at] + {"A": "C", "C": "G", "G": "T", "T": "A"}[normal[at]] + normal[at + 1:]
    t, n, out = _fasta(tmp_path / "tumour.fa", [tumour]), _fasta(tmp_path / "normal.fa", [normal]), tmp_path / "u.fa"
    rc, err = _run(capsys, "--seq-in", t, "--subtract-fa", n, "-k", K, "--unitigs-fa-out", out, "--verify", "--selection-out", tmp_path / "sel.tsv")
    assert rc == 0, err
    got = _records(out)
    want = tumour[at - K + 1:at + K]
    assert len(got) == 1 and len(got[0]) == 2 * K - 1 and got[0] in (want, synth.revcomp(want))
    assert "Verifying selection:" in err and "as counted" in err and "Verifying --subtract-fa" in err and "MISMATCH" not in err
    assert f"{600 - K + 1 - K} by subtract" in err  # inside the Loaded line: what the rule rejected
    lines = Path(tmp_path / "sel.tsv").read_text().splitlines()
    assert lines == [f"input\t{570}", "abundance_kept\t570", "forbid\t0", "require\t0", "carriers\t0", f"subtract\t{570 - K}", "intersect\t0", f"selected\t{K}"]


@pytest.fixture(scope="module")
def haplotypes(tmp_path_factory):
    """Three haplotypes of one genome of 500 bases: each with two substitutions of its own, the second also without a stretch."""
    rng = random.Random(2)
    genome = _dna(rng, 500)
    haps = []
    for h in range(3):
        s = list(genome)
        for at in (60 + 130 * h, 100 + 130 * h):
            s[at] = {"A": "C", "C": "G", "G": "T", "T": "A"}[s[at]]
        haps.append("".join(s))
    haps[1] = haps[1][:400]
    d = tmp_path_factory.mktemp("haps")
    return [_fasta(d / f"h{h}.fa", [haps[h][:250], haps[h][220:]]) for h in range(3)], [[haps[h][:250], haps[h][220:]] for h in range(3)]


def test_the_core_genome(gpu, haplotypes, tmp_path, capsys):
    paths, recs = haplotypes
    flat, colors = [r for rs in recs for r in rs], [h for h, rs in enumerate(recs) for _ in rs]
    args = [x for p in paths for x in ("--seq-in", p)]
    rc, err = _run(capsys, *args, "-k", K, "--min-colors", 3, "--unitigs-fa-out", tmp_path / "u.fa", "--selection-out", tmp_path / "sel.tsv",
                   "--color-matrix-out", tmp_path / "m.tsv", "--verify")
    assert rc == 0 and "MISMATCH" not in err, err
    want = S.compact_selected(flat, K, 1, colors, 3, min_colors=3)
    masks = KC.kmer_masks(flat, colors, K)
    core = {x for x, m in masks.items() if m == 0b111}
    got = _records(tmp_path / "u.fa")
    spelled = [synth.canonical(u[i:i + K]) for u in got for i in range(len(u) - K + 1)]
    assert 0 < len(core) < len(masks) and sorted(spelled) == sorted(core) and got == want["unitigs"]
    sel = dict(want["selection"], distinct_all=want["abundance"]["distinct_all"])
    assert Path(tmp_path / "sel.tsv").read_text().splitlines() == S.selection_lines(paths, want["colours"], sel)
    assert Path(tmp_path / "m.tsv").read_text().splitlines() == KC.matrix_lines(paths, want["colours"])
    assert want["selection"]["selected"] == want["colours"]["occupancy"][3]  # the occupancy row is how the threshold is chosen


def test_a_gene_panel(gpu, haplotypes, tmp_path, capsys):
    paths, recs = haplotypes
    flat = recs[0] + recs[2]
    panel = [recs[0][0][40:140], synth.revcomp(recs[2][1][100:180]).lower(), "ACGTNNNN" + recs[0][1][10:50]]
    rc, err = _run(capsys, "--seq-in", paths[0], "--seq-in", paths[2], "-k", K, "--intersect-fa", _fasta(tmp_path / "panel.fa", panel),
                   "--forbid-colors", "1", "--unitigs-fa-out", tmp_path / "u.fa", "--selection-out", tmp_path / "sel.tsv", "--verify")
    assert rc == 0 and "MISMATCH" not in err and "Verifying --intersect-fa" in err, err
    want = S.compact_selected(flat, K, 1, [0, 0, 1, 1], 2, forbid=0b10, intersect=panel)
    assert _records(tmp_path / "u.fa") == want["unitigs"] and 0 < want["selection"]["selected"] < want["selection"]["input_kmers"]
    assert want["selection"]["rejected_forbid"] > 0 and want["selection"]["rejected_intersect"] > 0
    sel = dict(want["selection"], distinct_all=want["abundance"]["distinct_all"])
    assert Path(tmp_path / "sel.tsv").read_text().splitlines() == S.selection_lines([paths[0], paths[2]], want["colours"], sel)


@pytest.mark.parametrize("argv,needles", [
    (["--seq-in", "a.fa", "--seq-in", "b.fa", "-k", "9", "--require-colors", "0,2", "--unitigs-fa-out", "u.fa"], ["--require-colors names file 2", "2 --seq-in files"]),
    (["--seq-in", "a.fa", "-k", "9", "--forbid-colors", "1-3", "--unitigs-fa-out", "u.fa"], ["--forbid-colors names file 3"]),
    (["--seq-in", "a.fa", "-k", "9", "--forbid-colors", "x", "--unitigs-fa-out", "u.fa"], ["--forbid-colors x"]),
    (["--seq-in", "a.fa", "--seq-in", "b.fa", "-k", "9", "--require-colors", "0-1", "--forbid-colors", "1", "--unitigs-fa-out", "u.fa"],
     ["--require-colors and --forbid-colors both name file 1"]),
    (["--seq-in", "a.fa", "-k", "9", "--min-colors", "2", "--max-colors", "1", "--unitigs-fa-out", "u.fa"], ["--min-colors 2 exceeds --max-colors 1"]),
    (["--seq-in", "a.fa", "-k", "9", "--max-colors", "65", "--unitigs-fa-out", "u.fa"], ["--max-colors must be in 0..64"]),
    (["--seq-in", "a.fa", "-k", "9", "--subtract-fa", "n.fa", "--subtract-min-abundance", "0", "--unitigs-fa-out", "u.fa"], ["--subtract-min-abundance must be >= 1"]),
    (["--seq-in", "a.fa", "-k", "9", "--intersect-min-abundance", "2", "--unitigs-fa-out", "u.fa"], ["--intersect-min-abundance needs --intersect-fa"]),
    (["--seq-in", "a.fa", "-k", "9", "--filter-min-base-quality", "20", "--unitigs-fa-out", "u.fa"], ["--filter-min-base-quality needs --subtract-fa"]),
    (["--fa-in", "a.fa", "-k", "9", "--subtract-fa", "n.fa", "--unitigs-fa-out", "u.fa"], ["--subtract-fa needs --seq-in"]),
    (["--bcalm-in", "a.fa", "-k", "9", "--min-colors", "1", "--unitigs-fa-out", "u.fa"], ["--min-colors needs --seq-in"]),
    (["--fa-in", "a.fa", "-k", "9", "--selection-out", "s.tsv"], ["--selection-out needs --seq-in"]),
    (["--index-in", "no.mtgx", "--intersect-fa", "p.fa", "--query-fa", "q.fa", "--query-out", "o.tsv"], ["--intersect-fa cannot be combined with --index-in"]),
    (["--index-in", "no.mtgx", "--max-colors", "1", "--query-fa", "q.fa", "--query-out", "o.tsv"], ["--max-colors cannot be combined with --index-in"]),
])
def test_argument_errors_name_their_flag_before_any_file_is_read(capsys, argv, needles):
    line = _error(capsys, *argv)
    assert line.startswith("matchtigs_amd: error: ") and all(n in line for n in needles), line


def test_nothing_selected(gpu, haplotypes, tmp_path, capsys):
    paths, _ = haplotypes
    rc, err = _run(capsys, "--seq-in", paths[0], "--seq-in", paths[1], "-k", K, "--require-colors", "0", "--max-colors", 1, "--subtract-fa", paths[0],
                   "--unitigs-fa-out", tmp_path / "u.fa", "--selection-out", tmp_path / "sel.tsv", "--color-matrix-out", tmp_path / "m.tsv",
                   "--kmer-spectrum-out", tmp_path / "spec.tsv")
    assert rc == 1 and "no k-mer is selected" in err and "by subtract" in err and not (tmp_path / "u.fa").exists()
    lines = Path(tmp_path / "sel.tsv").read_text().splitlines()
    assert lines[7] == "selected\t0" and lines[8].startswith(f"color\t{paths[0]}\t") and lines[8].endswith("\t0")
    assert (tmp_path / "m.tsv").read_text().startswith("color\tkmers") and (tmp_path / "spec.tsv").exists()


def test_the_index_file_records_the_flags(gpu, haplotypes, tmp_path, capsys):
    paths, _ = haplotypes
    rc, err = _run(capsys, "--seq-in", paths[0], "--seq-in", paths[1], "-k", K, "--min-colors", 2, "--subtract-fa", paths[2], "--subtract-min-abundance", 2,
                   "--index-out", tmp_path / "x.mtgx")
    assert rc == 0, err
    capsys.readouterr()
    assert main(["--index-info", str(tmp_path / "x.mtgx")]) == 0
    line = next(l for l in capsys.readouterr().out.splitlines() if l.startswith("meta.selection\t"))
    assert '"min_colors": 2' in line and '"subtract_min_abundance": 2' in line and paths[2] in line


def test_without_the_flags_the_files_are_the_same(gpu, haplotypes, tmp_path, capsys):
    paths, _ = haplotypes
    outs = []
    for name, extra in (("plain", []), ("trivial", ["--min-colors", 0, "--max-colors", 64])):
        d = tmp_path / name
        d.mkdir()
        rc, err = _run(capsys, "--seq-in", paths[0], "--seq-in", paths[1], "--seq-in", paths[2], "-k", K, "--min-abundance", 1, "--unitigs-fa-out", d / "u.fa",
                       "--greedytigs-fa-out", d / "g.fa", "--unitig-abundance-out", d / "a.tsv", "--color-matrix-out", d / "m.tsv",
                       "--unitig-colors-out", d / "c.tsv", "--unitigs-gfa-out", d / "u.gfa", *extra)
        assert rc == 0, err
        outs.append({p.name: p.read_bytes() for p in sorted(d.iterdir())})
    assert outs[0] == outs[1] and len(outs[0]) == 6 and all(outs[0].values())
