"""Threading through the command line (`--thread-fa`). Without a GPU: the C-ABI's declarations and the flag rules. On
the GPU: haplotypes threaded through the graph this run wrote -- one end-to-end walk each, over segments and links that the GFA
holds --, the table and the sparse index and a saved index with byte-identical files, and a read with an injected error broken in two
exactly where the cleaned graph lacks its k-mers."""
import random
import subprocess
import sys
from pathlib import Path

import pytest

from matchtigs_amd import _lib, synth

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = ("mtg_kmer_index_thread", "mtg_tig_index_thread", "mtg_kmer_walks_count", "mtg_kmer_walks_steps_count", "mtg_kmer_walks_arrays",
                "mtg_kmer_walks_steps", "mtg_kmer_walks_free", "mtg_last_kmer_thread_times", "mtg_last_tig_thread_times", "mtg_kmer_walks_gaf")
K = 21


def _cli(*a):
    return subprocess.run([sys.executable, "-m", "matchtigs_amd", *map(str, a)], capture_output=True, text=True, cwd=str(ROOT), timeout=300)


def test_entry_points_declared_and_exported(product_lib):
    names = _lib.declared_symbols()
    for n in ENTRY_POINTS:
        assert n in names and hasattr(product_lib, n), n


def test_help_lists_the_flags():
    r = _cli("--help")
    assert r.returncode == 0
    for flag in ("--thread-fa", "--thread-gaf-out", "--thread-report-out", "--thread-min-kmers", "--thread-min-base-quality", "--thread-index",
                 "--thread-minimizer-length"):
        assert flag in r.stdout, flag


def test_flag_misuse_exits_2(tmp_path):
    missing = tmp_path / "no_such.fa"
    base = ("--fa-in", missing, "-k", "5")
    for extra, message in ((("--thread-gaf-out", "t.gaf"), "--thread-gaf-out needs --thread-fa"),
                           (("--thread-report-out", "r.tsv"), "--thread-report-out needs --thread-fa"),
                           (("--thread-min-kmers", "3"), "--thread-min-kmers needs --thread-fa"),
                           (("--thread-index", "minimizer"), "--thread-index needs --thread-fa"),
                           (("--thread-fa", "r.fa"), "--thread-fa needs --thread-gaf-out or --thread-report-out"),
                           (("--thread-fa", "r.fa", "--thread-gaf-out", "t.gaf", "--thread-min-kmers", "0"), "--thread-min-kmers must be >= 1"),
                           (("--thread-fa", "r.fa", "--thread-gaf-out", "t.gaf", "--thread-min-base-quality", "94"), "must be in 0..93"),
                           (("--thread-fa", "r.fa", "--thread-gaf-out", "t.gaf", "--thread-minimizer-length", "3"),
                            "--thread-minimizer-length needs --thread-index minimizer"),
                           (("--thread-fa", "r.fa", "--thread-gaf-out", "t.gaf", "--thread-index", "minimizer", "--thread-minimizer-length", "6"),
                            "--thread-minimizer-length must be in 1..5")):
        r = _cli(*base, *extra)
        assert r.returncode == 2 and message in r.stderr, (extra, r.stderr[-500:])
    for extra, message in ((("--thread-fa", "r.fa", "--thread-gaf-out", "t.gaf", "--thread-index", "table"), "--thread-index table cannot be combined"),
                           (("--thread-fa", "r.fa", "--thread-gaf-out", "t.gaf", "--thread-minimizer-length", "3"), "are the file's to say"),
                           (("--thread-gaf-out", "t.gaf", "--query-fa", "q.fa", "--query-out", "q.tsv"), "--thread-gaf-out needs --thread-fa")):
        r = _cli("--index-in", tmp_path / "no_such.mtgx", *extra)
        assert r.returncode == 2 and message in r.stderr, (extra, r.stderr[-500:])
    # with its outputs named, the run gets as far as opening the input
    r = _cli(*base, "--thread-fa", missing, "--thread-gaf-out", tmp_path / "t.gaf")
    assert r.returncode != 0 and "needs" not in r.stderr, r.stderr[-2000:]


def _gaf(path):
    return [line.split("\t") for line in Path(path).read_text().splitlines()]


def _steps(path_column):
    out, at = [], 0
    while at < len(path_column):
        end = min([i for i in (path_column.find(">", at + 1), path_column.find("<", at + 1)) if i > 0] or [len(path_column)])
        out.append((path_column[at + 1:end], "+" if path_column[at] == ">" else "-"))
        at = end
    return out


@pytest.fixture(scope="module")
def haplotype_run(tmp_path_factory, product_lib):
    """Two haplotypes compacted, the graph written as GFA, both threaded through it on the table index, and the sparse index saved."""
    tmp = tmp_path_factory.mktemp("thread")
    haps = synth.random_genome(1500, seed=36, haplotypes=2, sub_rate=0.01)
    files = []
    for i, h in enumerate(haps):
        files.append(tmp / f"hap{i}.fa")
        files[-1].write_text(f">hap{i} a haplotype\n{h[:700]}\n{h[700:]}\n")
    shared = [x for f in files for x in ("--thread-fa", f)]
    r = _cli("--seq-in", files[0], "--seq-in", files[1], "-k", K, "--unitigs-gfa-out", tmp / "g.gfa", *shared, "--thread-gaf-out", tmp / "table.gaf",
             "--thread-report-out", tmp / "table.tsv", "--index-out", tmp / "g.mtgx")
    assert r.returncode == 0, r.stderr[-3000:]
    return tmp, haps, files, shared, r.stderr


@pytest.mark.gpu
def test_haplotypes_are_paths_of_the_written_graph(haplotype_run):
    tmp, haps, files, _, stderr = haplotype_run
    gfa = [line.split("\t") for line in (tmp / "g.gfa").read_text().splitlines()]
    segments = {f[1]: f[2] for f in gfa if f[0] == "S"}
    links = {(f[1], f[2], f[3], f[4]) for f in gfa if f[0] == "L"}
    flip = {"+": "-", "-": "+"}
    rows = _gaf(tmp / "table.gaf")
    assert [r[0] for r in rows] == ["hap0", "hap1"] and len(segments) > 10
    for row, h in zip(rows, haps):
        assert row[1:5] == [str(len(h)), "0", str(len(h)), "+"] and row[9:12] == [str(len(h)), str(len(h)), "255"]
        assert row[12:] == [f"cg:Z:{len(h)}=", f"km:i:{len(h) - K + 1}"]
        steps = _steps(row[5])
        assert len(steps) > 5 and all(name in segments for name, _ in steps)
        for (a, sa), (b, sb) in zip(steps, steps[1:]):
            assert (a, sa, b, sb) in links or (b, flip[sb], a, flip[sa]) in links, (a, sa, b, sb)
        spelled = ""
        for name, strand in steps:
            s = segments[name] if strand == "+" else synth.revcomp(segments[name])
            spelled = s if not spelled else spelled + s[K - 1:]
        assert len(spelled) == int(row[6]) and spelled[int(row[7]):int(row[8])] == h
    report = [line.split("\t") for line in (tmp / "table.tsv").read_text().splitlines()]
    assert report[0] == ["file", "record", "length", "kmers", "valid", "found", "walks", "steps", "longest"]
    for row, gaf_row, f, h in zip(report[1:], rows, files, haps):
        n = str(len(h) - K + 1)
        assert row == [str(f), gaf_row[0], str(len(h)), n, n, n, "1", str(len(_steps(gaf_row[5]))), n]
    assert stderr.count("Threading ") == 2 and "1 reads, 1 threaded end to end, 1 walks" in stderr


@pytest.mark.gpu
def test_sparse_index_and_saved_index_write_the_same_files(haplotype_run):
    tmp, _, files, shared, _ = haplotype_run
    r = _cli("--seq-in", files[0], "--seq-in", files[1], "-k", K, *shared, "--thread-gaf-out", tmp / "sparse.gaf", "--thread-report-out",
             tmp / "sparse.tsv", "--thread-index", "minimizer", "--thread-minimizer-length", "9")
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp / "sparse.gaf").read_bytes() == (tmp / "table.gaf").read_bytes() and (tmp / "sparse.tsv").read_bytes() == (tmp / "table.tsv").read_bytes()
    r = _cli("--index-in", tmp / "g.mtgx", *shared, "--thread-gaf-out", tmp / "loaded.gaf.gz", "--thread-min-kmers", "1")
    assert r.returncode == 0, r.stderr[-3000:]
    import gzip

    assert gzip.decompress((tmp / "loaded.gaf.gz").read_bytes()) == (tmp / "table.gaf").read_bytes()


@pytest.mark.gpu
@pytest.mark.parametrize("tag,handed_over,extra", [
    ("counted", True, ("--query-locate-out", "q.loc", "--count-fa", "hap1.fa", "--count-out", "c.tsv", "--correct-fa", "hap1.fa", "--correct-report-out", "fix.tsv")),
    ("sparse", True, ("--query-index", "minimizer", "--thread-index", "minimizer")),
    ("own", False, ("--query-index", "minimizer", "--thread-index", "minimizer", "--thread-minimizer-length", "9"))])
def test_the_queries_locating_index_is_handed_over(haplotype_run, tag, handed_over, extra):
    """The table under --query-locate-out -- a count in between and a correction behind it included -- and the sparse index of the
    same minimizer length serve the threading too: no second index is built; with another minimizer length one is. The file is the same."""
    tmp, _, files, shared, first = haplotype_run
    assert "Indexing the input for the threading: table index" in first
    extra = [tmp / x if "." in x else x for x in extra]
    r = _cli("--seq-in", files[0], "--seq-in", files[1], "-k", K, *shared, "--query-fa", files[0], "--query-out", tmp / f"{tag}.q.tsv", *extra,
             "--thread-gaf-out", tmp / f"{tag}.gaf")
    assert r.returncode == 0, r.stderr[-3000:]
    assert ("for the threading" not in r.stderr) == handed_over and r.stderr.count("Threading ") == 2, r.stderr[-3000:]
    assert (tmp / f"{tag}.gaf").read_bytes() == (tmp / "table.gaf").read_bytes()


@pytest.mark.gpu
def test_an_error_breaks_a_read_where_the_cleaned_graph_lacks_it(tmp_path, product_lib):
    """Reads of 100 bases tile a genome at every 50th base, three copies each; one more copy of a tile carries a substitution at its
    base 50. --min-abundance 2 drops the 21 k-mers over it, so that read is two walks, of the 30 windows before and the 29 behind."""
    rng = random.Random(36)
    genome = "".join(rng.choice("ACGT") for _ in range(650))
    tiles = [genome[at:at + 100] for at in range(0, 600, 50)]
    bad = tiles[5][:50] + {"A": "C", "C": "G", "G": "T", "T": "A"}[tiles[5][50]] + tiles[5][51:]
    reads = [t for t in tiles for _ in range(3)] + [bad]
    fa = tmp_path / "reads.fa"
    fa.write_text("".join(f">read{i}\n{s}\n" for i, s in enumerate(reads)))
    r = _cli("--seq-in", fa, "-k", K, "--min-abundance", "2", "--clip-tips", K, "--unitigs-gfa-out", tmp_path / "g.gfa", "--thread-fa", fa,
             "--thread-gaf-out", tmp_path / "t.gaf", "--thread-report-out", tmp_path / "r.tsv")
    assert r.returncode == 0, r.stderr[-3000:]
    rows = _gaf(tmp_path / "t.gaf")
    last = f"read{len(reads) - 1}"
    assert [row[0] for row in rows] == [f"read{i}" for i in range(len(reads) - 1)] + [last, last]
    assert all(row[2:4] == ["0", "100"] and row[-1] == "km:i:80" for row in rows[:-2])
    assert [row[2:4] + [row[-1]] for row in rows[-2:]] == [["0", "50", "km:i:30"], ["51", "100", "km:i:29"]]
    report = [line.split("\t") for line in (tmp_path / "r.tsv").read_text().splitlines()]
    assert report[-1][1:7] == [last, "100", "80", "80", "59", "2"] and report[-1][8] == "30"
    assert int(report[-1][7]) == sum(len(_steps(row[5])) for row in rows[-2:])
    assert all(row[3:7] == ["80", "80", "80", "1"] and row[8] == "80" for row in report[1:-1])
    assert f"{len(reads)} reads, {len(reads) - 1} threaded end to end, {len(reads) + 1} walks" in r.stderr
