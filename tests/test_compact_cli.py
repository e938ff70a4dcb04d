"""The unitig compaction (`--seq-in`, mtg_compact_unitigs), the part that needs no GPU: the C entry points are declared
and exported, the flag rules (each in a child process), the splitting FASTA reader, and the restatement the GPU tests
(test_gpu_compact.py) compare against is held to the structural properties of the contract and to synth.g_seq."""
import ctypes as C
import gzip
import re
import subprocess
import sys
from pathlib import Path

import pytest

import compact_ref as R
from matchtigs_amd import synth

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = ("mtg_compact_unitigs", "mtg_compact_unitigs_store", "mtg_last_compact_times", "mtg_read_sequences_split")


def _run(*a):
    return subprocess.run([sys.executable, "-m", "matchtigs_amd", *a], capture_output=True, text=True, cwd=str(ROOT), timeout=300)


def test_entry_points_declared_and_exported(product_lib):
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mtg_engine.h").read_text(), flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in include/mtg_engine.h"
        assert hasattr(product_lib, name), f"{name} is not exported"
    assert "mtg_compaction" in header
    from matchtigs_amd import _lib, api

    assert C.sizeof(_lib.MtgCompaction) == 8 * 8
    assert callable(api.compact_unitigs) and callable(api.last_compact_times)


def test_help_lists_the_flags(product_lib):
    r = _run("--help")
    assert r.returncode == 0 and "--seq-in" in r.stdout and "--unitigs-fa-out" in r.stdout


def test_seq_in_requires_k(tmp_path, product_lib):
    (tmp_path / "s.fa").write_text(">0\nACGTACGT\n")
    r = _run("--seq-in", str(tmp_path / "s.fa"), "--unitigs-fa-out", str(tmp_path / "u.fa"))
    assert r.returncode != 0 and "--seq-in requires -k" in r.stderr, r.stderr[-500:]


def test_seq_in_counts_as_an_input(tmp_path, product_lib):
    r = _run("--seq-in", str(tmp_path / "s.fa"), "--bcalm-in", str(tmp_path / "b.fa"), "-k", "5", "--unitigs-fa-out", str(tmp_path / "u.fa"))
    assert r.returncode != 0 and "Too many input arguments. Specify exactly least one of --fa-in, --gfa-in or --bcalm-in" in r.stderr


def test_existing_error_texts_stay(tmp_path, product_lib):
    r = _run("--unitigs-fa-out", str(tmp_path / "u.fa"))
    assert r.returncode != 0 and "Missing input argument. Specify exactly least one of --fa-in, --gfa-in or --bcalm-in" in r.stderr
    r = _run("--gfa-in", str(tmp_path / "g.gfa"), "-k", "5", "--unitigs-fa-out", str(tmp_path / "u.fa"))
    assert r.returncode != 0 and "only --bcalm-in and --fa-in are served by the MI355X engine (SURVEY.md 8 f-2)" in r.stderr
    r = _run("--fa-in", str(tmp_path / "f.fa"), "--unitigs-fa-out", str(tmp_path / "u.fa"))
    assert r.returncode != 0 and "--fa-in requires -k" in r.stderr


def test_unitigs_fa_out_counts_as_something_to_do(tmp_path, product_lib):
    """`--unitigs-fa-out` alone passes the "nothing to do" rule: the run gets as far as opening the (missing) input."""
    r = _run("--seq-in", str(tmp_path / "missing.fa"), "-k", "5", "--unitigs-fa-out", str(tmp_path / "u.fa"))
    assert r.returncode != 0 and "cannot open" in r.stderr and "nothing to do" not in r.stderr, r.stderr[-500:]
    r = _run("--seq-in", str(tmp_path / "missing.fa"), "-k", "5")
    assert r.returncode != 0 and "nothing to do" in r.stderr


SPLIT_TEXT = (">chr1 with gaps\nacgtNNNN\nNNtgca\nGGn\n\n>2 all N\nNNNN\n>3\nNACGTAC\r\nGTRYACGT\n>4 clean\nAC\nGT\n>5 gap across lines\nAAN\nNCC")
SPLIT_PIECES = ["ACGT", "TGCAGG", "ACGTACGT", "ACGT", "ACGT", "AA", "CC"]
SPLIT_RUNS = 6  # NNNN NN | n | NNNN | N | RY | N N


@pytest.mark.parametrize("gz", [False, True])
def test_read_sequences_split(tmp_path, product_lib, gz):
    """`N` runs (within and across lines, at record ends), IUPAC codes, lower case, multi-line records, CRLF, plain and gzipped."""
    from matchtigs_amd import api

    p = tmp_path / ("t.fa.gz" if gz else "t.fa")
    p.write_bytes(gzip.compress(SPLIT_TEXT.encode()) if gz else SPLIT_TEXT.encode())
    st = api.read_sequences(str(p), split_non_acgt=True)
    assert st.sequences() == SPLIT_PIECES
    assert st.pieces_cut == SPLIT_RUNS
    data, off = st.arrays()
    assert data.tobytes().decode() == "".join(SPLIT_PIECES) and list(off) == [0, 4, 10, 18, 22, 26, 28, 30]


def test_read_sequences_split_leaves_clean_files_alone(tmp_path, product_lib):
    from matchtigs_amd import api

    (tmp_path / "c.fa").write_text(">0\nACGT\nacgt\n>1\n>2\nTT\n")
    st = api.read_sequences(str(tmp_path / "c.fa"), split_non_acgt=True)
    assert st.sequences() == ["ACGTACGT", "TT"] and st.pieces_cut == 0  # (the empty record is dropped)
    assert api.read_sequences(str(tmp_path / "c.fa")).sequences() == ["ACGTACGT", "", "TT"]  # the plain reader is unchanged


# ---- the restatement against the contract's structure and against the tree's older compaction ----
def _case(k, seed):
    length = {5: 60, 12: 600}.get(k, 1200)
    return synth.random_genome(length, seed, haplotypes=4, sub_rate=0.02), length


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("k", [5, 12, 21, 31, 32])
def test_restatement_structure(k, seed):
    seqs, _ = _case(k, seed)
    unitigs, stats, closed = R.compact(seqs, k)
    _, reading, windows, _, out, into = R.graph_of(seqs, k)
    # every canonical k-mer of the input occurs exactly once over all unitigs
    seen = [synth.canonical(u[i:i + k]) for u in unitigs for i in range(len(u) - k + 1)]
    assert sorted(seen) == sorted(synth.kmer_set_of_tigs(seqs, k)) and len(seen) == len(set(seen)) == stats["distinct_kmers"]
    assert windows == sum(len(s) - k + 1 for s in seqs) == stats["windows"]
    for u, c in zip(unitigs, closed):
        # every interior junction is a passable node
        assert all(R.passable(u[i:i + k - 1], out, into) for i in range(1, len(u) - k + 1))
        # no unitig end is a passable node, unless the unitig is closed
        first, last = u[:k - 1], u[-(k - 1):]
        if c:
            assert first == last and R.passable(first, out, into)
        else:
            assert not R.passable(first, out, into) and not R.passable(last, out, into)
    # leaders: a unitig holds its first-created k-mer as read, and the unitigs come in the order of those
    creator = {x: p for x, p in R.graph_of(seqs, k)[0].items()}
    leaders = []
    for u in unitigs:
        p, w = min((creator[synth.canonical(u[i:i + k])], u[i:i + k]) for i in range(len(u) - k + 1))
        assert w == reading[synth.canonical(w)]
        leaders.append(p)
    assert leaders == sorted(leaders)


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("k", [5, 12, 21, 31, 32])
def test_restatement_agrees_with_g_seq(k, seed):
    """Same unitig set as synth.g_seq (which walks from sorted k-mers and stops at visited ones). The two differ in where a closed
    walk starts, so the comparison is made on inputs without closed walks -- checked here."""
    seqs, length = _case(k, seed)
    unitigs, stats, closed = R.compact(seqs, k)
    assert stats["closed_walks"] == 0 and not any(closed)
    ug = synth.g_seq(length, seed=seed, k=k, haplotypes=4, sub_rate=0.02)
    assert sorted(synth.canonical(u) for u in unitigs) == sorted(synth.canonical(u) for u in ug.unitigs)


def test_restatement_special_shapes():
    # a homopolymer: one closed walk of length 1
    u, s, c = R.compact(["AAAAAAA"], 4)
    assert u == ["AAAA"] and c == [True] and s["closed_walks"] == 1 and s["windows"] == 4
    # an even-k palindromic k-mer is a unitig of its own
    u, s, c = R.compact(["CCACGTGG"], 4)
    assert "ACGT" in u and s["closed_walks"] == 0
    # a circular sequence given with its first k - 1 bases repeated: one closed walk from the first window on
    circ = "ACGGTCATTGGA"
    u, s, c = R.compact([circ + circ[:4]], 5)
    assert u == [circ + circ[:4]] and c == [True]
    # ... rotated input: the walk starts at the new first window
    rot = circ[5:] + circ[:5]
    u, s, c = R.compact([rot + rot[:4]], 5)
    assert u == [rot + rot[:4]] and c == [True]
    # records shorter than k contribute nothing; lower case equals upper case
    assert R.compact(["ACG", "acggt", ""], 4)[0] == R.compact(["ACGGT"], 4)[0] == ["ACGGT"]
