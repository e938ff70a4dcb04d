"""Plain unitig FASTA input (`--fa-in X -k K`): flag rules and input errors (each in a child process: the library aborts like the
reference panics), which are all decided before the GPU join; and the two restatements of the graph contract that the GPU tests
(test_gpu_fasta_in.py) compare against agree with each other."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import fasta_in_ref as R
from matchtigs_amd import synth

ROOT = Path(__file__).resolve().parent.parent


def _run(*a):
    return subprocess.run([sys.executable, "-m", "matchtigs_amd", *a], capture_output=True, text=True, cwd=str(ROOT), timeout=300)


def test_fa_in_requires_k(tmp_path, product_lib):
    (tmp_path / "u.fa").write_text(">0\nACGTACGT\n")
    r = _run("--fa-in", str(tmp_path / "u.fa"), "--eulertigs-fa-out", str(tmp_path / "o.fa"))
    assert r.returncode != 0 and "--fa-in requires -k" in r.stderr


def test_gfa_in_stays_refused(tmp_path, product_lib):
    r = _run("--gfa-in", str(tmp_path / "u.gfa"), "-k", "5", "--eulertigs-fa-out", str(tmp_path / "o.fa"))
    assert r.returncode != 0 and "only --bcalm-in and --fa-in are served" in r.stderr


@pytest.mark.parametrize("case", ["non_acgt", "short", "missing"])
def test_fa_in_input_errors(tmp_path, product_lib, case):
    p = tmp_path / "u.fa"
    if case == "non_acgt":
        p.write_text(">0 L:+:1:+\nACGTACGT\n>1\nACGT\nACNT\n")
        msg = "not in the DNA alphabet"
    elif case == "short":
        p.write_text(">0\nACGTACGT\n>1\nACG\n")
        msg = "< k"
    else:
        msg = "cannot open"
    r = _run("--fa-in", str(p), "-k", "5", "--greedytigs-fa-out", str(tmp_path / "o.fa"))
    assert r.returncode != 0 and msg in r.stderr, r.stderr[-500:]
    assert not (tmp_path / "o.fa").exists()


@pytest.mark.parametrize("k", [5, 12, 21, 31, 32])
def test_restatements_agree(k):
    ug = synth.g_seq(4000, seed=k, k=min(k, 31), haplotypes=3, sub_rate=0.03)
    seqs = [s for s in ug.unitigs if len(s) >= k] + ["ACGT" * 8, "ACGT" * 8, "A" * k]
    data = "".join(seqs).encode()
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    d, n = R.graph_dict(seqs, k), R.graph_np(np.frombuffer(data, np.uint8), off, k)
    for f in d:
        assert np.array_equal(d[f], n[f]), f
