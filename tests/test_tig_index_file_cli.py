"""The command line of the index file without a GPU: the argument errors of `--index-out` / `--index-in`, raised before
any file is opened (no path below exists), the messages of runs without the new flags unchanged, and `--index-info` in a child
process that never initialises HIP."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import tig_index_file_ref as ref
from matchtigs_amd.__main__ import main

ROOT = Path(__file__).resolve().parent.parent


def _error(capsys, *argv):
    with pytest.raises(SystemExit) as e:
        main(list(argv))
    assert e.value.code == 2
    return capsys.readouterr().err.strip().splitlines()[-1]


@pytest.mark.parametrize("argv,needles", [
    (["--index-in", "no.mtgx", "--seq-in", "no.fa", "-k", "9", "--query-fa", "q.fa", "--query-out", "o.tsv"], ["--index-in cannot be combined with --seq-in"]),
    (["--index-in", "no.mtgx", "--fa-in", "no.fa"], ["--index-in cannot be combined with --fa-in"]),
    (["--index-in", "no.mtgx", "--greedytigs-fa-out", "g.fa"], ["--greedytigs-fa-out cannot be combined with --index-in", "sequences of the indexed set"]),
    (["--index-in", "no.mtgx", "--count-fa", "c.fa", "--count-out", "c.tsv"], ["--count-fa cannot be combined with --index-in"]),
    (["--index-in", "no.mtgx", "--correct-fa", "c.fa", "--correct-out", "c.out"], ["--correct-fa cannot be combined with --index-in"]),
    (["--index-in", "no.mtgx", "--verify", "--query-fa", "q.fa", "--query-out", "o.tsv"], ["--verify cannot be combined with --index-in"]),
    (["--index-in", "no.mtgx", "--unitigs-fa-out", "u.fa"], ["--unitigs-fa-out cannot be combined with --index-in"]),
    (["--index-in", "no.mtgx", "--clip-tips", "5", "--query-fa", "q.fa", "--query-out", "o.tsv"], ["--clip-tips cannot be combined with --index-in"]),
    (["--index-in", "no.mtgx", "--query-fa", "q.fa", "--query-out", "o.tsv", "--query-index", "table"], ["--query-index table cannot be combined with --index-in"]),
    (["--index-in", "no.mtgx", "--query-fa", "q.fa", "--query-out", "o.tsv", "--query-index-over", "greedytigs"], ["--query-index-over", "the file's to say"]),
    (["--index-in", "no.mtgx", "--query-fa", "q.fa", "--query-out", "o.tsv", "--query-minimizer-length", "7"], ["--query-minimizer-length", "the file's to say"]),
    (["--index-in", "no.mtgx", "--query-fa", "q.fa", "--query-out", "o.tsv", "--query-locate-out", "l.tsv"], ["--query-locate-out cannot be combined with --index-in"]),
    (["--index-in", "no.mtgx", "--pseudoalign-fa", "r.fa", "--pseudoalign-out", "o.tsv", "--pseudoalign-index", "table"], ["--pseudoalign-index table"]),
    (["--index-in", "no.mtgx", "--index-out", "other.mtgx"], ["--index-out cannot be combined with --index-in"]),
    (["--index-in", "no.mtgx"], ["nothing to do with --index-in"]),
    (["--index-in", "no.mtgx", "--query-fa", "q.fa"], ["--query-fa needs --query-out"]),
    (["--index-in", "no.mtgx", "--pseudoalign-fa", "r.fa"], ["--pseudoalign-fa needs --pseudoalign-out"]),
    (["--seq-in", "no.fa", "-k", "9", "--index-weights", "--greedytigs-fa-out", "g.fa"], ["--index-weights needs --index-out"]),
    (["--fa-in", "no.fa", "-k", "9", "--index-out", "x.mtgx", "--index-weights"], ["--index-weights needs --seq-in"]),
    (["--bcalm-in", "no.fa", "-k", "9", "--index-out", "x.mtgx", "--index-colors"], ["--index-colors needs --seq-in"]),
    (["--seq-in", "no.fa", "-k", "9", "--index-out", "x.mtgx", "--index-over", "greedytigs"], ["--index-over greedytigs needs --greedytigs-fa-out"]),
    (["--seq-in", "no.fa", "-k", "9", "--index-out", "x.mtgx", "--index-over", "eulertigs", "--greedytigs-fa-out", "g.fa"],
     ["--index-over eulertigs needs --eulertigs-fa-out"]),
    (["--seq-in", "no.fa", "-k", "9", "--index-out", "x.mtgx", "--index-minimizer-length", "10"], ["--index-minimizer-length must be in 1..9"]),
    (["--seq-in", "no.fa", "-k", "9", "--index-over", "input", "--greedytigs-fa-out", "g.fa"], ["--index-over needs --index-out"]),
    (["--seq-in"] + [x for i in range(65) for x in (f"no{i}.fa", "--seq-in")][:-1] + ["-k", "9", "--index-out", "x.mtgx", "--index-colors"],
     ["65 --seq-in files: at most 64 files can be told apart as colours"]),
])
def test_argument_errors_before_any_file_is_opened(capsys, argv, needles):
    line = _error(capsys, *argv)
    assert line.startswith("matchtigs_amd: error: ") and all(n in line for n in needles), line


def test_messages_without_the_new_flags_are_unchanged(capsys):
    assert _error(capsys, "-k", "9", "--greedytigs-fa-out", "g.fa") == (
        "matchtigs_amd: error: Missing input argument. Specify exactly least one of --fa-in, --gfa-in or --bcalm-in")
    assert _error(capsys, "--fa-in", "a.fa", "--bcalm-in", "b.fa", "-k", "9") == (
        "matchtigs_amd: error: Too many input arguments. Specify exactly least one of --fa-in, --gfa-in or --bcalm-in")
    assert _error(capsys, "--seq-in", "a.fa", "--greedytigs-fa-out", "g.fa") == "matchtigs_amd: error: --seq-in requires -k"
    assert _error(capsys, "--fa-in", "a.fa", "-k", "9", "--query-fa", "q.fa") == "matchtigs_amd: error: --query-fa needs --query-out"
    assert _error(capsys, "--fa-in", "a.fa", "-k", "9", "--pseudoalign-fa", "r.fa", "--pseudoalign-out", "o.tsv") == (
        "matchtigs_amd: error: --pseudoalign-fa needs --seq-in: the colours are the --seq-in files")
    assert _error(capsys, "--fa-in", "a.fa", "-k", "9") == (
        "matchtigs_amd: error: nothing to do: give --greedytigs-fa-out / --greedytigs-gfa-out and/or --eulertigs-fa-out / --eulertigs-gfa-out")
    assert _error(capsys, "--fa-in", "a.fa", "-k", "9", "--query-fa", "q.fa", "--query-out", "o.tsv", "--query-index-over", "greedytigs") == (
        "matchtigs_amd: error: --query-index-over greedytigs needs --greedytigs-fa-out")


CHILD = """
import os, sys
from matchtigs_amd.__main__ import main
rc = main(["--index-info", sys.argv[1]])
opened = [os.readlink(f"/proc/self/fd/{n}") for n in os.listdir("/proc/self/fd") if os.path.islink(f"/proc/self/fd/{n}")]
gpu = [t for t in opened if t.startswith(("/dev/kfd", "/dev/dri"))]
print(f"GPU_FILES={gpu}", file=sys.stderr)
sys.exit(rc)
"""


def _info(path):
    import os

    return subprocess.run([sys.executable, "-c", CHILD, str(path)], capture_output=True, text=True, cwd=ROOT,
                          env=dict(os.environ, PYTHONPATH=str(ROOT)))


def test_index_info_prints_the_header_without_a_gpu(tmp_path):
    fields = ref.plain_fields(k=5, m=3, records=2, characters=20, occurrences=12, anchors=3, locating=1)
    arrays = {"packed": np.zeros(4, np.uint32), "off": np.array([0, 12, 20], np.uint64), "dir": np.zeros(9, np.uint64), "entries": np.zeros(3, np.uint64)}
    path = tmp_path / "hand.mtgx"
    data = ref.write(path, fields, arrays, {"indexed": "greedytigs", "colors": ["a.fa", "ö.fa"], "min_abundance": 2, "cleaning": {"clip_tips": 9}})
    r = _info(path)
    assert r.returncode == 0, r.stderr
    assert "GPU_FILES=[]" in r.stderr  # the device files were never opened: HIP was not initialised
    rows = dict(line.split("\t", 1) for line in r.stdout.splitlines())
    assert all(line.count("\t") >= 1 for line in r.stdout.splitlines())
    assert rows["file_bytes"] == str(len(data)) and rows["format_version"] == "1" and rows["file"] == str(path)
    for f in ref.INFO_FIELDS:
        assert rows[f] == str(fields[f]), f
    assert rows["device_bytes"] == str(4 * 4 + 3 * 8 + 9 * 8 + 3 * 8)
    assert (rows["locating"], rows["weighted"], rows["colored"], rows["n_colors"]) == ("1", "0", "0", "0")
    assert rows["meta.indexed"] == "greedytigs" and rows["meta.colors"] == '["a.fa", "ö.fa"]' and rows["meta.min_abundance"] == "2"
    assert rows["meta.cleaning"] == '{"clip_tips": 9}'

    damaged = bytearray(data)
    damaged[60] ^= 1
    path.write_bytes(damaged)
    r = _info(path)
    assert r.returncode == 2 and r.stdout == "" and "header digest" in r.stderr and str(path) in r.stderr
    assert "GPU_FILES=[]" in r.stderr
    r = _info(tmp_path / "missing.mtgx")
    assert r.returncode == 2 and "cannot open" in r.stderr


def test_index_info_of_the_golden_file():
    r = _info(ROOT / "tests" / "golden" / "tig_index_v1.mtgx")
    assert r.returncode == 0, r.stderr
    rows = dict(line.split("\t", 1) for line in r.stdout.splitlines())
    assert (rows["k"], rows["m"], rows["records"], rows["locating"], rows["meta.indexed"]) == ("5", "3", "9", "0", "golden")
