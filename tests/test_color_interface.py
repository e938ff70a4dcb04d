"""The interface of the coloured k-mer set without a GPU: the new entry points are declared, exported and plain C99;
the command line refuses what it cannot serve before it touches a file; the Python layer refuses bad colours before it calls the
library."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from matchtigs_amd import _lib, api
from matchtigs_amd.__main__ import main

ROOT = Path(__file__).resolve().parent.parent
NEW = ("mtg_compact_unitigs_colored", "mtg_compact_unitigs_colored_store", "mtg_kmer_colors_count", "mtg_kmer_colors_array",
       "mtg_kmer_colors_free", "mtg_kmer_index_build_annotated", "mtg_kmer_index_build_annotated_store", "mtg_kmer_index_is_colored",
       "mtg_kmer_index_n_colors", "mtg_kmer_index_colors", "mtg_last_kmer_color_times")


def test_the_new_names_are_declared_and_exported(product_lib):
    names = _lib.declared_symbols()
    for n in NEW:
        assert n in names and hasattr(product_lib, n), n
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert set(NEW) <= syms  # unmangled => extern "C"
    for n in ("compact_unitigs_colored", "Colors", "KmerColorResult", "last_kmer_color_times"):
        assert hasattr(api, n), n


def test_the_headers_compile_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "matchtigs.h"\n#include "mtg_engine.h"\n'
                   "int main(void){mtg_color_stats s; return sizeof s == 8 * (1 + 64 + 65 + 64 * 64) && sizeof s.shared == 8 * 4096 ? 0 : 1;}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", str(ROOT / "include"), str(src), "-o", str(tmp_path / "t")], check=True)
    subprocess.run([str(tmp_path / "t")], check=True)
    assert _lib.C.sizeof(_lib.MtgColorStats) == 8 * (1 + 64 + 65 + 64 * 64)


def _exits_2(capsys, argv):
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_more_than_64_files_is_refused_before_any_file_is_touched(capsys, tmp_path):
    argv = ["-k", "31", "--color-matrix-out", str(tmp_path / "m.tsv")]
    for i in range(65):
        argv += ["--seq-in", str(tmp_path / f"missing_{i}.fa")]  # none of them exists
    err = _exits_2(capsys, argv)
    assert "64" in err and "65" in err and not (tmp_path / "m.tsv").exists()


def test_flags_that_need_other_flags(capsys, tmp_path):
    m = str(tmp_path / "x")
    err = _exits_2(capsys, ["--seq-in", m, "-k", "31", "--query-colors-out", m])
    assert "--query-colors-out needs" in err
    err = _exits_2(capsys, ["--fa-in", m, "-k", "31", "--unitig-colors-out", m, "--greedytigs-fa-out", m])
    assert "--unitig-colors-out needs --seq-in" in err
    err = _exits_2(capsys, ["--bcalm-in", m, "-k", "31", "--color-matrix-out", m])
    assert "--color-matrix-out needs --seq-in" in err
    assert not Path(m).exists()


SEQS = ["ACGTACGTAC", "AC", "GGGTTTAAAC"]  # k = 4: 7 + 0 + 7 windows
ARRAYS = (np.frombuffer("".join(SEQS).encode(), np.uint8), np.array([0, 10, 12, 22], np.uint64))


def test_bad_colours_are_refused_before_the_library_is_called(product_lib):
    """device_id 99 does not exist: a call that reached the library would abort the process."""
    for seqs in (SEQS, ARRAYS):
        for colors, n in (([0, 1, 2], 2), ([0, 3, 0], 3), ([0, -1, 0], 3), ([0, 0, 0], 0), ([0, 0, 0], 65), ([0, 0], 2), ([0, 0, 0, 0], 2),
                          ([], 1), (np.zeros((3, 1), np.uint8), 1), ([0.5, 0, 0], 2), ([0, 0, 0], None), ([0, 0, 0], 2.0)):
            with pytest.raises(ValueError):
                api.compact_unitigs_colored(seqs, 4, colors, n, device_id=99)
        with pytest.raises(ValueError):
            api.compact_unitigs_colored(seqs, 4, [0, 0, 0], 1, min_abundance=0, device_id=99)


def test_bad_masks_are_refused_before_the_library_is_called(product_lib):
    for seqs in (SEQS, ARRAYS):
        for colors, n in (([1] * 13, 2), ([1] * 15, 2), ([], 2), (np.ones((2, 7), np.uint64), 2), ([1] * 14, 0), ([1] * 14, 65),
                          ([1] * 14, None), ([1] * 13 + [4], 2), ([1] * 13 + [1 << 63], 63)):
            with pytest.raises(ValueError):
                api.KmerIndex(seqs, 4, device_id=99, colors=colors, n_colors=n)
        with pytest.raises(ValueError):
            api.KmerIndex(seqs, 4, device_id=99, weights=[1] * 13, colors=[1] * 14, n_colors=2)  # the weights' length
        with pytest.raises(ValueError):
            api.KmerIndex(seqs, 4, device_id=99, n_colors=2)  # colours without masks


def test_the_statistics_object():
    c = api.Colors(3, np.array([1, 3, 7, 4], np.uint64), np.array([3, 2, 2], np.uint64),
                   np.array([0, 2, 1, 1] + [0] * 61, np.uint64), np.array([[3, 2, 1], [2, 2, 1], [1, 1, 2]], np.uint64))
    assert (c.core, c.private) == (1, 2) and "1 core" in c.describe() and "2 private" in c.describe()
    j = c.jaccard()
    assert j.dtype == np.float64 and j.shape == (3, 3) and j[0, 1] == 2 / 3 and j[0, 2] == 1 / 4 and j[1, 1] == 1.0 and np.array_equal(j, j.T)
    empty = api.Colors(2, np.zeros(0, np.uint64), np.zeros(2, np.uint64), np.zeros(65, np.uint64), np.zeros((2, 2), np.uint64))
    assert np.isnan(empty.jaccard()).all() and empty.core == 0
