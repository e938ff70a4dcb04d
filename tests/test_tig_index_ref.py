"""What of the sparse minimizer index (mtg_tig_index_*, api.TigIndex, `--query-index`) can be checked without a GPU:
the restatement of the scheme (tig_index_ref.py) against the k-mer index's restatement (kmer_query_ref.py: a Python set) on the
hazards the GPU test runs -- it carries the exactness argument --, the C-ABI's declarations, the default minimizer length, the flag
rules of the command line and the closed index."""
import ctypes as C
import random
import subprocess
import sys
import types
from pathlib import Path

import numpy as np
import pytest

import kmer_query_ref as R
import tig_index_cases as cases
import tig_index_ref as T
from matchtigs_amd import _lib, api, synth

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = ("mtg_tig_index_build", "mtg_tig_index_build_store", "mtg_tig_index_get_info", "mtg_tig_index_query", "mtg_tig_index_free",
                "mtg_last_tig_index_times")


def _agree(index, query, k, m, limit, what):
    ix = T.TigIndexRef(index, k, m, limit or 64)
    got, want = T.query(ix, query, k), R.query(R.index_set(index, k), query, k)
    assert got == want, (what, k, m, limit)
    return ix, want


@pytest.mark.parametrize("k", [1, 2, 3, 5, 8, 12])
def test_restatement_on_random_pairs(k):
    rng = random.Random(2800 + k)
    heavy = light = found = absent = 0
    for i in range(25):
        index, query = cases.random_pair(rng, k)
        for m in cases.random_ms(k):
            for limit in (None, 1, 2):
                ix, want = _agree(index, query, k, m, limit, f"pair {i}")
                heavy += ix.heavy_windows
                light += ix.occurrences - ix.heavy_windows
                found += sum(want["found"])
                absent += sum(want["valid"]) - sum(want["found"])
    assert heavy and light and found and absent, (k, heavy, light, found, absent)  # (both paths, both answers)


def test_restatement_on_the_engineered_cases():
    names = set()
    for name, index, query, k, m, limit in cases.engineered():
        for lim in (limit, 1):
            _agree(index, query, k, m, lim, name)
        names.add(name.split(",")[0].split(" k=")[0])
    assert {"minimizer twice", "palindromic minimizer", "palindromic k-mer", "record borders", "record ends", "short records",
            "only short records"} <= names


def test_concatenation_kmers_are_not_found():
    name, index, query, k, m, limit = next(c for c in cases.engineered() if c[0] == "record borders k=31")
    _, want = _agree(index, query, k, m, limit, name)
    assert want["found"][:3 * (k - 1)] == [0] * (3 * (k - 1)) and want["valid"][:3 * (k - 1)] == [1] * (3 * (k - 1))
    assert want["found"][-3:] == [2 * k - k + 1, 2, 1]  # (the records themselves are all there)


def test_repeats_take_the_heavy_path():
    k = 15
    index, query = cases.repeats_case(300, k)
    ix, want = _agree(index, query, k, None, None, "repeats")
    assert len(ix.heavy) >= 1 and ix.heavy_windows >= 2 * (300 - k + 1) and ix.anchors > 0
    assert want["found"][:6] == [1, 1, 1, 1, k + 1, k + 1]
    n_neighbours = len(cases.neighbours("A" * k)[::3]) + len(cases.neighbours(("AC" * k)[:k])[::3])
    assert want["found"][6:6 + n_neighbours] == [0] * n_neighbours
    # the same with a limit nothing exceeds: no table, the same answers
    flat = T.TigIndexRef(index, k, None, 10 ** 6)
    assert not flat.heavy and flat.heavy_windows == 0 and T.query(flat, query, k) == want


def test_anchor_density_and_the_numpy_count():
    """2 / (w + 1) of the windows of random sequence are anchors; the vectorised count the size test uses equals the restatement's."""
    rng = random.Random(7)
    k, m = 31, 19
    seqs = [cases.dna(rng, n) for n in (3000, 0, 40, 30, 2500)]
    ix = T.TigIndexRef(seqs, k, m, 10 ** 6)
    density = ix.anchors / ix.occurrences
    assert abs(density - 2 / (k - m + 2)) < 0.02, density
    seq = np.frombuffer("".join(seqs).encode(), np.uint8)
    off = np.array([0] + list(np.cumsum([len(s) for s in seqs])), np.uint64)
    assert T.anchor_count_arrays(seq, off, k, m) == ix.anchors


def test_default_minimizer_length():
    want = {1: 1, 2: 2, 5: 4, 31: 19, 64: 19}
    for k, m in want.items():
        assert api.default_minimizer_length(k) == m == T.default_m(k), k


def test_entry_points_declared_and_exported(product_lib):
    names = _lib.declared_symbols()
    for n in ENTRY_POINTS:
        assert n in names and hasattr(product_lib, n), n
    fields = ["k", "m", "records", "characters", "occurrences", "anchors", "buckets", "bucket_limit", "heavy_buckets", "heavy_windows",
              "table_slots", "device_bytes"]
    assert C.sizeof(_lib.MtgTigIndexInfo) == 8 * len(fields) and [f for f, _ in _lib.MtgTigIndexInfo._fields_] == fields
    assert [f.name for f in api.TigIndexInfo.__dataclass_fields__.values()] == fields


def test_headers_compile_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "mtg_engine.h"\n#include "matchtigs.h"\n'
                   "int main(void) {\n    mtg_tig_index_info i;\n    double t[8];\n    mtg_tig_index *ix = mtg_tig_index_build(\"\", 0, 0, 31, 0, 0, 0);\n"
                   "    mtg_tig_index_get_info(ix, &i);\n    mtg_last_tig_index_times(t);\n    mtg_tig_index_free(ix);\n    return (int)i.anchors;\n}\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", str(ROOT / "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_info_properties():
    info = api.TigIndexInfo(k=31, m=19, records=2, characters=1000, occurrences=940, anchors=130, buckets=256, bucket_limit=64,
                            heavy_buckets=0, heavy_windows=0, table_slots=0, device_bytes=3760)
    assert info.bytes_per_kmer == 4.0
    text = info.describe()
    for part in ("m = 19", "1000 bases", "130 anchors", "0 heavy buckets", "3760 device bytes", "4.00 bytes per k-mer window"):
        assert part in text, (part, text)
    with pytest.raises(Exception):
        info.k = 3  # frozen
    assert api.TigIndexInfo(**{**info.__dict__, "occurrences": 0}).bytes_per_kmer == 0.0


def test_a_closed_index_refuses():
    ix = api.TigIndex.__new__(api.TigIndex)
    ix._L = types.SimpleNamespace(mtg_tig_index_free=lambda h: None)
    ix._h = None
    with pytest.raises(ValueError) as e:
        ix.query(["ACGT"])
    assert str(e.value) == "the index is closed"
    ix.close()
    for bad in ({"m": 0}, {"m": 6}, {"m": 32, "k": 40}, {"bucket_limit": 0}, {"bucket_limit": 65537}):
        with pytest.raises(ValueError):
            api.TigIndex(["ACGTACGT"], bad.pop("k", 5), **bad)  # (refused before the library is asked)


def _cli(*a):
    return subprocess.run([sys.executable, "-m", "matchtigs_amd", *a], capture_output=True, text=True, cwd=str(ROOT), timeout=300)


BASE = ("--fa-in", "no_such.fa", "-k", "21")
QUERY = ("--query-fa", "q.fa", "--query-out", "r.tsv")
REFUSED = [
    (("--query-index", "minimizer"), ["--query-index needs --query-fa"]),
    (("--query-index", "table"), ["--query-index needs --query-fa"]),
    (("--query-minimizer-length", "9"), ["--query-minimizer-length needs --query-fa"]),
    (("--query-index-over", "input"), ["--query-index-over needs --query-fa"]),
    (QUERY + ("--query-minimizer-length", "9"), ["--query-minimizer-length needs --query-index minimizer"]),
    (QUERY + ("--query-index", "table", "--query-minimizer-length", "9"), ["--query-minimizer-length needs --query-index minimizer"]),
    (QUERY + ("--query-index", "minimizer", "--query-minimizer-length", "0"), ["--query-minimizer-length must be in 1..21"]),
    (QUERY + ("--query-index", "minimizer", "--query-minimizer-length", "22"), ["--query-minimizer-length must be in 1..21"]),
    (("-k", "40") + QUERY + ("--query-index", "minimizer", "--query-minimizer-length", "32"), ["--query-minimizer-length must be in 1..31"]),
    (QUERY + ("--query-index-over", "greedytigs"), ["--query-index-over greedytigs needs --greedytigs-fa-out"]),
    (QUERY + ("--query-index-over", "eulertigs", "--greedytigs-fa-out", "g.fa"), ["--query-index-over eulertigs needs --eulertigs-fa-out"]),
    (QUERY + ("--query-index", "hash"), ["--query-index", "invalid choice"]),
    (QUERY + ("--query-index-over", "matchtigs"), ["--query-index-over", "invalid choice"]),
]
for _flag, _extra in (("--query-locate-out", ()), ("--query-abundance-out", ()), ("--query-abundance-profile-out", ("--query-abundance-out", "a.tsv")),
                      ("--query-colors-out", ())):
    _given = ("--seq-in", "no_such.fa", "-k", "21") + QUERY + (_flag, "x.out") + _extra
    REFUSED.append((_given + ("--query-index", "minimizer"), [_flag, "--query-index minimizer"]))
    REFUSED.append((_given + ("--query-index-over", "greedytigs", "--greedytigs-fa-out", "g.fa"), [_flag, "--query-index-over greedytigs"]))
    REFUSED.append((_given + ("--query-index-over", "eulertigs", "--eulertigs-fa-out", "e.fa"), [_flag, "--query-index-over eulertigs"]))


@pytest.mark.parametrize("i", range(len(REFUSED)))
def test_flag_rules(i):
    """Each refusal is argparse's own (exit status 2, `error:`): it comes before the library is loaded, let alone a GPU used."""
    given, parts = REFUSED[i]
    r = _cli(*(given if "--seq-in" in given else BASE + given))
    assert r.returncode == 2 and "error:" in r.stderr, (given, r.stderr[-500:])
    last = r.stderr.strip().splitlines()[-1]
    for part in parts:
        assert part in last, (given, last)


def test_accepted_flags_get_as_far_as_the_input(tmp_path):
    for extra in (("--query-index", "table"), ("--query-index", "minimizer", "--query-minimizer-length", "21"),
                  ("--query-index-over", "input", "--query-locate-out", str(tmp_path / "l.tsv")),
                  ("--query-index", "minimizer", "--query-index-over", "greedytigs", "--greedytigs-fa-out", str(tmp_path / "g.fa"))):
        r = _cli("--fa-in", str(tmp_path / "no_such.fa"), "-k", "21", "--query-fa", "q.fa", "--query-out", str(tmp_path / "r.tsv"), *extra)
        assert r.returncode != 0 and "error:" not in r.stderr and "cannot open" in r.stderr, (extra, r.stderr[-1000:])
    r = _cli("--help")
    for flag in ("--query-index", "--query-minimizer-length", "--query-index-over"):
        assert flag in r.stdout
