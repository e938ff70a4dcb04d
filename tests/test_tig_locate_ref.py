"""`locate` on the sparse minimizer index, without a GPU: the restatement (tig_locate_ref.py) against the arbiter
(kmer_locate_ref.py), the C ABI's declarations, the Python wrapper's refusals and the command line's flag rules."""
import ctypes as C
import random
import subprocess
import sys
import types
from pathlib import Path

import pytest

import kmer_locate_ref as LR
import tig_index_cases as cases
import tig_locate_ref as TL
from matchtigs_amd import _lib, api, synth

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = ("mtg_tig_index_build_locating", "mtg_tig_index_build_locating_store", "mtg_tig_index_is_locating", "mtg_tig_index_locate",
                "mtg_last_tig_locate_times")


def _agree(index, query, k, m, limit, what):
    ref = TL.TigLocateRef(index, k, m, limit)
    got, want = TL.locate(ref, query), LR.locate(index, query, k)
    for key in ("kmers", "valid", "found", "runs"):
        assert got[key] == want[key], (what, key, index, query)
    return ref


@pytest.mark.parametrize("k", [1, 2, 3, 5, 8, 12])
def test_restatement_on_random_pairs(k):
    """The minimum over all passing candidates (light) and the smallest table window (heavy) are loc, for every m and limit."""
    rng = random.Random(3000 + k)
    seen = {"heavy": False, "light": False, "minus": False, "long run": False}
    for i in range(25):
        index, query = cases.random_pair(rng, k)
        for m in sorted({1, min(2, k), -(-k // 2), k}) + [None]:
            for limit in (64, 1, 2):
                ref = _agree(index, query, k, m, limit, (k, i, m, limit))
                seen["heavy"] |= bool(ref.heavy_where)
                seen["light"] |= ref.anchors > 0
        runs = LR.locate(index, query, k)["runs"]
        seen["minus"] |= any(r[3] == 1 for r in runs)
        seen["long run"] |= any(r[2] > 1 for r in runs)
    assert all(seen.values()), seen


@pytest.mark.parametrize("k,m", [(5, 2), (12, 4), (31, 19), (33, 19)])
def test_the_first_passing_candidate_is_not_always_the_minimum(k, m):
    """On a reverse-complement palindrome the mirrored occurrence can lie earlier in the text while its anchor lies later."""
    rng = random.Random(100 * k + m)
    text, hard = TL.palindrome_case(rng, k, m)
    ref = TL.TigLocateRef([text], k, m)
    assert hard and all(ref.first_is_not_minimum(x) for x in hard)
    first = LR.first_positions([text], k)[0]
    for x in hard:
        c = ref.candidates(x)
        assert min(c) == first[synth.canonical(x)] == ref.where(x) and c[0] > min(c), (x, c)
    for limit in (64, 1):
        _agree([text], [text, synth.revcomp(text)] + hard, k, m, limit, (k, m, limit))


def test_hand_cases():
    for limit in (64, 1):
        ref = _agree(["AAAAAA"], ["AAAAA"], 3, None, limit, "poly-A")
        assert TL.locate(ref, ["AAAAA"])["runs"] == [(0, 0, 1, 0, 0, 0), (0, 1, 1, 0, 0, 0), (0, 2, 1, 0, 0, 0)]
    ref = _agree(["A", "C"], ["AC"], 1, None, 64, "k = 1")
    assert TL.locate(ref, ["AC"])["runs"] == [(0, 0, 1, 0, 0, 0), (0, 1, 1, 0, 1, 0)]
    index, query = cases.repeats_case(200, 9)
    ref = _agree(index, query, 9, 4, 8, "repeats")
    assert ref.heavy_where and ref.takes_heavy_path("A" * 9) and ref.where("A" * 9) == LR.first_positions(index, 9)[0]["A" * 9]


def test_entry_points_declared_and_exported(product_lib):
    names = _lib.declared_symbols()
    for n in ENTRY_POINTS:
        assert n in names and hasattr(product_lib, n), n
        assert getattr(product_lib, n).argtypes is not None, n
    assert product_lib.mtg_tig_index_is_locating.restype is C.c_int
    assert product_lib.mtg_tig_index_build_locating.restype is C.c_void_p
    assert len(product_lib.mtg_tig_index_locate.argtypes) == len(product_lib.mtg_kmer_index_locate.argtypes) == 8
    assert C.sizeof(_lib.MtgTigIndexInfo) == 8 * 12  # (no new field: the heavy positions show in device_bytes only)


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "mtg_engine.h"\n#include "matchtigs.h"\n'
                   "int main(void) {\n    uint64_t off[1] = {0}, kmers[1], valid[1], found[1];\n    double t[4];\n    mtg_kmer_runs *runs;\n"
                   "    mtg_tig_index_info i;\n"
                   "    mtg_tig_index *ix = mtg_tig_index_build_locating(\"\", off, 0, 31, 0, 0, 0);\n"
                   "    mtg_tig_index *iy = mtg_tig_index_build_locating_store((const mtg_unitigs *)0, 31, 0, 0, 0);\n"
                   "    int l = mtg_tig_index_is_locating(ix);\n"
                   "    mtg_tig_index_locate(ix, \"\", off, 0, kmers, valid, found, &runs);\n"
                   "    l += (int)mtg_kmer_runs_count(runs);\n    mtg_kmer_runs_free(runs);\n    mtg_last_tig_locate_times(t);\n"
                   "    mtg_tig_index_get_info(ix, &i);\n    mtg_tig_index_free(ix);\n    mtg_tig_index_free(iy);\n"
                   "    return l + (int)sizeof(i);\n}\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", str(ROOT / "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


DEATHS = [
    ("L.mtg_tig_index_locate(None, None, None, 0, None, None, None, None)", "mtg_tig_index_locate: null argument"),
    ("L.mtg_tig_index_is_locating(None)", "mtg_tig_index_is_locating: null argument"),
    ("L.mtg_tig_index_build_locating_store(None, 31, 0, 0, 0)", "mtg_tig_index_build_locating_store: null argument"),
    ("L.mtg_tig_index_build_locating(None, None, 1, 31, 0, 0, 0)", "mtg_tig_index_build_locating: null argument"),
    ("off = (C.c_uint64 * 2)(1, 5); L.mtg_tig_index_build_locating(b'ACGTA', off, 1, 3, 0, 0, 0)",
     "mtg_tig_index_build_locating: offsets must start at 0"),
    ("off = (C.c_uint64 * 3)(0, 5, 2); L.mtg_tig_index_build_locating(b'ACGTA', off, 2, 3, 0, 0, 0)",
     "mtg_tig_index_build_locating: offsets decrease at record 1"),
    ("off = (C.c_uint64 * 2)(0, 5); L.mtg_tig_index_build_locating(b'ACGTA', off, 1, 3, 4, 0, 0)", "mtg_tig_index_build_locating: the minimizer length 4"),
]


@pytest.mark.parametrize("i", range(len(DEATHS)))
def test_argument_checks_die_with_the_functions_name(product_lib, i):
    """Each is refused on the host, before a device is asked for: the child aborts with the entry point's name in the message."""
    code, message = DEATHS[i]
    r = subprocess.run([sys.executable, "-c", f"import ctypes as C\nfrom matchtigs_amd import _lib\nL = _lib.load()\n{code}\n"],
                       capture_output=True, text=True, cwd=str(ROOT), timeout=120)
    assert r.returncode != 0 and message in r.stderr, (code, r.returncode, r.stderr[-500:])


def _shell(locating, handle):
    ix = api.TigIndex.__new__(api.TigIndex)

    def asked(*a):
        raise AssertionError("the library was asked")

    ix._L = types.SimpleNamespace(mtg_tig_index_free=lambda h: None, mtg_tig_index_locate=asked)
    ix._h, ix.locating = handle, locating
    return ix


def test_locate_refuses_a_plain_and_a_closed_index():
    with pytest.raises(ValueError) as e:
        _shell(False, 1).locate(["ACGT"])
    assert "locate=True" in str(e.value)
    for locating in (False, True):
        with pytest.raises(ValueError) as e:
            _shell(locating, None).locate(["ACGT"])
        assert str(e.value) == "the index is closed"
    import inspect
    params = list(inspect.signature(api.TigIndex.__init__).parameters)
    assert params == ["self", "seqs_or_store", "k", "m", "device_id", "bucket_limit", "locate"]  # the new keyword goes last
    assert inspect.signature(api.TigIndex.__init__).parameters["locate"].default is False
    assert callable(api.last_tig_locate_times)


def _cli(*a):
    return subprocess.run([sys.executable, "-m", "matchtigs_amd", *a], capture_output=True, text=True, cwd=str(ROOT), timeout=300)


FLAG = "--query-index-locate-out"
BASE = ("--fa-in", "no_such.fa", "-k", "21")
REFUSED = [
    ((FLAG, "l.tsv"), [FLAG, "--query-fa"]),
    ((FLAG, "l.tsv", "--query-index", "minimizer"), [FLAG, "--query-fa"]),
    ((FLAG, "l.tsv", "--query-fa", "q.fa", "--query-index", "minimizer"), [FLAG, "--query-out"]),
    ((FLAG, "l.tsv", "--query-fa", "q.fa", "--query-out", "r.tsv"), [FLAG, "--query-index minimizer"]),
    ((FLAG, "l.tsv", "--query-fa", "q.fa", "--query-out", "r.tsv", "--query-index", "table"), [FLAG, "--query-index minimizer"]),
    ((FLAG, "l.tsv", "--query-fa", "q.fa", "--query-out", "r.tsv", "--query-index", "minimizer", "--query-locate-out", "m.tsv"),
     ["--query-locate-out", "--query-index minimizer"]),  # the table's flag stays refused beside the sparse index
]


@pytest.mark.parametrize("i", range(len(REFUSED)))
def test_flag_rules(i):
    given, parts = REFUSED[i]
    r = _cli(*(BASE + given))
    assert r.returncode == 2 and "error:" in r.stderr, (given, r.stderr[-500:])
    last = r.stderr.strip().splitlines()[-1]
    for part in parts:
        assert part in last, (given, last)


def test_accepted_flags_get_as_far_as_the_input(tmp_path):
    query = ("--query-fa", "q.fa", "--query-out", str(tmp_path / "r.tsv"), "--query-index", "minimizer", FLAG)
    for extra in ((str(tmp_path / "l.tsv"),), (str(tmp_path / "l.tsv.gz"), "--query-index-over", "input"),
                  (str(tmp_path / "l.tsv"), "--query-index-over", "greedytigs", "--greedytigs-fa-out", str(tmp_path / "g.fa")),
                  (str(tmp_path / "l.tsv"), "--query-index-over", "eulertigs", "--eulertigs-fa-out", str(tmp_path / "e.fa"),
                   "--query-minimizer-length", "11")):
        r = _cli("--fa-in", str(tmp_path / "no_such.fa"), "-k", "21", *query, *extra)
        assert r.returncode != 0 and "error:" not in r.stderr and "cannot open" in r.stderr, (extra, r.stderr[-1000:])
    assert FLAG in _cli("--help").stdout
