"""Tallies by position on the sparse minimizer index, without a GPU: the restatement (tig_tally_ref.py) against the
arbiter (kmer_tally_ref.py), hand cases for the ordinal, the invariants of the counters, the generator of the GPU test, the C ABI's
declarations, the host-side refusals of the library, the Python wrapper's errors and the command line's flag rules."""
import ctypes as C
import random
import subprocess
import sys
import types
from pathlib import Path

import pytest

import kmer_query_ref as Q
import kmer_tally_ref as KT
import tig_index_cases as cases
import tig_index_ref as T
import tig_locate_ref as TL
import tig_payload_ref as TP
import tig_tally_ref as TT
from matchtigs_amd import _lib, api, synth

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = ("mtg_tig_tally_create", "mtg_tig_tally_device_bytes", "mtg_tig_tally_windows", "mtg_tig_tally_add", "mtg_tig_tally_add_store",
                "mtg_tig_tally_coverage", "mtg_tig_tally_coverage_store", "mtg_tig_tally_counters", "mtg_tig_tally_reset", "mtg_tig_tally_free",
                "mtg_last_tig_tally_times")
GPU_KS = [1, 2, 3, 5, 16, 31, 32, 33, 64, 101]  # test_gpu_tig_tally.py's
GPU_PAIRS = 3


def _agree(index, adds, asked, k, m, limit, what):
    """Every output of the restatement equals the arbiter's; returns the restatement after the adds."""
    ref = TL.TigLocateRef([s.upper() for s in index], k, m, limit)
    tally = TT.TigTallyRef(ref)
    index_kmers = Q.index_set(index, k)
    found = 0
    for n, seqs in enumerate(adds):
        got = tally.add(seqs)
        want = Q.query(index_kmers, seqs, k)
        assert got == {f: want[f] for f in ("kmers", "valid", "found")}, (what, "add", n, index, seqs)
        found += sum(got["found"])
        counts = KT.tally(index_kmers, adds[:n + 1], k)
        for seqs2 in asked:
            assert tally.coverage(seqs2) == KT.coverage(index_kmers, counts, seqs2, k), (what, "coverage", n, index, adds, seqs2)
    # the invariants: the count of a class sits at its first window and nowhere else; nothing is lost
    assert tally.counters() == TT.counters_by_dictionary(index, adds, k), (what, index, adds)
    assert sum(tally.counters()) == found
    return ref, tally


@pytest.mark.parametrize("k", [1, 2, 3, 5, 8, 12])
def test_restatement_on_random_pairs(k):
    """counter[ordinal(where)] is the class's counter, for every m and limit, over two accumulating adds."""
    rng = random.Random(3200 + k)
    seen = {"heavy": False, "light": False, "later occurrence holds 0": False}
    for i in range(8):
        index, query = cases.random_pair(rng, k)
        _, more = cases.random_pair(rng, k)
        adds = [query, more + index]
        for m in sorted({1, -(-k // 2), k}) + [None]:
            for limit in (64, 1, 2):
                ref, tally = _agree(index, adds, [index, query], k, m, limit, (k, i, m, limit))
                seen["heavy"] |= bool(ref.heavy_where)
                seen["light"] |= ref.anchors > 0
                _, _, first, windows = TT.first_windows(index, k)
                seen["later occurrence holds 0"] |= windows > len(first) and sum(tally.counters()) > 0
    assert all(seen.values()), seen


@pytest.mark.parametrize("k,m", [(5, 2), (12, 4), (31, 19), (33, 19)])
def test_palindromes_count_at_the_minimum(k, m):
    """Inside a reverse-complement palindrome a class occurs twice; a kernel that took the first passing candidate would split the
    class over two counters. The counter is the one at the minimum."""
    rng = random.Random(100 * k + m)
    text, hard = TL.palindrome_case(rng, k, m)
    ref = TL.TigLocateRef([text], k, m)
    differing = 0
    for x in hard:
        c = ref.candidates(x)
        tally = TT.TigTallyRef(ref)
        tally.add([x, synth.revcomp(x)])
        at_first, at_min = TP.ordinal(ref.off, k, c[0]), TP.ordinal(ref.off, k, min(c))
        differing += at_first != at_min
        assert tally.counters()[at_min] == 2 and sum(tally.counters()) == 2, x
    assert differing >= 1  # (a generator that never produces such a window fails here)
    adds = [[text, synth.revcomp(text)] + hard, hard]
    for limit in (64, 1):
        _agree([text], adds, [[text], hard], k, m, limit, (k, m, limit))


def test_ordinals_by_hand():
    k = 4
    # records shorter than k and empty records between: windows 0..2 in record 1, 3..5 in record 5
    index = ["ACG", "AACCGT", "", "TT", "", "GATTAC", "C"]
    ref = TL.TigLocateRef(index, k, 2)
    tally = TT.TigTallyRef(ref)
    assert tally.win_off == [0, 0, 3, 3, 3, 3, 6, 6] and tally.windows == 6
    tally.add(["TTAC"])  # the last window of the text: the last ordinal
    assert tally.counters() == [0, 0, 0, 0, 0, 1]
    tally.add(["AACC", "GGTT", "CCGT", "ACGG"])  # ordinal 0 twice (the second reverse-complemented), ordinal 2 twice likewise
    assert tally.counters() == [2, 0, 2, 0, 0, 1]
    tally.add(["ACGA", "TTTT", "GTTT"])  # the concatenation spells these, no record does
    assert tally.counters() == [2, 0, 2, 0, 0, 1]
    cov = tally.coverage(index)
    assert (cov["covered"], cov["sum"], cov["max"]) == ([0, 2, 0, 0, 0, 1, 0], [0, 4, 0, 0, 0, 1, 0], [0, 2, 0, 0, 0, 1, 0])
    assert cov["per_window"][3:6] == [2, 0, 2] and sum(cov["per_window"]) == 5
    tally.reset()
    assert tally.counters() == [0] * 6
    # a class planted forward in record 3 and reverse-complemented in record 1: the count sits in record 1
    x = "ACCGGTTA"[:6] + "C"  # ACCGGTC, not its own reverse complement
    index = ["GGGGGGGGG", "TT" + synth.revcomp(x) + "TT", "CCCCCCCCC", "AA" + x + "AA"]
    k = len(x)
    for m, limit in ((3, 64), (3, 1), (7, 64), (1, 1)):
        ref = TL.TigLocateRef(index, k, m, limit)
        tally = TT.TigTallyRef(ref)
        tally.add([x, x, synth.revcomp(x)])
        want = [0] * tally.windows
        want[tally.win_off[1] + 2] = 3
        assert tally.counters() == want, (m, limit)
        cov = tally.coverage(index)
        assert cov["sum"] == [0, 3, 0, 3] and cov["covered"] == [0, 1, 0, 1]
    _agree(index, [[x, x, synth.revcomp(x)], index], [index], k, 3, 64, "planted")


def test_engineered_inputs_agree_with_the_arbiter():
    for name, index, query, k, m, limit in cases.engineered():
        _agree(index, [query, query[::2]], [index, query], k, m, limit or 64, name)


@pytest.mark.parametrize("k", GPU_KS)
def test_the_gpu_tests_generator_shows_every_hazard(k):
    """The pairs test_gpu_tig_tally.py draws (same seeds) complete its `seen` dictionary at every k, heavy and light paths included."""
    rng = random.Random(3240 + k)
    seen = dict.fromkeys(TT.needed(k) + ("heavy", "light"), False)
    for i in range(GPU_PAIRS):
        index, query = TT.tally_pair(rng, k)
        assert 3 <= len(index) <= 83
        for f, v in TT.seen_flags(index, query, k).items():
            if f in seen:
                seen[f] |= v
        if i == 0:  # (the paths: one pair says enough)
            for m in cases.random_ms(k):
                for limit in (64, 1, 2):
                    ref = T.TigIndexRef([s.upper() for s in index], k, m, limit)
                    seen["heavy"] |= ref.heavy_windows > 0
                    seen["light"] |= ref.heavy_windows < ref.occurrences
    assert all(seen.values()), (k, seen)


def test_the_generators_cases_agree_with_the_arbiter():
    rng = random.Random(3240 + 5)
    index, query = TT.tally_pair(rng, 5)
    for limit in (64, 1):
        _agree(index, [query, query[:7]], [index, query], 5, None, limit, ("generator", limit))


def test_entry_points_declared_and_exported(product_lib):
    names = _lib.declared_symbols()
    for n in ENTRY_POINTS:
        assert n in names and hasattr(product_lib, n), n
        assert getattr(product_lib, n).argtypes is not None, n
    nm = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "matchtigs_amd" / "libmatchtigs.so")], capture_output=True, text=True)
    exported = {line.split()[-1] for line in nm.stdout.splitlines() if line.strip()}
    assert nm.returncode == 0 and set(ENTRY_POINTS) <= exported  # unmangled
    L = product_lib
    assert L.mtg_tig_tally_create.restype is C.c_void_p
    assert L.mtg_tig_tally_device_bytes.restype is C.c_uint64 and L.mtg_tig_tally_windows.restype is C.c_uint64
    for mine, table in (("mtg_tig_tally_add", "mtg_kmer_tally_add"), ("mtg_tig_tally_add_store", "mtg_kmer_tally_add_store"),
                        ("mtg_tig_tally_coverage", "mtg_kmer_tally_coverage"), ("mtg_tig_tally_coverage_store", "mtg_kmer_tally_coverage_store"),
                        ("mtg_tig_tally_reset", "mtg_kmer_tally_reset"), ("mtg_tig_tally_free", "mtg_kmer_tally_free")):
        assert getattr(L, mine).argtypes == getattr(L, table).argtypes and getattr(L, mine).restype is None, mine
    assert len(L.mtg_tig_tally_counters.argtypes) == 2
    assert C.sizeof(_lib.MtgTigIndexInfo) == 8 * 12  # (unchanged: a tally says its own bytes)


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "mtg_engine.h"\n#include "matchtigs.h"\n'
                   "int main(void) {\n    uint64_t off[1] = {0}, kmers[1], valid[1], found[1], covered[1], sum[1], max[1], pw[1], out[1];\n"
                   "    double t[5];\n    mtg_tig_index_info i;\n"
                   "    mtg_tig_index *ix = mtg_tig_index_build_locating(\"\", off, 0, 31, 0, 0, 0);\n"
                   "    mtg_tig_tally *ta = mtg_tig_tally_create(ix);\n"
                   "    uint64_t n = mtg_tig_tally_device_bytes(ta) + mtg_tig_tally_windows(ta);\n"
                   "    mtg_tig_tally_add(ta, \"\", off, 0, kmers, valid, found);\n"
                   "    mtg_tig_tally_add_store(ta, (const mtg_unitigs *)0, kmers, valid, found);\n"
                   "    mtg_tig_tally_coverage(ta, \"\", off, 0, kmers, valid, found, covered, sum, max, pw);\n"
                   "    mtg_tig_tally_coverage_store(ta, (const mtg_unitigs *)0, kmers, valid, found, covered, sum, max, (uint64_t *)0);\n"
                   "    mtg_tig_tally_counters(ta, out);\n    mtg_tig_tally_reset(ta);\n    mtg_last_tig_tally_times(t);\n"
                   "    mtg_tig_tally_free(ta);\n    mtg_tig_tally_free((mtg_tig_tally *)0);\n"
                   "    mtg_tig_index_get_info(ix, &i);\n    mtg_tig_index_free(ix);\n"
                   "    return (int)n + (int)sizeof(i);\n}\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", str(ROOT / "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


DEATHS = [
    ("L.mtg_tig_tally_create(None)", "mtg_tig_tally_create: null argument"),
    ("L.mtg_tig_tally_device_bytes(None)", "mtg_tig_tally_device_bytes: null argument"),
    ("L.mtg_tig_tally_windows(None)", "mtg_tig_tally_windows: null argument"),
    ("L.mtg_tig_tally_add(None, None, None, 0, None, None, None)", "mtg_tig_tally_add: null argument"),
    ("L.mtg_tig_tally_add_store(None, None, None, None, None)", "mtg_tig_tally_add_store: null argument"),
    ("L.mtg_tig_tally_coverage(None, None, None, 0, None, None, None, None, None, None, None)", "mtg_tig_tally_coverage: null argument"),
    ("L.mtg_tig_tally_coverage_store(None, None, None, None, None, None, None, None, None)", "mtg_tig_tally_coverage_store: null argument"),
    ("L.mtg_tig_tally_counters(None, None)", "mtg_tig_tally_counters: null argument"),
    ("L.mtg_tig_tally_reset(None)", "mtg_tig_tally_reset: null argument"),
]


@pytest.mark.parametrize("i", range(len(DEATHS)))
def test_argument_checks_die_with_the_functions_name(product_lib, i):
    """Each is refused on the host, before a device is asked for: the child aborts with the entry point's name in the message."""
    code, message = DEATHS[i]
    r = subprocess.run([sys.executable, "-c", f"import ctypes as C\nfrom matchtigs_amd import _lib\nL = _lib.load()\n{code}\n"],
                       capture_output=True, text=True, cwd=str(ROOT), timeout=120)
    assert r.returncode != 0 and message in r.stderr, (code, r.returncode, r.stderr[-500:])


def test_free_accepts_null(product_lib):
    product_lib.mtg_tig_tally_free(None)
    out = (C.c_double * 5)()
    product_lib.mtg_last_tig_tally_times(out)
    assert list(out) == [0.0] * 5  # (no call on this thread yet)


def _asked(*a, **kw):
    raise AssertionError("the library was asked")


def _shell_index(handle, locating=True):
    ix = api.TigIndex.__new__(api.TigIndex)
    ix._L = types.SimpleNamespace(mtg_tig_index_free=lambda h: None, mtg_tig_tally_create=_asked, mtg_tig_tally_add=_asked,
                                  mtg_tig_tally_coverage=_asked, mtg_tig_tally_counters=_asked, mtg_tig_tally_reset=_asked,
                                  mtg_tig_tally_free=lambda h: None)
    ix._h, ix.locating, ix.weighted, ix.colored, ix.n_colors = handle, locating, False, False, 0
    return ix


def _shell_tally(index, handle):
    t = api.TigTally.__new__(api.TigTally)
    t.index, t._L, t._h, t.windows, t.device_bytes = index, index._L, handle, 3, 24
    return t


def test_the_wrappers_errors_come_before_the_library(monkeypatch):
    monkeypatch.setattr(_lib, "load", _asked)
    table = api.KmerIndex.__new__(api.KmerIndex)
    table._h = None
    with pytest.raises(TypeError) as e:
        api.TigTally(table)
    assert str(e.value) == "TigTally counts on a TigIndex"
    with pytest.raises(TypeError) as e:
        api.KmerTally(_shell_index(1))  # (KmerTally's own refusal stays)
    assert str(e.value) == "KmerTally counts on a KmerIndex"
    with pytest.raises(TypeError):
        api.TigTally(["ACGT"])
    with pytest.raises(ValueError) as e:
        api.TigTally(_shell_index(None))
    assert str(e.value) == "the index is closed"
    with pytest.raises(ValueError) as e:
        api.TigTally(_shell_index(1, locating=False))
    assert "locate=True" in str(e.value)
    calls = (lambda t: t.add(["ACGT"]), lambda t: t.coverage(["ACGT"]), lambda t: t.coverage(["ACGT"], per_window=True),
             lambda t: t.counters(), lambda t: t.reset())
    for call in calls:
        with pytest.raises(ValueError) as e:
            call(_shell_tally(_shell_index(1), None))
        assert str(e.value) == "the tally is closed"
        with pytest.raises(ValueError) as e:
            call(_shell_tally(_shell_index(None), 1))
        assert str(e.value) == "the index is closed"
    t = _shell_tally(_shell_index(1), 1)
    with t as same:
        assert same is t and t.index._h == 1
    assert t._h is None
    t.close()  # (twice is fine)
    with pytest.raises(ValueError) as e:
        t.add(["ACGT"])
    assert str(e.value) == "the tally is closed"
    import matchtigs_amd

    assert matchtigs_amd.TigTally is api.TigTally and matchtigs_amd.last_tig_tally_times is api.last_tig_tally_times


def test_the_library_refuses_a_non_locating_index():
    """mtg_tig_tally_create's own message names the build that is needed (the wrapper never gets that far). Without a GPU the build of
    the index dies first, with another message; the text is then checked in the source."""
    source = (ROOT / "matchtigs_amd" / "csrc" / "tig_index_device.hip").read_text()
    at = source.index("TigTally *device_tig_tally_create")
    body = source[at:at + 600]
    assert "if (!ix->locating) MTG_DIE(" in body and "mtg_tig_index_build_locating" in body and '"mtg_tig_tally_create"' in body


def _cli(*a):
    return subprocess.run([sys.executable, "-m", "matchtigs_amd", *a], capture_output=True, text=True, cwd=str(ROOT), timeout=300)


CI, CM, CO = "--count-index", "--count-minimizer-length", "--count-index-over"
COUNT = ("--count-fa", "s.fa", "--count-out", "c.tsv")
SPARSE = (CI, "minimizer")
REFUSED = [
    (("--fa-in", "x.fa", "--greedytigs-fa-out", "g.fa", CI, "minimizer"), [CI, "--count-fa"]),
    (("--fa-in", "x.fa", "--greedytigs-fa-out", "g.fa", CI, "table"), [CI, "--count-fa"]),
    (("--fa-in", "x.fa", *COUNT, CM, "11"), [CM, "--count-index minimizer"]),
    (("--fa-in", "x.fa", *COUNT, CM, "11", CI, "table"), [CM, "--count-index minimizer"]),
    (("--fa-in", "x.fa", *COUNT, CO, "input"), [CO, "--count-index minimizer"]),
    (("--fa-in", "x.fa", *COUNT, CO, "greedytigs", "--greedytigs-fa-out", "g.fa", CI, "table"), [CO, "--count-index minimizer"]),
    (("--fa-in", "x.fa", *COUNT, *SPARSE, CM, "0"), [CM, "1..21", "--query-minimizer-length"]),
    (("--fa-in", "x.fa", *COUNT, *SPARSE, CM, "22"), [CM, "1..21", "--query-minimizer-length"]),
    (("--fa-in", "x.fa", *COUNT, *SPARSE, CO, "greedytigs"), [CO + " greedytigs", "--greedytigs-fa-out"]),
    (("--fa-in", "x.fa", *COUNT, *SPARSE, CO, "eulertigs", "--greedytigs-fa-out", "g.fa"), [CO + " eulertigs", "--eulertigs-fa-out"]),
    (("--seq-in", "x.fa", *COUNT, *SPARSE, CO, "eulertigs"), [CO + " eulertigs", "--eulertigs-fa-out"]),
]


@pytest.mark.parametrize("i", range(len(REFUSED)))
def test_flag_rules(i):
    given, parts = REFUSED[i]
    r = _cli("-k", "21", *given)
    assert r.returncode == 2 and "error:" in r.stderr, (given, r.stderr[-500:])
    last = r.stderr.strip().splitlines()[-1]
    for part in parts:
        assert part in last, (given, last)


def test_the_range_of_m_follows_k():
    r = _cli("-k", "40", "--fa-in", "x.fa", *COUNT, *SPARSE, CM, "32")
    assert r.returncode == 2 and "1..31" in r.stderr.strip().splitlines()[-1]
    r = _cli("-k", "40", "--fa-in", "x.fa", *COUNT, CI, "sparse")
    assert r.returncode == 2 and "invalid choice" in r.stderr


@pytest.mark.parametrize("route", ["--seq-in", "--fa-in", "--bcalm-in"])
def test_accepted_flags_get_as_far_as_the_input(tmp_path, route):
    t = lambda name: str(tmp_path / name)
    count = ("--count-fa", "s.fa", "--count-out", t("c.tsv"))
    query = ("--query-fa", "q.fa", "--query-out", t("r.tsv"), "--query-index", "minimizer")
    for extra in ((CI, "table"), SPARSE, (*SPARSE, CM, "11"), (*SPARSE, CO, "input", CM, "21"),
                  (*SPARSE, CO, "greedytigs", "--greedytigs-fa-out", t("g.fa")),
                  (*SPARSE, CO, "eulertigs", "--eulertigs-fa-out", t("e.fa"), CM, "1"),
                  (*SPARSE, *query), (*SPARSE, *query, CM, "11", "--query-index-locate-out", t("l.tsv")),
                  (*SPARSE, *query, "--query-index-over", "greedytigs", CO, "greedytigs", "--greedytigs-fa-out", t("g.fa"))):
        r = _cli(route, t("no_such.fa"), "-k", "21", *count, *extra)
        assert r.returncode != 0 and "error:" not in r.stderr and "cannot open" in r.stderr, (extra, r.stderr[-1000:])


def test_help_names_the_flags():
    out = _cli("--help").stdout
    for flag in (CI, CM, CO):
        assert flag in out
