"""Payloads by position on the sparse minimizer index, without a GPU: the restatement (tig_payload_ref.py) against the
arbiters (kmer_abundance_ref.py, kmer_color_ref.py), the layout and byte rules, the generator of the GPU test, the C ABI's
declarations, the host-side refusals of the library, the Python wrapper's ValueErrors and the command line's flag rules."""
import ctypes as C
import inspect
import random
import subprocess
import sys
import types
from pathlib import Path

import pytest

import kmer_abundance_ref as KA
import kmer_color_ref as KC
import tig_index_cases as cases
import tig_index_ref as T
import tig_locate_ref as TL
import tig_payload_ref as TP
from matchtigs_amd import _lib, api, synth

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = ("mtg_tig_index_build_annotated", "mtg_tig_index_build_annotated_store", "mtg_tig_index_is_weighted", "mtg_tig_index_is_colored",
                "mtg_tig_index_get_payload_info", "mtg_tig_index_abundance", "mtg_tig_index_colors", "mtg_last_tig_payload_times")
GPU_KS = [1, 2, 3, 5, 16, 31, 32, 33, 64, 101]  # test_gpu_tig_payload.py's
GPU_PAIRS = 8


def _agree(index, query, k, m, limit, weights, masks, n_colors, what):
    ref = TL.TigLocateRef([s.upper() for s in index], k, m, limit)
    want_a, want_c = KA.abundance(index, weights, query, k), KC.color_hits(index, masks, n_colors, query, k)
    for layout in ("dense", "runs"):
        got = TP.abundance(ref, TP.Payload(weights, "weights", layout=layout), query)
        assert got == want_a, (what, layout, "abundance", index, query, weights)
        got = TP.color_hits(ref, TP.Payload(masks, "colors", n_colors, layout), n_colors, query)
        assert got == want_c, (what, layout, "colors", index, query, masks)
    return ref


@pytest.mark.parametrize("k", [1, 2, 3, 5, 8, 12])
def test_restatement_on_random_pairs(k):
    """The payload at the smallest position of the class is the payload of the class's first window, for every m, limit and layout."""
    rng = random.Random(3100 + k)
    seen = {"heavy": False, "light": False}
    for i in range(10):
        index, query = cases.random_pair(rng, k)
        windows = sum(max(0, len(s) - k + 1) for s in index)
        weights = TP.runny(rng, windows, [0, 1, 7, 300, 70000, (1 << 32) - 1])
        n_colors = rng.choice([1, 3, 8, 9, 33, 64])
        masks = TP.runny(rng, windows, [0, 1, (1 << n_colors) - 1, 1 << (n_colors - 1), rng.randint(0, (1 << n_colors) - 1)])
        for m in sorted({1, -(-k // 2), k}) + [None]:
            for limit in (64, 1, 2):
                ref = _agree(index, query, k, m, limit, weights, masks, n_colors, (k, i, m, limit))
                seen["heavy"] |= bool(ref.heavy_where)
                seen["light"] |= ref.anchors > 0
    assert all(seen.values()), seen


@pytest.mark.parametrize("k,m", [(5, 2), (12, 4), (31, 19), (33, 19)])
def test_palindromes_take_the_payload_at_the_minimum(k, m):
    """The two occurrences of a class inside a reverse-complement palindrome carry different weights; the first passing candidate's is
    not the answer, the one at the minimum is."""
    rng = random.Random(100 * k + m)
    text, hard = TL.palindrome_case(rng, k, m)
    ref = TL.TigLocateRef([text], k, m)
    weights, pairs = TP.palindrome_weights(ref, text, hard)
    assert hard and len(pairs) == len(hard)
    want = KA.class_weights([text], weights, k)
    differing = 0
    for x, (at_first, at_min) in zip(hard, pairs):
        assert want[synth.canonical(x)] == at_min, x
        differing += at_first != at_min
        got = TP.abundance(ref, TP.Payload(weights), [x])
        assert (got["sum"], got["min"], got["max"]) == ([at_min], [at_min], [at_min])
    assert differing >= 1  # (a generator that never produces such a window fails here)
    query = [text, synth.revcomp(text)] + hard
    masks = [w % 7 for w in weights]
    for limit in (64, 1):
        _agree([text], query, k, m, limit, weights, masks, 3, (k, m, limit))


def test_layout_width_and_bytes():
    P = TP.Payload
    assert TP.runs_of([]) == ([], []) and TP.runs_of([5, 5, 5]) == ([0], [5]) and TP.runs_of([1, 2, 2, 1]) == ([0, 1, 3], [1, 2, 1])
    for top, width in ((0, 1), (255, 1), (256, 2), (65535, 2), (65536, 4), ((1 << 32) - 1, 4)):
        assert P([0, top]).width == width, top
    for n_colors, width in ((1, 1), (8, 1), (9, 2), (16, 2), (17, 4), (32, 4), (33, 8), (64, 8)):
        assert P([1 << (n_colors - 1)], "colors", n_colors).width == width, n_colors
    const = P([9] * 100)
    assert const.info() == {"layout": "runs", "width": 1, "windows": 100, "runs": 1, "device_bytes": 12}
    alt = P([1, 2] * 50)
    assert alt.info() == {"layout": "dense", "width": 1, "windows": 100, "runs": 100, "device_bytes": 100}
    assert P([70000] * 3 + [1] * 3 + [2] * 6).info() == {"layout": "runs", "width": 4, "windows": 12, "runs": 3, "device_bytes": 36}
    assert P([70000, 1, 1]).layout == "dense"  # 2 runs * 12 B = 24 > 3 windows * 4 B
    tie = P([70000] * 3 + [1] * 3)  # 2 runs * 12 B == 6 windows * 4 B: the tie goes to dense
    assert (tie.runs_bytes, tie.dense_bytes, tie.layout, tie.device_bytes) == (24, 24, "dense", 24)
    tie = P([1] * 2 + [0] * 2, "colors", 64)  # 2 runs * 16 B == 4 windows * 8 B
    assert (tie.runs_bytes, tie.dense_bytes, tie.layout) == (32, 32, "dense")
    empty = P([])
    assert empty.info() == {"layout": "dense", "width": 1, "windows": 0, "runs": 0, "device_bytes": 0}
    for layout in ("dense", "runs"):
        p = P([4, 4, 9, 9, 9, 1], layout=layout)
        assert [p.at(i) for i in range(6)] == [4, 4, 9, 9, 9, 1] and p.layout == layout
    assert TP.window_offsets([0, 5, 5, 7, 12], 3) == [0, 3, 3, 3, 6]
    assert [TP.ordinal([0, 5, 5, 7, 12], 3, t) for t in (0, 2, 7, 9)] == [0, 2, 3, 5]  # a run may cross the border between 2 and 3


@pytest.mark.parametrize("k", GPU_KS)
def test_the_gpu_tests_generator_shows_every_hazard(k):
    """The pairs test_gpu_tig_payload.py draws (same seeds) complete its `seen` dictionary at every k, heavy and light paths included."""
    rng = random.Random(3140 + k)
    seen = dict.fromkeys(TP.SEEN + ("heavy", "light"), False)
    for i in range(GPU_PAIRS):
        index, query, weights, masks, n_colors = TP.payload_pair(rng, k)
        assert len(weights) == len(masks) == len(KA.windows(index, k)) and all(x >> n_colors == 0 for x in masks)
        for f, v in TP.seen_flags(index, weights, query, k).items():
            seen[f] |= v
        if i < 2:  # (the paths: two pairs say enough)
            for m in cases.random_ms(k):
                for limit in (64, 1, 2):
                    ref = T.TigIndexRef([s.upper() for s in index], k, m, limit)
                    seen["heavy"] |= ref.heavy_windows > 0
                    seen["light"] |= ref.heavy_windows < ref.occurrences
    assert all(seen.values()), (k, seen)


def test_the_generators_cases_agree_with_the_arbiters():
    rng = random.Random(3140 + 5)
    for i in range(3):
        index, query, weights, masks, n_colors = TP.payload_pair(rng, 5)
        for limit in (64, 1):
            _agree(index, query, 5, None, limit, weights, masks, n_colors, ("generator", i, limit))


def test_entry_points_declared_and_exported(product_lib):
    names = _lib.declared_symbols()
    for n in ENTRY_POINTS:
        assert n in names and hasattr(product_lib, n), n
        assert getattr(product_lib, n).argtypes is not None, n
    assert product_lib.mtg_tig_index_is_weighted.restype is C.c_int and product_lib.mtg_tig_index_is_colored.restype is C.c_int
    assert product_lib.mtg_tig_index_build_annotated.restype is C.c_void_p
    assert len(product_lib.mtg_tig_index_build_annotated.argtypes) == 13 and len(product_lib.mtg_tig_index_build_annotated_store.argtypes) == 11
    assert len(product_lib.mtg_tig_index_abundance.argtypes) == len(product_lib.mtg_kmer_index_abundance.argtypes) == 11
    assert len(product_lib.mtg_tig_index_colors.argtypes) == len(product_lib.mtg_kmer_index_colors.argtypes) == 9
    assert C.sizeof(_lib.MtgTigIndexInfo) == 8 * 12  # (unchanged: the payloads show in device_bytes and in mtg_tig_payload_info)
    assert C.sizeof(_lib.MtgTigPayload) == 8 * 5 and C.sizeof(_lib.MtgTigPayloadInfo) == 8 * 12


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "mtg_engine.h"\n#include "matchtigs.h"\n'
                   "int main(void) {\n    uint64_t off[1] = {0}, kmers[1], valid[1], found[1], sum[1], masks[1] = {0}, pw64[1];\n"
                   "    uint32_t lo[1], hi[1], weights[1] = {0}, per_color[1], pw32[1];\n    double t[12];\n"
                   "    mtg_tig_index_info i;\n    mtg_tig_payload_info p;\n"
                   "    mtg_tig_index *ix = mtg_tig_index_build_annotated(\"\", off, 0, 31, 0, 0, weights, 0, masks, 0, 3, 0, 0);\n"
                   "    mtg_tig_index *iy = mtg_tig_index_build_annotated_store((const mtg_unitigs *)0, 31, 0, 0, weights, 0, masks, 0, 3, 2, 0);\n"
                   "    int l = mtg_tig_index_is_weighted(ix) + mtg_tig_index_is_colored(ix) + mtg_tig_index_is_locating(ix);\n"
                   "    mtg_tig_index_abundance(ix, \"\", off, 0, kmers, valid, found, sum, lo, hi, pw32);\n"
                   "    mtg_tig_index_colors(ix, \"\", off, 0, kmers, valid, found, per_color, pw64);\n"
                   "    mtg_last_tig_payload_times(t);\n    mtg_tig_index_get_payload_info(ix, &p);\n"
                   "    l += (int)(p.weights.layout + p.weights.width + p.weights.windows + p.weights.runs + p.weights.device_bytes + p.colors.layout"
                   " + p.n_colors + p.win_offset_bytes);\n"
                   "    mtg_tig_index_get_info(ix, &i);\n    mtg_tig_index_free(ix);\n    mtg_tig_index_free(iy);\n"
                   "    return l + (int)sizeof(i);\n}\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", str(ROOT / "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


_SEQ = "off = (C.c_uint64 * 2)(0, 5); w = (C.c_uint32 * 3)(1, 2, 3); c = (C.c_uint64 * 3)(1, 2, 4); "
_BUILD = "L.mtg_tig_index_build_annotated(b'ACGTA', off, 1, 3, 0, 0, "
DEATHS = [
    ("L.mtg_tig_index_build_annotated_store(None, 31, 0, 0, None, 0, None, 0, 0, 0, 0)", "mtg_tig_index_build_annotated_store: null argument"),
    ("L.mtg_tig_index_build_annotated(None, None, 1, 31, 0, 0, None, 0, None, 0, 0, 0, 0)", "mtg_tig_index_build_annotated: null argument"),
    (_SEQ + _BUILD + "None, 3, None, 0, 0, 0, 0)", "mtg_tig_index_build_annotated: 3 weights but no array"),
    (_SEQ + _BUILD + "None, 0, None, 3, 3, 0, 0)", "mtg_tig_index_build_annotated: 3 colour words but no array"),
    (_SEQ + _BUILD + "w, 2, None, 0, 0, 0, 0)", "mtg_tig_index_build_annotated: 2 weights for 3 windows"),
    (_SEQ + _BUILD + "None, 0, c, 2, 3, 0, 0)", "mtg_tig_index_build_annotated: 2 colour words for 3 windows"),
    (_SEQ + _BUILD + "None, 0, c, 3, 0, 0, 0)", "mtg_tig_index_build_annotated: 0 colours; 1 .. 64 are served"),
    (_SEQ + _BUILD + "None, 0, c, 3, 65, 0, 0)", "mtg_tig_index_build_annotated: 65 colours; 1 .. 64 are served"),
    (_SEQ + _BUILD + "None, 0, c, 3, 2, 0, 0)", "mtg_tig_index_build_annotated: the mask of window 2 has a bit at or beyond n_colors = 2"),
    (_SEQ + _BUILD + "w, 3, None, 0, 0, 3, 0)", "mtg_tig_index_build_annotated: layout 3"),
    (_SEQ + _BUILD + "w, 3, None, 0, 0, -1, 0)", "mtg_tig_index_build_annotated: layout -1"),
    (_SEQ + "L.mtg_tig_index_build_annotated(b'ACGTA', off, 1, 3, 4, 0, w, 3, None, 0, 0, 0, 0)", "mtg_tig_index_build_annotated: the minimizer length 4"),
    (_SEQ + "L.mtg_tig_index_build_annotated(b'ACGTA', off, 1, 0, 0, 0, w, 3, None, 0, 0, 0, 0)", "mtg_tig_index_build_annotated: k must be >= 1"),
    ("off = (C.c_uint64 * 2)(1, 5); L.mtg_tig_index_build_annotated(b'ACGTA', off, 1, 3, 0, 0, None, 0, None, 0, 0, 0, 0)",
     "mtg_tig_index_build_annotated: offsets must start at 0"),
    ("L.mtg_tig_index_abundance(None, None, None, 0, None, None, None, None, None, None, None)", "mtg_tig_index_abundance: null argument"),
    ("L.mtg_tig_index_colors(None, None, None, 0, None, None, None, None, None)", "mtg_tig_index_colors: null argument"),
    ("L.mtg_tig_index_is_weighted(None)", "mtg_tig_index_is_weighted: null argument"),
    ("L.mtg_tig_index_is_colored(None)", "mtg_tig_index_is_colored: null argument"),
    ("L.mtg_tig_index_get_payload_info(None, None)", "mtg_tig_index_get_payload_info: null argument"),
]


@pytest.mark.parametrize("i", range(len(DEATHS)))
def test_argument_checks_die_with_the_functions_name(product_lib, i):
    """Each is refused on the host, before a device is asked for: the child aborts with the entry point's name in the message."""
    code, message = DEATHS[i]
    r = subprocess.run([sys.executable, "-c", f"import ctypes as C\nfrom matchtigs_amd import _lib\nL = _lib.load()\n{code}\n"],
                       capture_output=True, text=True, cwd=str(ROOT), timeout=120)
    assert r.returncode != 0 and message in r.stderr, (code, r.returncode, r.stderr[-500:])


def _shell(weighted, colored, handle):
    ix = api.TigIndex.__new__(api.TigIndex)

    def asked(*a):
        raise AssertionError("the library was asked")

    ix._L = types.SimpleNamespace(mtg_tig_index_free=lambda h: None, mtg_tig_index_abundance=asked, mtg_tig_index_colors=asked)
    ix._h, ix.locating, ix.weighted, ix.colored, ix.n_colors = handle, True, weighted, colored, 2 if colored else 0
    return ix


def test_calls_refuse_a_missing_payload_and_a_closed_index():
    with pytest.raises(ValueError) as e:
        _shell(False, True, 1).abundance(["ACGT"])
    assert str(e.value) == "abundance() needs an index built with weights"
    with pytest.raises(ValueError) as e:
        _shell(True, False, 1).color_hits(["ACGT"])
    assert str(e.value) == "color_hits() needs an index built with colors"
    for call in ("abundance", "color_hits"):
        with pytest.raises(ValueError) as e:
            getattr(_shell(True, True, None), call)(["ACGT"])
        assert str(e.value) == "the index is closed"
    assert callable(api.last_tig_payload_times)


def test_the_constructors_value_errors_come_before_the_library(monkeypatch):
    """KmerIndex's checks, word for word, and none of them loads the library."""
    def asked():
        raise AssertionError("the library was asked")

    monkeypatch.setattr(_lib, "load", asked)
    seqs, k = ["ACGTACG", "AC", "GGGGG"], 3  # 5 + 0 + 3 windows
    make = api.TigIndex.annotated
    for kw, part in (({"weights": [1] * 7}, "weights must hold one entry per window: (7,) for 8 windows"),
                     ({"weights": [[1] * 4] * 2}, "weights must hold one entry per window"),
                     ({"colors": [1] * 9, "n_colors": 2}, "colors must hold one entry per window: (9,) for 8 windows"),
                     ({"colors": [1] * 8}, "n_colors must be in 1..64, not None"),
                     ({"colors": [1] * 8, "n_colors": 0}, "n_colors must be in 1..64, not 0"),
                     ({"colors": [1] * 8, "n_colors": 65}, "n_colors must be in 1..64, not 65"),
                     ({"colors": [1] * 8, "n_colors": True}, "n_colors must be in 1..64, not True"),
                     ({"colors": [1] * 7 + [4], "n_colors": 2}, "a mask has a colour beyond the 2 given"),
                     ({"n_colors": 2}, "n_colors needs colors"),
                     ({"weights": [1] * 8, "payload_layout": "sparse"}, "payload_layout must be None, 'dense' or 'runs'"),
                     ({"payload_layout": "runs"}, "payload_layout needs weights or colors"),
                     ({"weights": [1] * 8, "m": 4}, "m must be in 1..min(k, 31)"),
                     ({"weights": [1] * 8, "bucket_limit": 0}, "bucket_limit must be in 1..65536")):
        with pytest.raises(ValueError) as e:
            make(seqs, k, **kw)
        assert part in str(e.value), (kw, str(e.value))
    params = list(inspect.signature(make).parameters)
    assert params == ["seqs_or_store", "k", "m", "device_id", "bucket_limit", "weights", "colors", "n_colors", "payload_layout"]


def _cli(*a):
    return subprocess.run([sys.executable, "-m", "matchtigs_amd", *a], capture_output=True, text=True, cwd=str(ROOT), timeout=300)


AB, PR, CO = "--query-index-abundance-out", "--query-index-abundance-profile-out", "--query-index-colors-out"
Q = ("--query-fa", "q.fa", "--query-out", "r.tsv")
SPARSE = ("--query-index", "minimizer")
REFUSED = [
    (("--fa-in", "x.fa", AB, "a.tsv", *Q, *SPARSE), [AB, "--seq-in"]),
    (("--fa-in", "x.fa", CO, "c.tsv", *Q, *SPARSE), [CO, "--seq-in"]),
    (("--seq-in", "x.fa", AB, "a.tsv", *SPARSE), [AB, "--query-fa"]),
    (("--seq-in", "x.fa", CO, "c.tsv", *SPARSE), [CO, "--query-fa"]),
    (("--seq-in", "x.fa", AB, "a.tsv", "--query-fa", "q.fa", *SPARSE), [AB, "--query-out"]),
    (("--seq-in", "x.fa", CO, "c.tsv", "--query-fa", "q.fa", *SPARSE), [CO, "--query-out"]),
    (("--seq-in", "x.fa", AB, "a.tsv", *Q), [AB, "--query-index minimizer"]),
    (("--seq-in", "x.fa", CO, "c.tsv", *Q), [CO, "--query-index minimizer"]),
    (("--seq-in", "x.fa", AB, "a.tsv", *Q, "--query-index", "table"), [AB, "--query-index minimizer"]),
    (("--seq-in", "x.fa", CO, "c.tsv", *Q, "--query-index", "table"), [CO, "--query-index minimizer"]),
    (("--seq-in", "x.fa", PR, "p.txt", *Q, *SPARSE), [PR, AB]),
    (("--seq-in", "x.fa", AB, "a.tsv", *Q, *SPARSE, "--query-abundance-out", "b.tsv"), ["--query-abundance-out", "--query-index minimizer"]),
    (("--seq-in", "x.fa", CO, "c.tsv", *Q, *SPARSE, "--query-colors-out", "d.tsv"), ["--query-colors-out", "--query-index minimizer"]),
    (("--seq-in", "x.fa", CO, "c.tsv", *Q, *SPARSE, "--min-component-kmers", "5"), ["--min-component-kmers", CO]),
]


@pytest.mark.parametrize("i", range(len(REFUSED)))
def test_flag_rules(i):
    given, parts = REFUSED[i]
    r = _cli("-k", "21", *given)
    assert r.returncode == 2 and "error:" in r.stderr, (given, r.stderr[-500:])
    last = r.stderr.strip().splitlines()[-1]
    for part in parts:
        assert part in last, (given, last)


def test_accepted_flags_get_as_far_as_the_input(tmp_path):
    t = lambda name: str(tmp_path / name)
    query = ("--query-fa", "q.fa", "--query-out", t("r.tsv"), *SPARSE)
    for extra in ((AB, t("a.tsv")), (CO, t("c.tsv.gz")), (AB, t("a.tsv.gz"), PR, t("p.txt"), CO, t("c.tsv"), "--query-index-over", "input"),
                  (AB, t("a.tsv"), PR, t("p.txt.gz"), "--query-index-over", "greedytigs", "--greedytigs-fa-out", t("g.fa")),
                  (CO, t("c.tsv"), AB, t("a.tsv"), "--query-index-over", "eulertigs", "--eulertigs-fa-out", t("e.fa"), "--query-minimizer-length", "11"),
                  (AB, t("a.tsv"), CO, t("c.tsv"), "--query-index-locate-out", t("l.tsv"), "--query-presence-out", t("p.txt"))):
        r = _cli("--seq-in", t("no_such.fa"), "-k", "21", *query, *extra)
        assert r.returncode != 0 and "error:" not in r.stderr and "cannot open" in r.stderr, (extra, r.stderr[-1000:])
    out = _cli("--help").stdout
    for flag in (AB, PR, CO):
        assert flag in out
