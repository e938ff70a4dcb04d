"""Pseudoalignment with equivalence classes, without a GPU: the worked example by hand, the restatement's rule against
a brute-force set intersection and against kmer_color_ref.py's counters, the C ABI's declarations, the header as C99, the library's
host-side refusals, the command line's flag rules and threshold parsing, and the Python wrapper's errors."""
import ctypes as C
import random
import subprocess
import sys
import types
from pathlib import Path

import pytest

import kmer_color_ref as KC
import pseudoalign_ref as PA
from matchtigs_amd import __main__ as cli
from matchtigs_amd import _lib, api, synth

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = ("mtg_pseudoaligner_create", "mtg_pseudoaligner_create_tig", "mtg_pseudoaligner_align", "mtg_pseudoaligner_align_store",
                "mtg_pseudoaligner_classes", "mtg_pseudoaligner_totals", "mtg_pseudoaligner_reset", "mtg_pseudoaligner_free",
                "mtg_last_pseudoalign_times")


def _dna(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def test_worked_example_row_by_row():
    k, index, colors = PA.EXAMPLE_K, PA.EXAMPLE_INDEX, PA.example_colors()
    masks = PA.class_masks(index, colors, k)
    assert masks[synth.canonical("CATG")] == 0b101 and masks[synth.canonical("ACGT")] == 0b011 and masks["AAAA"] == 0b100
    for read, mate, kmers, valid, found, hits, strict, half in PA.EXAMPLE_ROWS:
        records = [read] if mate is None else [read, mate]
        assert PA.fragment(masks, k, records, 3) == (kmers, valid, found, hits), read
        assert PA.assign(valid, found, hits, 1000, "found") == strict, read
        assert PA.assign(valid, found, hits, 500, "found") == half, read
        assert PA.intersection(masks, k, records) == strict, read
    # the pair at P = 600: 4000 >= 3600 over found, 4000 < 4200 over valid
    assert PA.assign(7, 6, [4, 0, 4], 600, "found") == 0b101 and PA.assign(7, 6, [4, 0, 4], 600, "valid") == 0
    # neither mate alone gives the pair's answer at P = 500: the first has colours 0 and 2 at 4/4 and 2/4 ...
    a = PA.Aligner(index, colors, 3, k, 500)
    r = a.align([row[0] for row in PA.EXAMPLE_ROWS], None)
    assert r["masks"] == [0b011, 0b101, 0b011, 0b011, 0, 0b101, 0]
    assert a.classes() == {"mask": [0b011, 0b101], "carriers": [2, 2], "fragments": [3, 2], "first": [0, 1]}
    assert a.totals == {"fragments": 7, "eligible": 5, "assigned": 5, "ambiguous": 5}
    assert a.color_reads() == ([5, 3, 2], [0, 0, 0])
    strict = PA.Aligner(index, colors, 3, k)
    reads = [row[0] for row in PA.EXAMPLE_ROWS]
    mates = [row[1] or "" for row in PA.EXAMPLE_ROWS]
    assert strict.align(reads, mates)["masks"] == [row[6] for row in PA.EXAMPLE_ROWS]
    assert strict.classes() == {"mask": [0b011, 0b001, 0b010], "carriers": [2, 1, 1], "fragments": [1, 1, 1], "first": [0, 2, 3]}
    assert strict.color_reads() == ([2, 2, 0], [1, 1, 0])
    strict.align(reads[:1])  # ordinals run across calls
    assert strict.classes()["fragments"] == [2, 1, 1] and strict.totals["fragments"] == 8
    strict.reset()
    assert strict.classes()["mask"] == [] and strict.totals["fragments"] == 0


def _random_colouring(rng, k):
    C_ = rng.choice([1, 2, 3, 5, 64])
    index = [_dna(rng, rng.randint(0, 3 * k + 8), "ACGT" if k > 3 else "AC") for _ in range(rng.randint(1, 5))]
    windows = sum(max(0, len(s) - k + 1) for s in index)
    colors = [rng.choice([0, 1, (1 << C_) - 1, rng.getrandbits(C_), rng.getrandbits(C_)]) for _ in range(windows)]
    pool = "".join(index) + synth.revcomp("".join(index))
    reads = []
    for _ in range(6):
        at = rng.randrange(max(1, len(pool)))
        s = list(pool[at:at + rng.randint(0, 2 * k + 6)])
        for _ in range(rng.randint(0, 2)):
            if s:
                s[rng.randrange(len(s))] = rng.choice("NnACGTacgt")
        reads.append("".join(s))
    return C_, index, colors, reads


@pytest.mark.parametrize("k", [1, 2, 3, 5, 8])
def test_the_rule_against_the_set_intersection_and_the_counters(k):
    rng = random.Random(3300 + k)
    seen = {"assigned": False, "unassigned with hits": False, "mask 0 found": False, "pair differs": False}
    for i in range(25):
        C_, index, colors, reads = _random_colouring(rng, k)
        masks = PA.class_masks(index, colors, k)
        mates = reads[3:] + reads[:3]
        counters = KC.color_hits(index, colors, C_, reads, k)  # the one cross-check of the two restatements
        for P in (1, 500, 600, 999, 1000):
            for over in ("found", "valid"):
                for min_kmers in (1, 5):
                    a = PA.Aligner(index, colors, C_, k, P, over, min_kmers)
                    single, paired = a.align(reads), a.align(reads, mates)
                    assert single["hits"] == counters["per_color"] and single["found"] == counters["found"]
                    for r, s in enumerate(reads):
                        for got, records in ((single, [s]), (paired, [s, mates[r]])):
                            m, denom = got["masks"][r], got[over][r]
                            assert m >> C_ == 0
                            if P == 1000:
                                want = PA.intersection(masks, k, records, over) if denom >= min_kmers else 0
                                assert m == want, (k, i, over, min_kmers, records)
                            if P == 1:  # every colour that has a hit at all
                                assert m == (sum(1 << c for c in range(C_) if got["hits"][r][c]) if denom >= min_kmers else 0)
                            seen["assigned"] |= m != 0
                            seen["unassigned with hits"] |= m == 0 and any(got["hits"][r])
                            seen["mask 0 found"] |= got["found"][r] > 0 and not any(got["hits"][r])
                        seen["pair differs"] |= paired["masks"][r] not in (single["masks"][r], single["masks"][(r + 3) % 6])
                    cl = a.classes()
                    assert sum(cl["fragments"]) == a.totals["assigned"] and cl["first"] == sorted(cl["first"]) and 0 not in cl["mask"]
                    assert a.totals["fragments"] == 12 and a.totals["ambiguous"] <= a.totals["assigned"] <= a.totals["eligible"] <= 12
    assert all(seen.values()), (k, seen)


def test_entry_points_declared_and_exported(product_lib):
    names = _lib.declared_symbols()
    for n in ENTRY_POINTS:
        assert n in names and hasattr(product_lib, n), n
        assert getattr(product_lib, n).argtypes is not None, n
    nm = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "matchtigs_amd" / "libmatchtigs.so")], capture_output=True, text=True)
    exported = {line.split()[-1] for line in nm.stdout.splitlines() if line.strip()}
    assert nm.returncode == 0 and set(ENTRY_POINTS) <= exported  # unmangled
    L = product_lib
    assert L.mtg_pseudoaligner_create.restype is C.c_void_p and L.mtg_pseudoaligner_create_tig.restype is C.c_void_p
    assert L.mtg_pseudoaligner_classes.restype is C.c_uint64 and len(L.mtg_pseudoaligner_align.argtypes) == 10
    assert len(L.mtg_pseudoaligner_align_store.argtypes) == 7 and len(L.mtg_pseudoaligner_classes.argtypes) == 4


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "mtg_engine.h"\n#include "matchtigs.h"\n'
                   "int main(void) {\n    uint64_t off[1] = {0}, kmers[1], valid[1], found[1], masks[1], totals[4], *m, *f, *first, n;\n"
                   "    double t[6];\n    mtg_pseudoalign_params p = {1000, 0, 1};\n"
                   "    mtg_pseudoaligner *a = mtg_pseudoaligner_create((const mtg_kmer_index *)0, &p);\n"
                   "    mtg_pseudoaligner *b = mtg_pseudoaligner_create_tig((const mtg_tig_index *)0, (const mtg_pseudoalign_params *)0);\n"
                   "    mtg_pseudoaligner_align(a, \"\", off, 0, (const char *)0, (const uint64_t *)0, kmers, valid, found, masks);\n"
                   "    mtg_pseudoaligner_align_store(b, (const mtg_unitigs *)0, (const mtg_unitigs *)0, kmers, valid, found, masks);\n"
                   "    n = mtg_pseudoaligner_classes(a, &m, &f, &first);\n    mtg_pseudoaligner_totals(a, totals);\n"
                   "    mtg_pseudoaligner_reset(a);\n    mtg_last_pseudoalign_times(t);\n    mtg_free(m);\n"
                   "    mtg_pseudoaligner_free(a);\n    mtg_pseudoaligner_free(b);\n    mtg_pseudoaligner_free((mtg_pseudoaligner *)0);\n"
                   "    return (int)n + (int)sizeof(p);\n}\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", str(ROOT / "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


DEATHS = [
    ("L.mtg_pseudoaligner_create(None, None)", "mtg_pseudoaligner_create: null argument"),
    ("L.mtg_pseudoaligner_create_tig(None, None)", "mtg_pseudoaligner_create_tig: null argument"),
    ("L.mtg_pseudoaligner_align(None, None, None, 0, None, None, None, None, None, None)", "mtg_pseudoaligner_align: null argument"),
    ("L.mtg_pseudoaligner_align_store(None, None, None, None, None, None, None)", "mtg_pseudoaligner_align_store: null argument"),
    ("L.mtg_pseudoaligner_classes(None, None, None, None)", "mtg_pseudoaligner_classes: null argument"),
    ("L.mtg_pseudoaligner_totals(None, None)", "mtg_pseudoaligner_totals: null argument"),
    ("L.mtg_pseudoaligner_reset(None)", "mtg_pseudoaligner_reset: null argument"),
]


@pytest.mark.parametrize("i", range(len(DEATHS)))
def test_argument_checks_die_with_the_functions_name(product_lib, i):
    code, message = DEATHS[i]
    r = subprocess.run([sys.executable, "-c", f"import ctypes as C\nfrom matchtigs_amd import _lib\nL = _lib.load()\n{code}\n"],
                       capture_output=True, text=True, cwd=str(ROOT), timeout=120)
    assert r.returncode != 0 and message in r.stderr, (code, r.returncode, r.stderr[-500:])


def test_free_accepts_null_and_the_refusals_name_their_function(product_lib):
    product_lib.mtg_pseudoaligner_free(None)
    out = (C.c_double * 6)()
    product_lib.mtg_last_pseudoalign_times(out)
    assert list(out) == [0.0] * 6  # (no call on this thread yet)
    # the refusals that need an index are made on the host before a device is asked; without a GPU no index exists, so their text
    # is checked in the source
    source = (ROOT / "matchtigs_amd" / "csrc" / "engine_api.cpp").read_text()
    body = source[source.index("static mtg_pseudoaligner *pseudoaligner_new"):source.index("void mtg_pseudoaligner_align_store")]
    for part in ("the index keeps no colours", "is outside 1 .. 1000", "min_kmers must be >= 1", "mate_seq and mate_off go together",
                 '"mtg_pseudoaligner_create"', '"mtg_pseudoaligner_create_tig"', "if (n == 0) return;"):
        assert part in body, part


# ---- the command line ----
def _cli(*a):
    return subprocess.run([sys.executable, "-m", "matchtigs_amd", *a], capture_output=True, text=True, cwd=str(ROOT), timeout=300)


PF, PO = "--pseudoalign-fa", "--pseudoalign-out"
SEQ = ("--seq-in", "a.fa", "--seq-in", "b.fa")
REFUSED = [
    ((*SEQ, "--pseudoalign-mate-fa", "m.fa"), ["--pseudoalign-mate-fa", PF]),
    ((*SEQ, PO, "o.tsv"), [PO, PF]),
    ((*SEQ, "--pseudoalign-classes-out", "o.tsv"), ["--pseudoalign-classes-out", PF]),
    ((*SEQ, "--pseudoalign-summary-out", "o.tsv"), ["--pseudoalign-summary-out", PF]),
    ((*SEQ, "--unitigs-fa-out", "u.fa", "--pseudoalign-threshold", "0.5"), ["--pseudoalign-threshold", PF]),
    ((*SEQ, "--unitigs-fa-out", "u.fa", "--pseudoalign-over", "valid"), ["--pseudoalign-over", PF]),
    ((*SEQ, "--unitigs-fa-out", "u.fa", "--pseudoalign-min-kmers", "3"), ["--pseudoalign-min-kmers", PF]),
    ((*SEQ, "--unitigs-fa-out", "u.fa", "--pseudoalign-min-base-quality", "3"), ["--pseudoalign-min-base-quality", PF]),
    ((*SEQ, "--unitigs-fa-out", "u.fa", "--pseudoalign-index", "minimizer"), ["--pseudoalign-index", PF]),
    ((*SEQ, "--unitigs-fa-out", "u.fa", "--pseudoalign-minimizer-length", "5"), ["--pseudoalign-minimizer-length", PF]),
    (("--fa-in", "x.fa", PF, "r.fa", PO, "o.tsv"), [PF, "--seq-in"]),
    (("--bcalm-in", "x.fa", PF, "r.fa", PO, "o.tsv"), [PF, "--seq-in"]),
    ((*SEQ, PF, "r.fa"), [PF, PO, "--pseudoalign-classes-out", "--pseudoalign-summary-out"]),
    ((*SEQ, PF, "r.fa", PF, "s.fa", PO, "o.tsv", "--pseudoalign-mate-fa", "m.fa"), ["--pseudoalign-mate-fa", PF, "1", "2"]),
    ((*SEQ, PF, "r.fa", PO, "o.tsv", "--pseudoalign-min-kmers", "0"), ["--pseudoalign-min-kmers", ">= 1"]),
    ((*SEQ, PF, "r.fa", PO, "o.tsv", "--pseudoalign-minimizer-length", "5"), ["--pseudoalign-minimizer-length", "--pseudoalign-index minimizer"]),
    ((*SEQ, PF, "r.fa", PO, "o.tsv", "--pseudoalign-index", "minimizer", "--pseudoalign-minimizer-length", "22"),
     ["--pseudoalign-minimizer-length", "1..21"]),
    ((*SEQ, PF, "r.fa", PO, "o.tsv", "--pseudoalign-min-base-quality", "94"), ["--pseudoalign-min-base-quality", "0..93"]),
    ((*SEQ, PF, "r.fa", PO, "o.tsv", "--min-component-kmers", "3"), ["--min-component-kmers", PF]),
] + [((*SEQ, PF, "r.fa", PO, "o.tsv", "--pseudoalign-threshold", t), ["--pseudoalign-threshold", "(0, 1]", repr(t)])
     for t in ("0", "1.0001", "0.8005", "abc", "-0.5", "nan", "2")]


@pytest.mark.parametrize("i", range(len(REFUSED)))
def test_flag_rules(i):
    given, parts = REFUSED[i]
    r = _cli("-k", "21", *given)
    assert r.returncode == 2 and "error:" in r.stderr, (given, r.stderr[-500:])
    last = r.stderr.strip().splitlines()[-1]
    for part in parts:
        assert part in last, (given, last)


def test_threshold_parsing():
    assert [cli._permille(t) for t in ("0.8", "1", "0.001", "1.000", "0.25", ".5", "1e-3", "8E-1")] == [800, 1000, 1, 1000, 250, 500, 1, 800]
    assert [cli._permille(t) for t in ("0", "1.0001", "0.8005", "abc", "", "-1", "inf", "nan", "0.0001", "1.001")] == [None] * 10
    assert all(cli._permille(f"0.{n:03d}") == n for n in range(1, 1000))  # every thousandth, exactly
    import inspect

    source = inspect.getsource(cli._permille)
    assert "decimal.Decimal(" in source and "float(" not in source  # never through a float


def test_accepted_flags_get_as_far_as_the_input(tmp_path):
    t = lambda name: str(tmp_path / name)
    for extra in ((PO, t("o.tsv")), ("--pseudoalign-classes-out", t("c.tsv")), ("--pseudoalign-summary-out", t("s.tsv"), "--pseudoalign-threshold", "0.8"),
                  (PO, t("o.tsv"), "--pseudoalign-over", "valid", "--pseudoalign-min-kmers", "3", "--pseudoalign-index", "table"),
                  (PO, t("o.tsv"), "--pseudoalign-index", "minimizer", "--pseudoalign-minimizer-length", "11", "--pseudoalign-mate-fa", t("m.fa"))):
        r = _cli("--seq-in", t("no_such_a.fa"), "--seq-in", t("no_such_b.fa"), "-k", "21", PF, t("r.fa"), *extra)
        assert r.returncode != 0 and "error:" not in r.stderr and "cannot open" in r.stderr, (extra, r.stderr[-1000:])
    out = _cli("--help").stdout
    for flag in (PF, "--pseudoalign-mate-fa", PO, "--pseudoalign-classes-out", "--pseudoalign-summary-out", "--pseudoalign-threshold",
                 "--pseudoalign-over", "--pseudoalign-min-kmers", "--pseudoalign-min-base-quality", "--pseudoalign-index",
                 "--pseudoalign-minimizer-length"):
        assert flag in out


def test_a_mate_file_with_another_record_count_ends_the_run_with_2(tmp_path, monkeypatch, capsys):
    """_pseudoalign itself, with the library stubbed out: both files and both counts are named, nothing is aligned."""
    reads, mates = str(tmp_path / "r.fa"), str(tmp_path / "m.fa")

    class Stub(types.SimpleNamespace):
        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return None

    def _asked(*a, **kw):
        raise AssertionError("the reads were aligned")

    info = types.SimpleNamespace(characters=0, records=0, device_bytes=0, occurrences=0)
    stub_api = types.SimpleNamespace(
        KmerIndex=lambda *a, **kw: Stub(info=info),
        Pseudoaligner=lambda *a, **kw: Stub(over="found", min_kmers=1, align=_asked),
        read_sequences_named=lambda path: ((["ACGT"] * 3, ["a", "b", "c"]) if path == reads else (["ACGT"] * 2, ["a", "b"])))
    args = types.SimpleNamespace(pseudoalign_index=None, pseudoalign_minimizer_length=None, k=4, device=0, pseudoalign_permille=1000,
                                 pseudoalign_over=None, pseudoalign_min_kmers=None, pseudoalign_out=None, pseudoalign_classes_out=None,
                                 pseudoalign_summary_out=str(tmp_path / "s.tsv"), pseudoalign_fa=[reads], pseudoalign_mate_fa=[mates],
                                 pseudoalign_min_base_quality=None, seq_in=["a.fa", "b.fa"], compression_level=6)
    colors = types.SimpleNamespace(kmer_colors=[], n_colors=2)
    assert cli._pseudoalign(stub_api, args, None, colors) == 2
    err = capsys.readouterr().err.strip().splitlines()[-1]
    assert reads in err and mates in err and " 3 " in err and " 2" in err


# ---- the wrapper ----
def _asked(*a, **kw):
    raise AssertionError("the library was asked")


def _shell_index(cls, handle, colored=True):
    ix = cls.__new__(cls)
    ix._L = types.SimpleNamespace(mtg_kmer_index_free=lambda h: None, mtg_tig_index_free=lambda h: None, mtg_pseudoaligner_create=_asked,
                                  mtg_pseudoaligner_create_tig=_asked, mtg_pseudoaligner_align=_asked, mtg_pseudoaligner_classes=_asked,
                                  mtg_pseudoaligner_totals=_asked, mtg_pseudoaligner_reset=_asked, mtg_pseudoaligner_free=lambda h: None)
    ix._h, ix.locating, ix.weighted, ix.colored, ix.n_colors = handle, False, False, colored, 3 if colored else 0
    return ix


def _shell_aligner(index, handle):
    a = api.Pseudoaligner.__new__(api.Pseudoaligner)
    a.index, a._L, a._h, a.n_colors = index, index._L, handle, index.n_colors
    return a


@pytest.mark.parametrize("cls", [api.KmerIndex, api.TigIndex])
def test_the_wrappers_errors_come_before_the_library(monkeypatch, cls):
    monkeypatch.setattr(_lib, "load", _asked)
    with pytest.raises(TypeError):
        api.Pseudoaligner(["ACGT"])
    with pytest.raises(ValueError) as e:
        api.Pseudoaligner(_shell_index(cls, None))
    assert str(e.value) == "the index is closed"
    with pytest.raises(ValueError) as e:
        api.Pseudoaligner(_shell_index(cls, 1, colored=False))
    assert "built with colors" in str(e.value)
    for kw in ({"threshold_permille": 0}, {"threshold_permille": 1001}, {"threshold_permille": 0.8}, {"threshold_permille": True},
               {"over": "present"}, {"over": None}, {"min_kmers": 0}, {"min_kmers": -1}, {"min_kmers": 1.5}):
        with pytest.raises(ValueError) as e:
            api.Pseudoaligner(_shell_index(cls, 1), **kw)
        assert next(iter(kw)) in str(e.value) or "over" in str(e.value)
    calls = (lambda a: a.align(["ACGT"]), lambda a: a.align(["ACGT"], ["ACGT"]), lambda a: a.classes(), lambda a: a.totals,
             lambda a: a.color_reads, lambda a: a.reset())
    for call in calls:
        with pytest.raises(ValueError) as e:
            call(_shell_aligner(_shell_index(cls, 1), None))
        assert str(e.value) == "the aligner is closed"
        with pytest.raises(ValueError) as e:
            call(_shell_aligner(_shell_index(cls, None), 1))
        assert str(e.value) == "the index is closed"
    with pytest.raises(ValueError) as e:  # unequal record counts: before the library
        _shell_aligner(_shell_index(cls, 1), 1).align(["ACGT", "ACGT"], ["ACGT"])
    assert "2 reads and 1 mates" in str(e.value)
    a = _shell_aligner(_shell_index(cls, 1), 1)
    with a as same:
        assert same is a
    assert a._h is None
    a.close()  # (twice is fine)
    import matchtigs_amd

    assert matchtigs_amd.Pseudoaligner is api.Pseudoaligner and matchtigs_amd.last_pseudoalign_times is api.last_pseudoalign_times


def test_the_result_names_its_colours():
    import numpy as np

    r = api.PseudoalignResult(4, np.zeros(3, np.uint64), *(np.zeros(2, np.uint64) for _ in range(3)), np.array([0b101, 1 << 63], np.uint64))
    assert r.colors(0) == [0, 2] and r.colors(1) == [63]
    with pytest.raises(Exception):
        r.masks = None  # frozen
