"""Read correction, without a GPU: the worked example row by row, the restatement against a second, deliberately naive
one, the rule's invariants, the C ABI's declarations, the header as C99, the library's host-side refusals, the command line's flag
rules, the wrapper's errors, and the patching of FASTA / FASTQ text with the library stubbed out by the restatement."""
import ctypes as C
import gzip
import random
import subprocess
import sys
import types
from pathlib import Path

import numpy as np
import pytest

import kmer_correct_ref as CR
from matchtigs_amd import __main__ as cli
from matchtigs_amd import _lib, api, synth

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = ("mtg_kmer_index_correct", "mtg_kmer_index_correct_store", "mtg_last_kmer_correct_times")
GOOD = set("ACGTacgt")


def _dna(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def test_worked_example_row_by_row():
    k, solid = CR.EXAMPLE_K, CR.solid_set(CR.EXAMPLE_INDEX, CR.EXAMPLE_K)
    assert len(solid) == 13
    for read, valid, found, candidates, by_w in CR.EXAMPLE_ROWS:
        for W in (1, 2, 4):
            if W not in by_w:
                continue
            subs, found_after = by_w[W]
            r = CR.correct(solid, k, [read], W, 1)
            assert (r["kmers"], r["valid"], r["found"], r["candidates"]) == ([max(0, len(read) - k + 1)], [valid], [found], [candidates]), (read, W)
            assert [f"{p}:{a}>{b}" for p, a, b in r["substitutions"][0]] == subs and r["found_after"] == [found_after], (read, W)
            assert r["corrected"] == [len(subs)] and r["round_corrected"] == [len(subs)] + [0] * 7
    # all rows in one call: positions index the concatenated reads
    reads = [row[0] for row in CR.EXAMPLE_ROWS]
    r = CR.correct(solid, k, reads, 4, 1)
    starts = np.cumsum([0] + [len(s) for s in reads]).tolist()
    assert r["positions"] == [starts[1] + 4, starts[2] + 0, starts[3] + 6, starts[5] + 4] and r["bases"] == ["T", "A", "A", "T"]
    assert r["ambiguous"] == [0] * len(reads)
    # the other strand of the second row is corrected to the other strand of the first
    assert CR.correct(solid, k, [synth.revcomp("ACGTAGCATGG")], 4, 1)["texts"] == [synth.revcomp("ACGTTGCATGG")]


def _naive_round(both_strands, k, x, W):
    """One round, the slow way: every window of the record is looked at for every position, a window is a string in a set that
    holds both strands, and the best base comes out of a sorted list."""
    n = len(x)

    def solid(y, i):
        return set(y[i:i + k]) <= GOOD and y[i:i + k].upper() in both_strands

    candidates, ambiguous, subs = [], [], {}
    for p in range(n):
        cover = [i for i in range(n - k + 1) if i <= p < i + k and set(x[i:i + k]) <= GOOD]
        if not cover or any(solid(x, i) for i in cover):
            continue
        candidates.append(p)
        scores = sorted(((sum(solid(x[:p] + b + x[p + 1:], i) for i in cover), b) for b in "ACGT" if b != x[p].upper()), reverse=True)
        if scores[0][0] < min(W, len(cover)):
            continue
        if scores[0][0] == scores[1][0]:
            ambiguous.append(p)
        else:
            subs[p] = scores[0][1]
    return candidates, ambiguous, subs


def _random_case(rng, k):
    alphabet = "A" if k == 1 else "AC" if k <= 3 else "ACGT"
    index = [_dna(rng, rng.randint(0, 4 * k + 12), alphabet) for _ in range(rng.randint(1, 4))]
    pool = "".join(index) + synth.revcomp("".join(index)) + "ACGT"
    reads = []
    for _ in range(6):
        at = rng.randrange(len(pool))
        s = list(pool[at:at + rng.randint(0, 3 * k + 6)])
        for _ in range(rng.randint(0, 3)):
            if s:
                s[rng.randrange(len(s))] = rng.choice("NnACGTacgt")
        reads.append("".join(s))
    return index, reads


@pytest.mark.parametrize("k", [1, 2, 3, 5, 8])
def test_the_restatement_against_the_naive_one_and_the_invariants(k):
    rng = random.Random(3400 + k)
    seen = {"substituted": False, "ambiguous": False, "second round": False, "too few": False, "lower case": False, "twice": False,
            "not alone": False}
    for i in range(30):
        index, reads = _random_case(rng, k)
        solid = CR.solid_set(index, k)
        both = solid | {synth.revcomp(s) for s in solid}
        for W in (1, 2, 4, k + 1):
            for x in reads:
                got = CR.one_round(solid, k, x, W)
                assert got == _naive_round(both, k, x, W), (k, i, W, x)
                seen["ambiguous"] |= bool(got[1])
                seen["too few"] |= len(got[0]) > len(got[1]) + len(got[2])
            for R in (1, 2, 3, 8):
                r = CR.correct(solid, k, reads, W, R)
                seen["substituted"] |= bool(r["positions"])
                seen["second round"] |= r["round_corrected"][1] > 0
                assert sum(r["round_corrected"]) >= len(r["positions"]) == sum(r["corrected"]) and r["round_corrected"][R:] == [0] * (8 - R)
                seen["twice"] |= sum(r["round_corrected"]) > len(r["positions"])
                assert r["positions"] == sorted(set(r["positions"]))
                after = CR.correct(solid, k, r["texts"], W, 1)
                assert after["valid"] == r["valid"] and after["kmers"] == r["kmers"]  # valid is unchanged by correction
                assert after["found"] == r["found_after"]
                for x, y, subs, n in zip(reads, r["texts"], r["substitutions"], r["corrected"]):
                    differ = [p for p in range(len(x)) if x[p] != y[p]]
                    assert len(x) == len(y) and differ == [p for p, _, _ in subs] and n == len(differ)  # corrected = where apply differs
                    assert all(a == x[p] and b == y[p] and a.islower() == b.islower() and a.upper() != b.upper() for p, a, b in subs)
                    seen["lower case"] |= any(b.islower() for _, _, b in subs)
                    # a substituted position is never a candidate afterwards -- where no other substitution of its round lies within
                    # k - 1 of it (kmer_correct_ref's note); one round, so that the rounds are told apart
                    once = CR.one_round(solid, k, x, W)[2]
                    again = set(CR.one_round(solid, k, CR.patched(x, once), W)[0])
                    alone = {p for p in once if not any(q != p and abs(q - p) < k for q in once)}
                    assert not again & alone, (k, i, W, x)
                    seen["not alone"] |= bool(again & set(once))
                # R rounds are R single-round calls chained
                texts, total, per_round = reads, 0, []
                for _ in range(R):
                    step = CR.correct(solid, k, texts, W, 1)
                    texts, ambiguous = step["texts"], step["ambiguous"]
                    per_round.append(step["round_corrected"][0])
                    total += per_round[-1]
                assert texts == r["texts"] and ambiguous == r["ambiguous"] and total == sum(r["round_corrected"])
                assert per_round == r["round_corrected"][:R]
                # the wrapper's apply() on the restatement's substitutions
                off = np.cumsum([0] + [len(x) for x in reads]).astype(np.uint64)
                res = api.CorrectionResult(k, off, *(np.array(r[f], np.uint64) for f in (
                    "kmers", "valid", "found", "found_after", "candidates", "ambiguous", "corrected")), np.array(r["positions"], np.uint64),
                    np.frombuffer("".join(r["bases"]).encode(), np.uint8), np.array(r["round_corrected"], np.uint64))
                assert res.apply(reads) == r["texts"]
                assert [res.record_of(j) for j in range(len(res.positions))] == [q for q, subs in enumerate(r["substitutions"]) for _ in subs]
    assert seen["ambiguous"] or k >= 8, (k, seen)
    assert (seen["twice"] and seen["not alone"]) == (k in (3, 5)), (k, seen)  # (dense sets: the note's case happens, and is covered)
    if k >= 2:
        assert seen["substituted"] and seen["too few"], (k, seen)
    if k >= 5:
        assert seen["second round"] and seen["lower case"], (k, seen)


def test_the_result_is_frozen_and_apply_wants_the_same_records():
    z = np.zeros(1, np.uint64)
    r = api.CorrectionResult(4, np.array([0, 4], np.uint64), z, z, z, z, z, z, z, np.array([1], np.uint64), np.frombuffer(b"T", np.uint8),
                             np.zeros(8, np.uint64))
    assert r.apply(["AcGT"]) == ["AtGT"] and r.apply(["ACGT"]) == ["ATGT"] and r.record_of(0) == 0
    with pytest.raises(Exception):
        r.positions = None  # frozen
    with pytest.raises(ValueError):
        r.apply(["ACGTA"])
    with pytest.raises(ValueError):
        r.apply(["AC", "GT"])


def test_entry_points_declared_and_exported(product_lib):
    names = _lib.declared_symbols()
    for n in ENTRY_POINTS:
        assert n in names and hasattr(product_lib, n), n
        assert getattr(product_lib, n).argtypes is not None, n
    nm = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "matchtigs_amd" / "libmatchtigs.so")], capture_output=True, text=True)
    exported = {line.split()[-1] for line in nm.stdout.splitlines() if line.strip()}
    assert nm.returncode == 0 and set(ENTRY_POINTS) <= exported  # unmangled
    assert len(product_lib.mtg_kmer_index_correct.argtypes) == 16 and len(product_lib.mtg_kmer_index_correct_store.argtypes) == 14


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "mtg_engine.h"\n#include "matchtigs.h"\n'
                   "int main(void) {\n    uint64_t off[1] = {0}, a[1], b[1], c[1], d[1], e[1], f[1], g[1], *positions, n, rounds[8];\n"
                   "    uint8_t *bases;\n    double t[8];\n    mtg_correct_params p = {4, 2};\n"
                   "    mtg_kmer_index_correct((const mtg_kmer_index *)0, \"\", off, 0, &p, a, b, c, d, e, f, g, &positions, &bases, &n, rounds);\n"
                   "    mtg_kmer_index_correct_store((const mtg_kmer_index *)0, (const mtg_unitigs *)0, (const mtg_correct_params *)0, a, b, c, d, e, f, g,\n"
                   "                                 &positions, &bases, &n, rounds);\n"
                   "    mtg_last_kmer_correct_times(t);\n    mtg_free(positions);\n    mtg_free(bases);\n"
                   "    return (int)n + (int)sizeof(p) + (int)p.min_solid + (int)p.rounds;\n}\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", str(ROOT / "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


_OUTS = "None, None, None, None, None, None, None, C.byref(pos), C.byref(bases), C.byref(n), rounds"
_SETUP = "pos, bases, n, rounds = C.c_void_p(), C.c_void_p(), C.c_uint64(), (C.c_uint64 * 8)()\n"
DEATHS = [
    (f"L.mtg_kmer_index_correct(None, None, None, 0, None, {_OUTS})", "mtg_kmer_index_correct: null argument"),
    ("L.mtg_kmer_index_correct(None, None, None, 0, None, None, None, None, None, None, None, None, None, None, None, None)",
     "mtg_kmer_index_correct: null argument"),
    (f"L.mtg_kmer_index_correct_store(None, None, None, {_OUTS})", "mtg_kmer_index_correct_store: null argument"),
    (f"p = (C.c_uint32 * 2)(0, 2)\nL.mtg_kmer_index_correct(None, None, None, 0, C.cast(p, C.c_void_p), {_OUTS})",
     "mtg_kmer_index_correct: min_solid must be >= 1"),
    (f"p = (C.c_uint32 * 2)(4, 0)\nL.mtg_kmer_index_correct(None, None, None, 0, C.cast(p, C.c_void_p), {_OUTS})",
     "mtg_kmer_index_correct: rounds 0 is outside 1 .. 8"),
    (f"p = (C.c_uint32 * 2)(4, 9)\nL.mtg_kmer_index_correct(None, None, None, 0, C.cast(p, C.c_void_p), {_OUTS})",
     "mtg_kmer_index_correct: rounds 9 is outside 1 .. 8"),
]


@pytest.mark.parametrize("i", range(len(DEATHS)))
def test_argument_checks_die_with_the_functions_name(product_lib, i):
    code, message = DEATHS[i]
    r = subprocess.run([sys.executable, "-c", f"import ctypes as C\nfrom matchtigs_amd import _lib\nL = _lib.load()\n{_SETUP}{code}\n"],
                       capture_output=True, text=True, cwd=str(ROOT), timeout=120)
    assert r.returncode != 0 and message in r.stderr, (code, r.returncode, r.stderr[-500:])


def test_the_times_are_zero_before_a_call_and_the_checks_come_first(product_lib):
    out = (C.c_double * 8)()
    product_lib.mtg_last_kmer_correct_times(out)
    assert list(out) == [0.0] * 8  # (no call on this thread yet)
    source = (ROOT / "matchtigs_amd" / "csrc" / "engine_api.cpp").read_text()
    body = source[source.index("void mtg_kmer_index_correct("):source.index("void mtg_kmer_index_correct_store(")]
    assert body.index("min_solid must be >= 1") < body.index("if (n == 0) return;") < body.index("device_kmer_index_correct(")
    header = (ROOT / "include" / "mtg_engine.h").read_text()
    for part in ("CANDIDATE", "AMBIGUOUS", "need = min(W, |cover(p)|)", "typedef struct mtg_correct_params { uint32_t min_solid, rounds; }"):
        assert part in header, part


# ---- the command line ----
def _cli(*a):
    return subprocess.run([sys.executable, "-m", "matchtigs_amd", *a], capture_output=True, text=True, cwd=str(ROOT), timeout=300)


CF, CO, CR_OUT = "--correct-fa", "--correct-out", "--correct-report-out"
SEQ = ("--seq-in", "a.fa", "--unitigs-fa-out", "u.fa")
REFUSED = [
    ((*SEQ, CO, "o.fa"), [CO, CF]),
    ((*SEQ, CR_OUT, "o.tsv"), [CR_OUT, CF]),
    ((*SEQ, "--correct-min-solid", "3"), ["--correct-min-solid", CF]),
    ((*SEQ, "--correct-rounds", "2"), ["--correct-rounds", CF]),
    ((*SEQ, CF, "r.fa"), [CF, CO, CR_OUT]),
    ((*SEQ, CF, "r.fa", CF, "s.fa", CO, "o.fa"), [CO, CF, "1", "2"]),
    ((*SEQ, CF, "r.fa", CO, "o.fa", CO, "p.fa"), [CO, CF, "2", "1"]),
    ((*SEQ, CF, "r.fa", CO, "o.fa", "--correct-min-solid", "0"), ["--correct-min-solid", ">= 1"]),
    ((*SEQ, CF, "r.fa", CO, "o.fa", "--correct-rounds", "0"), ["--correct-rounds", "1..8"]),
    ((*SEQ, CF, "r.fa", CO, "o.fa", "--correct-rounds", "9"), ["--correct-rounds", "1..8"]),
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
    for route, extra in (("--seq-in", (CO, t("o.fa"))), ("--fa-in", (CR_OUT, t("r.tsv"))),
                         ("--bcalm-in", (CO, t("o.fa.gz"), CR_OUT, t("r.tsv"), "--correct-min-solid", "2", "--correct-rounds", "8"))):
        r = _cli(route, t("no_such.fa"), "-k", "21", CF, t("r.fa"), *extra)
        assert r.returncode != 0 and "error:" not in r.stderr and "cannot open" in r.stderr, (route, extra, r.stderr[-1000:])
    out = _cli("--help").stdout
    for flag in (CF, CO, CR_OUT, "--correct-min-solid", "--correct-rounds"):
        assert flag in out


# ---- the wrapper ----
def _asked(*a, **kw):
    raise AssertionError("the library was asked")


def _shell_index(cls, handle):
    ix = cls.__new__(cls)
    ix._L = types.SimpleNamespace(mtg_kmer_index_free=lambda h: None, mtg_tig_index_free=lambda h: None, mtg_kmer_index_correct=_asked,
                                  mtg_kmer_index_correct_store=_asked)
    ix._h, ix.locating, ix.weighted, ix.colored, ix.n_colors = handle, False, False, False, 0
    return ix


def test_the_wrappers_errors_come_before_the_library(monkeypatch):
    monkeypatch.setattr(_lib, "load", _asked)
    with pytest.raises(TypeError):
        api.ReadCorrector(["ACGT"])
    with pytest.raises(TypeError) as e:
        api.ReadCorrector(_shell_index(api.TigIndex, 1))
    assert "sparse" in str(e.value)
    with pytest.raises(ValueError) as e:
        api.ReadCorrector(_shell_index(api.KmerIndex, None))
    assert str(e.value) == "the index is closed"
    for kw in ({"min_solid": 0}, {"min_solid": -1}, {"min_solid": 1.5}, {"min_solid": True}, {"min_solid": 1 << 32}, {"rounds": 0}, {"rounds": 9},
               {"rounds": 2.0}, {"rounds": None}):
        with pytest.raises(ValueError) as e:
            api.ReadCorrector(_shell_index(api.KmerIndex, 1), **kw)
        assert next(iter(kw)) in str(e.value)
    c = api.ReadCorrector(_shell_index(api.KmerIndex, 1))
    assert (c.min_solid, c.rounds) == (4, 2)
    with c as same:
        assert same is c
    with pytest.raises(ValueError) as e:
        c.correct(["ACGT"])
    assert str(e.value) == "the corrector is closed"
    c.close()  # (twice is fine)
    ix = _shell_index(api.KmerIndex, 1)
    c = api.ReadCorrector(ix, 1, 8)
    ix._h = None
    with pytest.raises(ValueError) as e:
        c.correct(["ACGT"])
    assert str(e.value) == "the index is closed"
    import matchtigs_amd

    assert matchtigs_amd.ReadCorrector is api.ReadCorrector and matchtigs_amd.last_kmer_correct_times is api.last_kmer_correct_times


# ---- the text patching, with the library stubbed out by the restatement ----
class _Store:
    def __init__(self, records):
        self.records = records

    def arrays(self):
        off = np.cumsum([0] + [len(s) for s in self.records]).astype(np.uint64)
        return np.frombuffer("".join(self.records).encode("latin-1"), np.uint8), off


class _Ctx(types.SimpleNamespace):
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return None


def _stub_api(index, k, parsed):
    """parsed: path -> (records, names), what the readers would hand out."""
    solid = CR.solid_set(index, k)

    def corrector(ix, W, R):
        def correct(store):
            r = CR.correct(solid, k, store.records, W, R)
            off = store.arrays()[1]
            return api.CorrectionResult(k, off, *(np.array(r[f], np.uint64) for f in (
                "kmers", "valid", "found", "found_after", "candidates", "ambiguous", "corrected")), np.array(r["positions"], np.uint64),
                np.frombuffer("".join(r["bases"]).encode(), np.uint8), np.array(r["round_corrected"], np.uint64))
        return _Ctx(correct=correct, rounds=R, min_solid=W)

    return types.SimpleNamespace(
        KmerIndex=lambda *a, **kw: _Ctx(), ReadCorrector=corrector, patched_bytes=api.patched_bytes,
        read_sequences_named=lambda path: (_Store(parsed[path][0]), parsed[path][1]),
        read_fastq=lambda path, q, device, named: (_Store(parsed[path][0]), parsed[path][1], None))


def test_the_text_is_patched_byte_for_byte(tmp_path, capsys):
    k = 9
    rng = random.Random(34)
    g = _dna(rng, 120)
    good = [g[0:40], g[30:75], synth.revcomp(g[60:110]), g[5:33]]
    bad = []
    for s in good:
        s = list(s)
        p = rng.randrange(10, len(s) - 10)
        s[p] = rng.choice([c for c in "ACGT" if c != s[p]])
        bad.append("".join(s))
    bad[1] = bad[1].lower()
    bad[3] = "N" + bad[3][1:]
    names = ["r0", "r1", "r2", "r3"]
    wrapped = "".join(f">{n} some text\n" + "".join(s[i:i + 17] + "\n" for i in range(0, len(s), 17)) for n, s in zip(names, bad))
    texts = {
        "multi.fa": wrapped.encode(),
        "crlf.fa": wrapped.replace("\n", "\r\n").encode() + b"\r\n>empty\r\n",
        "reads.fq": "".join(f"@{n} x\n{s}\n+{n}\n{'I' * len(s)}\n" for n, s in zip(names, bad)).encode(),
        "crlf.fq": "".join(f"@{n}\r\n{s}\r\n+\r\n{'A' * len(s)}\r\n" for n, s in zip(names, bad)).encode()[:-2],
        "zipped.fa.gz": gzip.compress("".join(f">{n}\n{s}\n" for n, s in zip(names, bad)).encode()),
    }
    parsed = {}
    for name, raw in texts.items():
        (tmp_path / name).write_bytes(raw)
        parsed[str(tmp_path / name)] = (bad + [""] if name == "crlf.fa" else bad, names + ["empty"] if name == "crlf.fa" else names)
    fastq = {str(tmp_path / "reads.fq"), str(tmp_path / "crlf.fq")}
    paths = [str(tmp_path / n) for n in texts]
    outs = [str(tmp_path / ("out_" + n)) for n in texts]
    args = types.SimpleNamespace(k=k, device=0, correct_fa=paths, correct_out=outs, correct_report_out=str(tmp_path / "report.tsv.gz"),
                                 correct_min_solid=2, correct_rounds=None, compression_level=6)
    cli._correct(_stub_api([g], k, parsed), args, None, fastq)
    want = CR.correct(CR.solid_set([g], k), k, bad, 2, 2)
    assert want["corrected"][:3] == [1, 1, 1] and want["texts"][1].islower() and "N" in want["texts"][3]
    report = gzip.decompress((tmp_path / "report.tsv.gz").read_bytes()).decode().splitlines()
    expected = CR.report_lines("", names, bad, want)
    assert report[0] == expected[0]
    rows = report[1:]
    at = 0
    for name, path, out in zip(texts, paths, outs):
        raw = gzip.decompress(texts[name]) if name.endswith(".gz") else texts[name]
        got = Path(out).read_bytes()
        if name.endswith(".gz"):
            assert got[:2] == b"\x1f\x8b"
            got = gzip.decompress(got)
        differ = [i for i in range(len(raw)) if raw[i] != got[i]]
        assert len(got) == len(raw) and len(differ) == sum(want["corrected"]), name
        # the bases, taken out of the patched text by the same line rules, are the restatement's corrected reads
        n_rec = len(parsed[path][0])
        where = cli._sequence_bytes(got, n_rec, path in fastq)
        assert bytes(np.frombuffer(got, np.uint8)[where]).decode() == "".join(want["texts"]), name
        n_rows = n_rec
        assert rows[at:at + 4] == [path + line for line in expected[1:]], name
        if name == "crlf.fa":
            assert rows[at + 4] == f"{path}\tempty\t0\t0\t0\t0\t0\t0\t0\t0\t-"
        at += n_rows
    assert at == len(rows)
    err = capsys.readouterr().err
    assert err.count("Correcting ") == len(texts) and f"{sum(want['candidates'])} candidates" in err and " substitutions in 2 rounds" in err


def test_a_text_that_is_not_the_readers_is_refused(tmp_path):
    k = 5
    path = tmp_path / "r.fa"
    path.write_text(">a\nACGTACGTAC\n")
    parsed = {str(path): (["ACGTACGTAA"], ["a"])}  # (a reader that disagrees with the text)
    args = types.SimpleNamespace(k=k, device=0, correct_fa=[str(path)], correct_out=[str(tmp_path / "o.fa")], correct_report_out=None,
                                 correct_min_solid=None, correct_rounds=None, compression_level=6)
    with pytest.raises(SystemExit) as e:
        cli._correct(_stub_api(["ACGTACGTAC"], k, parsed), args, None, ())
    assert str(path) in str(e.value) and not (tmp_path / "o.fa").exists()
