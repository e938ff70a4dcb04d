"""Read correction on the GPU (kmer_correct_device.hpp, api.ReadCorrector): every output as exact integers and bytes
against the restatement (kmer_correct_ref.py, which knows nothing about bit arrays, waves or tables). k in 1 .. 64 puts the 3 c tasks
of a candidate below, at and above the 64 lanes of a wave and runs both identities of a window, the code (k <= 31) and the hashes."""
import gzip
import random
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import collision_cases as CC
import kmer_correct_ref as CR
from matchtigs_amd import api, synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
KS = (1, 2, 5, 16, 21, 22, 31, 32, 33, 64)
FIELDS = ("kmers", "valid", "found", "found_after", "candidates", "ambiguous", "corrected")


@pytest.fixture(scope="module")
def gpu(product_lib):
    import torch

    if product_lib.mtg_device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("these tests need a GPU: the corrector has no CPU path")
    return torch


def _dna(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _genome(rng, k, n):
    """Small k: a random text over ACGT holds every k-mer, so nothing could be an error; fewer letters leave k-mers out."""
    return _dna(rng, n, "A" if k == 1 else "AC" if k <= 5 else "ACGT")


def _plant(s, positions, rng):
    s = list(s)
    for p in positions:
        s[p] = rng.choice([c for c in "ACGT" if c != s[p].upper()])
    return "".join(s)


def _same(got, want, reads, what):
    for f in FIELDS:
        a = getattr(got, f)
        assert a.dtype == np.uint64 and a.tolist() == want[f], (what, f, a.tolist()[:40], want[f][:40])
    assert got.positions.dtype == np.uint64 and got.positions.tolist() == want["positions"], (what, got.positions.tolist()[:40], want["positions"][:40])
    assert got.bases.dtype == np.uint8 and got.bases.tobytes().decode() == "".join(want["bases"]), what
    assert got.round_corrected.tolist() == want["round_corrected"], (what, got.round_corrected.tolist(), want["round_corrected"])
    assert got.apply(reads) == want["texts"], what
    assert [got.record_of(i) for i in range(len(got.positions))] == [r for r, subs in enumerate(want["substitutions"]) for _ in subs], what


def _check(index, k, reads, rules, what=""):
    """One index, one corrector per (W, R); returns the restatement's answers by rule."""
    solid, memo = CR.solid_set(index, k), {}
    wants = {}
    with api.KmerIndex(index, k) as ix:
        for W, R in rules:
            wants[W, R] = want = CR.correct(solid, k, reads, W, R, memo)
            with api.ReadCorrector(ix, W, R) as c:
                _same(c.correct(reads), want, reads, (what, k, W, R))
    return wants


def _rules(k):
    return [(W, R) for W in sorted({1, 4, k, k + 1}) for R in (1, 2, 8)]


@pytest.mark.parametrize("k", KS)
def test_reads_of_every_length_with_one_error_on_either_strand_in_either_case(gpu, k):
    rng = random.Random(3400 + k)
    g = _genome(rng, k, 6 * k + 120)
    reads = []
    for n in (k, k + 1, 2 * k - 1, 2 * k, 3 * k):
        for strand in (0, 1):
            at = rng.randrange(len(g) - n)
            s = g[at:at + n]
            s = synth.revcomp(s) if strand else s
            s = _plant(s, [rng.randrange(n)], rng)
            reads.append(s.lower() if strand else s)
            reads.append("".join(c.lower() if rng.random() < 0.5 else c for c in s))
    wants = _check([g, g[:k - 1] if k > 1 else ""], k, reads, _rules(k))
    if k >= 16:
        assert sum(wants[1, 1]["corrected"]) >= 10 and any(b != b.upper() for t in wants[1, 1]["texts"] for b in t)


@pytest.mark.parametrize("k", KS)
def test_one_error_at_every_position_across_the_word_boundaries(gpu, k):
    """One read per position of the error, one after the other: the reads lie across every multiple of 64 of the concatenated data,
    where the bit arrays change their word and the query's threads their run."""
    rng = random.Random(3500 + k)
    g = _genome(rng, k, 4 * k + 60)
    n = min(len(g), 2 * k + 3)
    read = g[7:7 + n]
    reads = ["ACGTA"] + [_plant(read, [j], rng) for j in range(n)]
    assert len(read) % 64 != 0
    wants = _check([g], k, reads, [(1, 1), (4, 2), (k + 1, 1)])
    if k >= 16:
        assert wants[4, 2]["corrected"][1:] == [1] * n and wants[4, 2]["texts"][1:] == [read] * n


@pytest.mark.parametrize("k", KS)
def test_two_errors_at_every_distance_and_three_within_k(gpu, k):
    rng = random.Random(3600 + k)
    g = _genome(rng, k, 6 * k + 80)
    n = 3 * k + 5
    read = g[11:11 + n]
    # (the first two: an error in the last base of one read and in the first of the next, neighbours in one packed 32-bit word)
    two = [_plant(read, [n - 1], rng), _plant(read, [0], rng)] + [_plant(read, [k // 2 + 1, k // 2 + 1 + d], rng) for d in range(1, k + 2)]
    three = []
    for _ in range(12):
        at = rng.randrange(n - k) if n > k else 0
        three.append(_plant(read, sorted(rng.sample(range(at, at + k), min(3, k))), rng))
    wants = _check([g], k, two + three, [(1, 1), (1, 2), (2, 8), (4, 2), (k, 8)])
    if k >= 16:
        assert wants[1, 2]["round_corrected"][1] > 0  # the middle error of a triple needs the second round
        assert n % 16 and wants[1, 1]["positions"][:2] == [n - 1, n]  # two substitutions of one round in one word
        assert any(c == 2 for c in wants[1, 1]["corrected"][2:k + 3])  # two errors closer than k, both put right at once


@pytest.mark.parametrize("k", KS)
def test_an_n_at_every_position_beside_an_error(gpu, k):
    rng = random.Random(3700 + k)
    g = _genome(rng, k, 5 * k + 60)
    n = 2 * k + 6
    read = _plant(g[5:5 + n], [k + 1], rng)
    reads = [read[:j] + rng.choice("Nn-") + read[j + 1:] for j in range(n)]
    _check([g], k, reads, [(1, 1), (4, 2), (k, 1)])


@pytest.mark.parametrize("k", [2, 5, 16, 31, 32, 64])
def test_two_neighbours_of_a_weak_window_are_ambiguous(gpu, k):
    rng = random.Random(3800 + k)
    g = _genome(rng, k, 4 * k + 40)
    m = 2 * k + 3
    others = [c for c in "ACGT" if c != g[m]]
    index = [g, g[:m] + others[0] + g[m + 1:]]  # two solid spellings of position m ...
    read = g[m - k:m] + others[1] + g[m + 1:m + k + 2]  # ... and a read with a third
    wants = _check(index, k, [read, synth.revcomp(read)], [(1, 1), (4, 2), (k, 8)])
    if k >= 16:
        assert wants[4, 2]["ambiguous"] == [1, 1] and wants[4, 2]["corrected"] == [0, 0]


@pytest.mark.parametrize("k", [2, 16, 22, 32, 64])
def test_a_palindrome_as_the_fix(gpu, k):
    rng = random.Random(3900 + k)
    half = _dna(rng, k // 2)
    pal = half + synth.revcomp(half)
    assert synth.revcomp(pal) == pal
    g = _dna(rng, 40) + pal + _dna(rng, 40)
    reads = [_plant(pal, [j], rng) for j in range(k)] + [_plant(g[30:50 + k], [10 + k // 2], rng)]
    wants = _check([g], k, reads, [(1, 1), (4, 2)])
    if k >= 16:
        assert wants[1, 1]["texts"][:k] == [pal] * k


@pytest.mark.parametrize("k", [1031, 1056])
def test_substituted_windows_whose_hash_collides_with_another_class(gpu, k):
    """collision_cases' pair: the windows of y that hold the whole block collide in all 64 bits of the hash, tag included, with the
    windows of x at the same place. An index of x alone must not take a corrected window of y for solid; an index of both must.
    The reads are k + 8 bases of x and y, cut so that (nearly) all of their windows hold the block."""
    x, y = CC.cases()["pair"]
    rng = random.Random(k)
    s = 40 + CC.BLOCK - k
    cut_x, cut_y = x[s:s + k + 8], y[s:s + k + 8]
    at = (k + 8) // 2
    bad_y, bad_x = _plant(cut_y, [at], rng), _plant(cut_x, [at], rng)
    reads = [bad_y, synth.revcomp(bad_y), bad_x, cut_y]
    only_x = _check([x], k, reads, [(4, 2)], "x alone")
    both = _check([x, y], k, reads, [(4, 2)], "x and y")
    assert only_x[4, 2]["corrected"] == [0, 0, 1, 0] and both[4, 2]["corrected"] == [1, 1, 1, 0]
    assert only_x[4, 2]["candidates"][0] == k + 8 and both[4, 2]["texts"][0] == cut_y and both[4, 2]["found_after"] == [9] * 4


@pytest.mark.parametrize("k", [2, 3, 5])
def test_dense_sets_where_a_position_is_substituted_twice(gpu, k):
    """Random reads against a small, dense set over two letters: substitutions of one round that share a window, positions that
    are candidates again and get another base, or their first one back (kmer_correct_ref's note)."""
    rng = random.Random(3400 + k)
    twice = False
    for i in range(30):
        index = [_dna(rng, rng.randint(0, 4 * k + 12), "AC") for _ in range(rng.randint(1, 4))]
        pool = "".join(index) + synth.revcomp("".join(index)) + "ACGT"
        reads = []
        for _ in range(8):
            at = rng.randrange(len(pool))
            s = list(pool[at:at + rng.randint(0, 3 * k + 6)])
            for _ in range(rng.randint(0, 3)):
                if s:
                    s[rng.randrange(len(s))] = rng.choice("NnACGTacgt")
            reads.append("".join(s))
        wants = _check(index, k, reads, [(1, 8), (2, 3), (4, 2)], i)
        twice |= any(sum(w["round_corrected"]) > len(w["positions"]) for w in wants.values())
    assert twice or k == 2, k


def test_records_without_windows_and_no_record_at_all(gpu):
    rng = random.Random(34)
    for k in (5, 33):
        g = _genome(rng, k, 4 * k + 30)
        bad = _plant(g[3:3 + 2 * k], [k], rng)
        reads = ["", "ACG"[:k - 1], "N" * (2 * k), "", bad, "", g[:k - 1], "n" * k + "N", bad.lower(), ""]
        _check([g], k, reads, [(1, 1), (4, 2)])
        _check([g], k, [], [(4, 2)])
        _check([g], k, ["", ""], [(4, 2)])
        _check([g], k, ["ACGTN"[:k - 1]], [(4, 2)])
        _check([""], k, [bad, g], [(4, 2)])  # an index without k-mers: every good position is a candidate, none has a fix


def test_every_position_a_candidate_beyond_the_grid(gpu):
    """More candidates than the evaluation's capped grid has waves (8192): the waves stride."""
    k = 16
    rng = random.Random(35)
    g = _dna(rng, 600)
    reads = [_dna(rng, 120) for _ in range(90)] + [_plant(g[40:140], [50], rng)]
    wants = _check([g], k, reads, [(4, 2)])
    assert sum(wants[4, 2]["candidates"]) > 8192 + 64 and wants[4, 2]["corrected"][-1] == 1


def test_the_index_answers_its_probes_as_before_and_correctors_are_independent(gpu):
    k = 21
    rng = random.Random(36)
    g = _dna(rng, 500)
    windows = len(g) - k + 1
    reads = [_plant(g[at:at + 80], [40], rng) for at in range(0, 400, 37)] + ["ACGTNNACGT", ""]
    probes = ("query", "locate", "abundance", "color_hits")
    with api.KmerIndex([g], k, locate=True, weights=list(range(1, windows + 1)), colors=[1 + i % 3 for i in range(windows)], n_colors=2) as ix:
        def answers():
            out = []
            for name in probes:
                r = getattr(ix, name)(reads, True) if name != "locate" else ix.locate(reads)
                out.append({f: np.asarray(v).tolist() for f, v in vars(r).items() if isinstance(v, np.ndarray)})
            return out

        before = answers()
        want = CR.correct(CR.solid_set([g], k), k, reads, 4, 2)
        with api.ReadCorrector(ix) as a, api.ReadCorrector(ix, 1, 1) as b:
            assert (a.min_solid, a.rounds, b.min_solid, b.rounds) == (4, 2, 1, 1)
            first = a.correct(reads)
            assert answers() == before
            _same(b.correct(reads), CR.correct(CR.solid_set([g], k), k, reads, 1, 1), reads, "b")
            api.release_device_memory(0)
            again = a.correct(reads)
            assert answers() == before
            _same(first, want, reads, "first")
            _same(again, want, reads, "again")
            times = api.last_kmer_correct_times()
            assert set(times) == {"upload_ms", "pack_ms", "query_ms", "flag_ms", "evaluate_ms", "apply_ms", "download_ms", "total_ms"}
            assert times["evaluate_ms"] > 0 and times["total_ms"] >= times["evaluate_ms"]
        with api.ReadCorrector(ix) as c:
            store_like = (np.frombuffer("".join(reads).encode(), np.uint8), np.cumsum([0] + [len(s) for s in reads]).astype(np.uint64))
            _same(c.correct(store_like), want, reads, "arrays")
    with pytest.raises(ValueError) as e:
        a.correct(reads)
    assert str(e.value) == "the corrector is closed"
    with pytest.raises(ValueError) as e:
        api.ReadCorrector(ix)
    assert str(e.value) == "the index is closed"
    with api.TigIndex([g], k) as sparse, pytest.raises(TypeError):
        api.ReadCorrector(sparse)


def test_through_the_product(gpu, tmp_path):
    """--seq-in reads with planted errors and --min-abundance 2: the solid set is what the reads show twice. A FASTQ file and a gzipped,
    wrapped FASTA file are corrected in one run: the outputs differ from the inputs exactly at the reported substitutions, the report
    is the restatement's, a query of the corrected files finds found_after, and no other output notices the new flags."""
    from matchtigs_amd import __main__ as cli

    k = 15
    rng = random.Random(340)
    g = _dna(rng, 1200)
    clean = [g[at:at + 100] for at in range(0, 1101, 25)]  # every k-mer of g at least twice (the ends: the first and last read twice)
    clean += [clean[0], clean[-1]]
    noisy = [_plant(s, rng.sample(range(100), rng.choice([1, 1, 2, 3])), rng) for s in clean[:30]]
    noisy = [synth.revcomp(s) if i % 2 else s for i, s in enumerate(noisy)]
    noisy[3] = noisy[3].lower()
    noisy[5] = noisy[5][:50] + "N" + noisy[5][51:]
    seq_in = tmp_path / "reads.fa"
    seq_in.write_text("".join(f">r{i}\n{s}\n" for i, s in enumerate(clean + noisy)))
    counts = {}
    for s in clean + noisy:
        for piece in s.upper().split("N"):
            for p in range(len(piece) - k + 1):
                x = synth.canonical(piece[p:p + k])
                counts[x] = counts.get(x, 0) + 1
    solid = {x for x, c in counts.items() if c >= 2}
    assert CR.solid_set([g], k) <= solid

    fq_reads, fa_reads = noisy[:15] + ["", "ACGT"], noisy[15:] + [_dna(rng, 60)]
    fq_names, fa_names = [f"q{i}" for i in range(len(fq_reads))], [f"a{i}" for i in range(len(fa_reads))]
    fq, fa = tmp_path / "noisy.fq", tmp_path / "noisy.fa.gz"
    fq.write_text("".join(f"@{n} x\n{s}\n+\n{'I' * len(s)}\n" for n, s in zip(fq_names, fq_reads)))
    fa.write_bytes(gzip.compress("".join(f">{n} y\n" + "".join(s[i:i + 37] + "\n" for i in range(0, len(s), 37)) for n, s in zip(fa_names, fa_reads)).encode()))

    t = lambda name: str(tmp_path / name)
    common = [sys.executable, "-m", "matchtigs_amd", "--seq-in", str(seq_in), "-k", str(k), "--min-abundance", "2"]
    shared = lambda tag: ["--unitigs-fa-out", t(tag + ".u.fa"), "--query-fa", str(fq), "--query-out", t(tag + ".q.tsv"), "--count-fa", str(fq),
                          "--count-out", t(tag + ".c.tsv")]

    def run(*flags):
        r = subprocess.run(common + list(flags), capture_output=True, text=True, cwd=str(ROOT), timeout=600)
        assert r.returncode == 0, (flags, r.returncode, r.stderr[-2000:])
        return r.stderr

    err = run(*shared("with"), "--correct-fa", str(fq), "--correct-fa", str(fa), "--correct-out", t("fixed.fq.gz"), "--correct-out", t("fixed.fa"),
              "--correct-report-out", t("report.tsv"), "--correct-min-solid", "3", "--correct-rounds", "3")
    plain_err = run(*shared("plain"))
    for x in (".u.fa", ".q.tsv", ".c.tsv"):  # the other outputs do not notice the new flags
        assert Path(t("with" + x)).read_bytes() == Path(t("plain" + x)).read_bytes(), x
    assert err.count("Correcting ") == 2 and "Correcting" not in plain_err

    report = Path(t("report.tsv")).read_text().splitlines()
    want_lines, found_after = [], {}
    for path, names, reads, out, is_fq in ((fq, fq_names, fq_reads, t("fixed.fq.gz"), True), (fa, fa_names, fa_reads, t("fixed.fa"), False)):
        want = CR.correct(solid, k, reads, 3, 3)
        lines = CR.report_lines(str(path), names, reads, want)
        want_lines += lines[1:] if want_lines else lines
        raw, got = path.read_bytes(), Path(out).read_bytes()
        raw = gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw
        assert (got[:2] == b"\x1f\x8b") == out.endswith(".gz")
        got = gzip.decompress(got) if out.endswith(".gz") else got
        where = cli._sequence_bytes(raw, len(reads), is_fq)
        differ = [i for i in range(len(raw)) if raw[i] != got[i]]
        assert len(raw) == len(got) and differ == [int(where[p]) for p in want["positions"]], path  # exactly the substitutions
        assert [chr(got[i]) for i in differ] == [b.lower() if chr(raw[i]).islower() else b for i, b in zip(differ, want["bases"])], path
        assert sum(want["corrected"]) >= 8
        found_after[out] = (names, want["found_after"])
    assert report == want_lines

    # a second run that queries the corrected files reports found_after
    run("--query-fa", t("fixed.fq.gz"), "--query-fa", t("fixed.fa"), "--query-out", t("after.q.tsv"))
    rows = [line.split("\t") for line in Path(t("after.q.tsv")).read_text().splitlines()[1:]]
    assert [(r[0], int(r[4])) for r in rows] == [(n, f) for names, fs in found_after.values() for n, f in zip(names, fs)]
