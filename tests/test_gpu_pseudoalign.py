"""Pseudoalignment with equivalence classes on the GPU (pseudoalign_device.hpp, api.Pseudoaligner): every output as
exact integers against the restatement (pseudoalign_ref.py, which knows nothing about counters on a device, waves or tables), on a
coloured KmerIndex and on TigIndex.annotated with both payload layouts and bucket_limit in {default, 1}."""
import gzip
import random
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import pseudoalign_ref as PA
from matchtigs_amd import api, synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
RULES = [(P, over) for P in (1, 500, 999, 1000) for over in ("found", "valid")]


@pytest.fixture(scope="module")
def gpu(product_lib):
    import torch

    if product_lib.mtg_device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("these tests need a GPU: the pseudoaligner has no CPU path")
    return torch


def _dna(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _kinds(index, masks, C, k):
    """The five coloured indexes of one sequence set, as (name, constructor)."""
    kinds = [("table", lambda: api.KmerIndex(index, k, colors=masks, n_colors=C))]
    for layout in ("dense", "runs"):
        for limit in (None, 1):
            kinds.append((f"sparse {layout} limit={limit}", lambda layout=layout, limit=limit: api.TigIndex.annotated(
                index, k, bucket_limit=limit, colors=masks, n_colors=C, payload_layout=layout)))
    return kinds


def _same(result, want, what):
    for f in ("kmers", "valid", "found", "masks"):
        got = getattr(result, f)
        assert got.dtype == np.uint64 and got.tolist() == want[f], (what, f, got.tolist()[:40], want[f][:40])


def _check(index, masks, C, k, calls, rules=RULES, min_kmers=(1,), kinds=None):
    """calls: [(reads, mates or None)], aligned in turn by one aligner per (index kind, rule); every result, then classes / totals /
    color_reads after each call."""
    wants = {}
    for P, over in rules:
        for mk in min_kmers:
            ref = PA.Aligner(index, masks, C, k, P, over, mk)
            steps = []
            for reads, mates in calls:
                want = ref.align(reads, mates)
                steps.append((want, ref.classes(), dict(ref.totals), ref.color_reads()))
            wants[P, over, mk] = steps
    for name, make in kinds or _kinds(index, masks, C, k):
        with make() as ix:
            for (P, over, mk), steps in wants.items():
                with api.Pseudoaligner(ix, P, over, mk) as a:
                    for (reads, mates), (want, classes, totals, color_reads) in zip(calls, steps):
                        what = (name, k, C, P, over, mk)
                        r = a.align(reads, mates)
                        _same(r, want, what)
                        cl = a.classes()
                        assert {f: cl[f].tolist() for f in cl} == classes, (what, cl, classes)
                        assert a.totals == totals, (what, a.totals, totals)
                        assert tuple(x.tolist() for x in a.color_reads) == color_reads, what


def _random_case(rng, k, C):
    genome = _dna(rng, 3 * k + 90)
    index = [genome[:k + 40], "", genome[k + 20:2 * k + 70], genome[:k - 1], synth.revcomp(genome[2 * k + 30:])]
    windows = sum(max(0, len(s) - k + 1) for s in index)
    top = 1 << (C - 1)
    palette = [0, 1, top, (1 << C) - 1, top | 1] + [rng.getrandbits(C) for _ in range(4)]
    masks, m = [], 1
    for _ in range(windows):  # runs of equal masks with single outliers
        if rng.random() < 0.2:
            m = rng.choice(palette)
        masks.append(m if rng.random() < 0.9 else rng.choice(palette))
    both = genome + synth.revcomp(genome)
    reads = []
    for _ in range(10):
        at = rng.randrange(len(both) - k)
        s = list(both[at:at + rng.randint(k, 2 * k + 70)])
        if rng.random() < 0.5:
            s[rng.randrange(len(s))] = rng.choice("NnXacgt")
        if rng.random() < 0.3:
            s[rng.randrange(len(s))] = rng.choice("ACGT")
        reads.append("".join(s))
    reads += ["", genome[:k - 1], _dna(rng, k + 5), "N" * (k + 3)]
    rng.shuffle(reads)
    mates = reads[5:] + reads[:5]
    return index, masks, reads, mates, top


@pytest.mark.parametrize("k", [1, 2, 5, 16, 31, 32, 33, 64])
def test_random_sets(gpu, k):
    rng = random.Random(3300 + k)
    seen = {"top bit set": False, "top bit clear": False, "nothing assigned": False}
    for C in (1, 2, 3, 63, 64):
        index, masks, reads, mates, top = _random_case(rng, k, C)
        _check(index, masks, C, k, [(reads, None), (reads, mates)])
        got = PA.Aligner(index, masks, C, k, 500).align(reads, mates)["masks"]
        if C >= 63:
            seen["top bit set"] |= any(m & top for m in got)
            seen["top bit clear"] |= any(m and not m & top for m in got)
        seen["nothing assigned"] |= 0 in got
    assert all(seen.values()), (k, seen)


def test_worked_example(gpu):
    k, index, masks = PA.EXAMPLE_K, PA.EXAMPLE_INDEX, PA.example_colors()
    reads = [row[0] for row in PA.EXAMPLE_ROWS]
    mates = [row[1] or "" for row in PA.EXAMPLE_ROWS]
    rules = [(P, over) for P in (1000, 500, 600) for over in ("found", "valid")]
    _check(index, masks, 3, k, [(reads, mates)], rules)
    for name, make in _kinds(index, masks, 3, k):
        with make() as ix:
            for P, column in ((1000, 6), (500, 7)):
                with api.Pseudoaligner(ix, threshold_permille=P) as a:
                    r = a.align(reads, mates)
                    assert r.masks.tolist() == [row[column] for row in PA.EXAMPLE_ROWS], (name, P)
                    assert r.kmers.tolist() == [row[2] for row in PA.EXAMPLE_ROWS] and r.found.tolist() == [row[4] for row in PA.EXAMPLE_ROWS]
                    assert r.colors(0) == [0, 1] and r.colors(4) == []
            with api.Pseudoaligner(ix, 600, "found") as a, api.Pseudoaligner(ix, 600, "valid") as b:
                assert a.align(reads[5:6], mates[5:6]).masks.tolist() == [0b101] and b.align(reads[5:6], mates[5:6]).masks.tolist() == [0]
                times = api.last_pseudoalign_times()
                assert set(times) == {"upload_ms", "pack_ms", "probe_ms", "mask_ms", "dictionary_ms", "download_ms"}
                assert all(v >= 0 for v in times.values()) and times["probe_ms"] > 0


@pytest.mark.parametrize("k", [5, 32])
def test_a_read_over_four_runs_with_the_change_and_an_n_everywhere(gpu, k):
    """A read of 64 * 3 + k bases spans four threads' runs of window starts. The text is twice as long and its colour set changes once
    (disjoint colours before and after), so the reads cut at every offset see the change at every one of their positions in turn; then
    one read with an N at every position in turn."""
    rng = random.Random(64 + k)
    L = 64 * 3 + k
    text = _dna(rng, 2 * L)
    W = len(text) - k + 1
    change = L
    masks = [0b01 if i < change else 0b10 for i in range(W)]
    moving = [text[s:s + L] for s in range(L + 1)]
    kinds = _kinds([text], masks, 2, k)
    _check([text], masks, 2, k, [(moving, None)], [(1000, "found"), (500, "found"), (1, "valid")], kinds=kinds[:1] + kinds[3:4])
    read = moving[L // 2]
    holes = [read[:p] + "N" + read[p + 1:] for p in range(L)]
    _check([text], masks, 2, k, [(holes, None)], [(1000, "found"), (1000, "valid"), (500, "valid")], kinds=kinds[:1] + kinds[2:3])


def test_records_without_windows_or_hits(gpu):
    k = 6
    rng = random.Random(6)
    text = _dna(rng, 80)
    masks = [0b11] * (len(text) - k + 1)
    other = "".join({"A": "C", "C": "A", "G": "T", "T": "G"}[c] for c in text[:30])
    reads = ["N" * 20, other, "", "ACG", text[:k - 1], text[10:40], "ACGTN" * 5]
    empty = [""] * len(reads)
    calls = [(reads, None), (reads, empty), (empty, reads), (empty, None), (empty, empty), (["", "AC"], ["A", ""])]
    _check([text], masks, 2, k, calls, [(1000, "found"), (1000, "valid"), (1, "found")])
    with api.KmerIndex([text], k, colors=masks, n_colors=2) as ix, api.Pseudoaligner(ix) as a:
        r = a.align([])
        assert len(r.masks) == 0 and a.totals["fragments"] == 0 and len(a.classes()["mask"]) == 0
        r = a.align([], [])
        assert len(r.masks) == 0


def test_mask_zero_classes_are_found_and_lower_every_ratio(gpu):
    k = 11
    rng = random.Random(50)
    text = _dna(rng, 120)
    assert len({synth.canonical(text[i:i + k]) for i in range(len(text) - k + 1)}) == len(text) - k + 1  # (no class occurs twice)
    W = len(text) - k + 1
    masks = [0 if i % 3 == 0 else 0b101 if i < W // 2 else 0b010 for i in range(W)]
    reads = [text[:40], text[30:90], text[70:], text[3:3 + k], text[:k]]
    want = PA.Aligner([text], masks, 3, k, 1000).align(reads)
    assert all(m == 0 for m in want["masks"][:3]) and want["found"][4] == 1 and want["hits"][4] == [0, 0, 0]  # found, no column
    assert PA.Aligner([text], masks, 3, k, 600).align(reads)["masks"][0] == 0b101
    _check([text], masks, 3, k, [(reads, None), (reads, reads[::-1])], [(1000, "found"), (667, "found"), (600, "found"), (600, "valid"), (1, "found")])


def test_mates_vote_together(gpu):
    k = 4
    index = ["ACGTTGCA", "GGATCCTA"]
    masks = [0b011] * 5 + [0b110] * 5
    want = PA.Aligner(index, masks, 3, k).align(index[:1], index[1:])
    assert want["masks"] == [0b010] and PA.Aligner(index, masks, 3, k).align(index)["masks"] == [0b011, 0b110]
    _check(index, masks, 3, k, [(index[:1], index[1:]), (index, None), (index, index[::-1])], [(1000, "found"), (500, "found")])
    with api.KmerIndex(index, k, colors=masks, n_colors=3) as ix, api.Pseudoaligner(ix) as a:
        with pytest.raises(ValueError):
            a.align(index, index[:1])
        assert a.totals["fragments"] == 0
        for store_mates in (False, True):  # the store entry point
            reads_store = api.read_sequences(_fasta(index[:1]))
            r = a.align(reads_store, api.read_sequences(_fasta(index[1:])) if store_mates else index[1:])
            assert r.masks.tolist() == [0b010]


_TMP = []


def _fasta(seqs):
    import tempfile

    f = tempfile.NamedTemporaryFile("w", suffix=".fa", delete=False)
    f.write("".join(f">s{i}\n{s}\n" for i, s in enumerate(seqs)))
    f.close()
    _TMP.append(f.name)
    return f.name


def teardown_module(module):
    import os

    for name in _TMP:
        os.unlink(name)


def test_min_kmers_around_the_denominator(gpu):
    k = 7
    rng = random.Random(7)
    text = _dna(rng, 60)
    masks = [0b1] * (len(text) - k + 1)
    reads = [text[:20], text[5:30] + "N" + text[31:50], _dna(rng, 30)]
    ref = PA.Aligner([text], masks, 1, k).align(reads)
    for over in ("found", "valid"):
        denoms = sorted({d + e for d in ref[over] for e in (-1, 0, 1) if d + e >= 1})
        _check([text], masks, 1, k, [(reads, None)], [(1000, over), (1, over)], min_kmers=denoms)


def test_the_dictionary(gpu):
    """4 096 fragments with 4 096 distinct masks (C = 12; the mask 0 is no class), then all equal, then two alternating lane by lane;
    accumulation over three calls, `first` across calls, reset, two aligners on one index."""
    k, C, n = 8, 12, 4096
    rng = random.Random(4096)
    kmers = set()
    while len(kmers) < n:
        kmers.add(synth.canonical(_dna(rng, k)))
    kmers = sorted(kmers)
    rng.shuffle(kmers)
    for name, masks in (("distinct", list(range(n))), ("equal", [5] * n), ("alternating", [5 if i % 2 == 0 else 9 for i in range(n)])):
        want_classes = {}
        for i, m in enumerate(masks):
            if m:
                want_classes.setdefault(m, [0, i])[0] += 1
        order = sorted(want_classes, key=lambda m: want_classes[m][1])
        for kind, make in _kinds(kmers, masks, C, k)[:2]:
            with make() as ix, api.Pseudoaligner(ix) as a, api.Pseudoaligner(ix, 1) as other:
                r = a.align(kmers)
                assert r.masks.tolist() == masks and r.found.tolist() == [1] * n, (name, kind)
                cl = a.classes()
                assert cl["mask"].tolist() == order and cl["fragments"].tolist() == [want_classes[m][0] for m in order], (name, kind)
                assert cl["first"].tolist() == [want_classes[m][1] for m in order] and cl["carriers"].tolist() == [bin(m).count("1") for m in order]
                assert a.totals == {"fragments": n, "eligible": n, "assigned": n - masks.count(0),
                                    "ambiguous": sum(bin(m).count("1") > 1 for m in masks)}
                assert other.totals["fragments"] == 0 and len(other.classes()["mask"]) == 0  # independent
                # two more calls: a reversed slice, then everything again; `first` keeps running
                a.align(kmers[100:300][::-1])
                a.align(kmers)
                cl = a.classes()
                extra = {}
                for m in masks[100:300]:
                    extra[m] = extra.get(m, 0) + 1
                assert cl["mask"].tolist() == order and cl["first"].tolist() == [want_classes[m][1] for m in order]
                assert cl["fragments"].tolist() == [2 * want_classes[m][0] + extra.get(m, 0) for m in order], (name, kind)
                assert a.totals["fragments"] == 2 * n + 200
                other.align(kmers[7:9])
                assert other.classes()["first"].tolist() == ([0, 1] if masks[7] != masks[8] else [0]) and a.totals["fragments"] == 2 * n + 200
                a.reset()
                assert a.totals == dict.fromkeys(("fragments", "eligible", "assigned", "ambiguous"), 0) and len(a.classes()["mask"]) == 0
                r = a.align(kmers[7:9][::-1])
                assert a.classes()["first"].tolist()[0] == 0 and a.classes()["mask"].tolist()[0] == masks[8]


def test_the_index_answers_color_hits_as_before(gpu):
    k = 9
    rng = random.Random(9)
    index, masks, reads, mates, _ = _random_case(rng, k, 5)
    for name, make in _kinds(index, masks, 5, k)[:2]:
        with make() as ix:
            before = ix.color_hits(reads, per_window=True)
            with api.Pseudoaligner(ix, 500) as a:
                first = a.align(reads, mates)
                after = ix.color_hits(reads, per_window=True)
                api.release_device_memory(0)
                again = a.align(reads, mates)
                late = ix.color_hits(reads, per_window=True)
            for r in (after, late):
                for f in ("kmers", "valid", "found", "per_color", "per_window"):
                    assert np.array_equal(getattr(r, f), getattr(before, f)), (name, f)
            assert np.array_equal(first.masks, again.masks)
            # the parent's way to the same masks: the downloaded counters and the rule in numpy
            single = a_masks = None
            with api.Pseudoaligner(ix, 500) as a:
                a_masks = a.align(reads).masks
            hits, denom = before.per_color.astype(np.uint64), before.found
            on = (hits > 0) & (hits * np.uint64(1000) >= np.uint64(500) * denom[:, None]) & (denom[:, None] >= 1)
            single = (on.astype(np.uint64) << np.arange(5, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint64)
            assert np.array_equal(a_masks, single), name


def _fastq(path, records, qualities):
    path.write_text("".join(f"@{name} extra\n{s}\n+\n{q}\n" for (name, s), q in zip(records, qualities)))


def test_through_the_product(gpu, tmp_path):
    """Three --seq-in files as colours, two samples, one of them paired FASTQ with a quality threshold: the table and the minimizer
    index write the same three files, they are the restatement's, the masks follow from --query-colors-out of the same run, the other
    outputs do not notice the new flags, and mates of another count end the run with 2."""
    k, Q = 15, 20
    rng = random.Random(33)
    base = _dna(rng, 1500)
    haps = [base, base[:700] + _dna(rng, 100) + base[800:], base[:300] + _dna(rng, 200) + base[500:]]
    seq_in = []
    for i, h in enumerate(haps):
        seq_in.append(tmp_path / f"hap{i}.fa")
        seq_in[-1].write_text(f">h{i}a\n{h[:800]}\n>h{i}b\n{h[790:]}\n")
    records = [h[:800] for h in haps] + [h[790:] for h in haps]
    record_colors = [0, 1, 2, 0, 1, 2]

    def piece():
        h = rng.choice(haps)
        at = rng.randrange(len(h) - 80)
        s = h[at:at + rng.randint(10, 80)]
        s = synth.revcomp(s) if rng.random() < 0.5 else s
        return s if rng.random() < 0.7 else s[:len(s) // 2] + rng.choice("NACGT") + s[len(s) // 2 + 1:]

    single = [(f"s{i}", piece()) for i in range(40)] + [("short", "ACGT"), ("foreign", _dna(rng, 60))]
    r1 = [(f"p{i}/1", piece()) for i in range(30)]
    r2 = [(f"p{i}/2", piece()) for i in range(30)]
    quals = [["".join(chr(33 + (rng.choice([2, 40]) if rng.random() < 0.03 else 40)) for _ in s) for _, s in rs] for rs in (r1, r2)]
    s_fa, r1_fq, r2_fq = tmp_path / "single.fa", tmp_path / "r1.fq", tmp_path / "r2.fq"
    s_fa.write_text("".join(f">{n} x\n{s}\n" for n, s in single))
    _fastq(r1_fq, r1, quals[0])
    _fastq(r2_fq, r2, quals[1])
    masked = [["".join(c if ord(q) - 33 >= Q else "N" for c, q in zip(s, qs)) for (_, s), qs in zip(rs, qq)] for rs, qq in ((r1, quals[0]), (r2, quals[1]))]
    assert any("N" in s and "N" not in raw for s, (_, raw) in zip(masked[0] + masked[1], r1 + r2))

    t = lambda name: str(tmp_path / name)
    common = [sys.executable, "-m", "matchtigs_amd", *(x for p in seq_in for x in ("--seq-in", str(p))), "-k", str(k)]
    shared = lambda tag: ["--unitigs-fa-out", t(tag + ".u.fa"), "--query-fa", str(s_fa), "--query-out", t(tag + ".q.tsv"), "--query-colors-out", t(tag + ".qc.tsv")]

    def run(tag, *extra, status=0):
        r = subprocess.run(common + shared(tag) + list(extra), capture_output=True, text=True, cwd=str(ROOT), timeout=600)
        assert r.returncode == status, (tag, r.returncode, r.stderr[-2000:])
        return r.stderr

    def align_flags(tag, *more):
        return ["--pseudoalign-fa", str(s_fa), "--pseudoalign-fa", str(r1_fq), "--pseudoalign-mate-fa", str(s_fa), "--pseudoalign-mate-fa", str(r2_fq),
                "--pseudoalign-out", t(tag + ".pa.tsv"), "--pseudoalign-classes-out", t(tag + ".ec.tsv.gz"), "--pseudoalign-summary-out", t(tag + ".sum.tsv"),
                "--pseudoalign-min-base-quality", str(Q), *more]

    def read(path):
        raw = Path(path).read_bytes()
        return (gzip.decompress(raw) if str(path).endswith(".gz") else raw).decode()

    # (sample 0 is paired with itself: its mates are its reads, so every count doubles and the masks stay)
    err = run("table", *align_flags("table"))
    run("sparse", *align_flags("sparse", "--pseudoalign-index", "minimizer", "--pseudoalign-minimizer-length", "9"))
    run("plain")
    outs = [read(t("table" + x)) for x in (".pa.tsv", ".ec.tsv.gz", ".sum.tsv")]
    assert outs == [read(t("sparse" + x)) for x in (".pa.tsv", ".ec.tsv.gz", ".sum.tsv")]
    for x in (".u.fa", ".q.tsv", ".qc.tsv"):  # the other outputs do not notice the new flags
        assert read(t("table" + x)) == read(t("plain" + x)) == read(t("sparse" + x)), x
    assert err.count("Indexing the input for the pseudoalignment: ") == 1 and err.count("Pseudoaligning ") == 2

    # the restatement
    masks = PA.masks_by_record(records, record_colors, k)
    ref = PA.Aligner(records, masks, 3, k)
    names = [str(p) for p in seq_in]
    lines, class_lines, columns, totals = ["record\tkmers\tvalid\tfound\tcolors"], ["sample\tclass\tmask\tcarriers\tfragments"], [], []
    for sample, who, reads, mates in ((str(s_fa), [n for n, _ in single], [s for _, s in single], [s for _, s in single]),
                                      (str(r1_fq), [n for n, _ in r1], masked[0], masked[1])):
        lines += PA.out_lines(who, ref.align(reads, mates))[1:]
        class_lines += PA.class_lines(sample, ref.classes())
        columns += list(ref.color_reads())
        totals.append(dict(ref.totals))
        ref.reset()
    assert outs[0].splitlines() == lines
    assert outs[1].splitlines() == class_lines
    summary = ["\t".join(["color"] + [f"{s}:{w}" for s in (str(s_fa), str(r1_fq)) for w in ("assigned", "unique")])]
    summary += ["\t".join([names[c]] + [str(col[c]) for col in columns]) for c in range(3)]
    summary += ["\t".join([f"#{w}"] + [x for tot in totals for x in (str(tot[w]), "-")]) for w in ("fragments", "eligible", "assigned", "ambiguous")]
    assert outs[2].splitlines() == summary
    assert len(class_lines) > 3 and any(line.endswith("\t-") for line in lines) and totals[1]["ambiguous"] > 0

    # the masks of sample 0 from --query-colors-out of the same run: at the default threshold a colour is assigned iff it carries
    # every found k-mer (the pair with itself doubles both sides)
    derived = []
    for row in read(t("table.qc.tsv")).splitlines()[1:]:
        f = row.split("\t")
        found, per_color = int(f[3]), [int(x) for x in f[4:]]
        derived.append(",".join(str(c) for c in range(3) if found and per_color[c] == found) or "-")
    assert [line.split("\t")[4] for line in lines[1:1 + len(single)]] == derived

    # mates of another count: exit status 2, both files and both counts named, in a child process
    r = subprocess.run(common + ["--pseudoalign-fa", str(r1_fq), "--pseudoalign-mate-fa", str(s_fa), "--pseudoalign-out", t("bad.tsv")],
                       capture_output=True, text=True, cwd=str(ROOT), timeout=600)
    last = r.stderr.strip().splitlines()[-1]
    assert r.returncode == 2 and str(r1_fq) in last and str(s_fa) in last and "30" in last and "42" in last, (r.returncode, r.stderr[-1500:])
