"""Abundances and colours from the sparse minimizer index on the GPU (tig_payload_device.hpp, api.TigIndex.annotated):
every field as exact integers against the two arbiters (kmer_abundance_ref.abundance, kmer_color_ref.color_hits, which know nothing about
positions or layouts), per_window included, and on the larger case field for field against the annotated api.KmerIndex. Random pairs
over k, m, bucket_limit and both layouts, the shapes and widths of a payload, the layout rule and the memory equalities, the palindromes
with a different weight on either occurrence, awkward inputs, reuse of one index, and the path through the product."""
import gzip
import random
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import kmer_abundance_ref as KA
import kmer_color_ref as KC
import tig_index_cases as cases
import tig_locate_ref as TL
import tig_payload_ref as TP
from matchtigs_amd import api, synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
KS = [1, 2, 3, 5, 16, 31, 32, 33, 64, 101]
PAIRS = 8  # (test_tig_payload_ref.py checks that these pairs, from these seeds, show every hazard at every k)


@pytest.fixture(scope="module")
def gpu(product_lib):
    import torch

    if product_lib.mtg_device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("these tests need a GPU: the tig index has no CPU path")
    return torch


def _check_abundance(ix, query, want, what=""):
    got = ix.abundance(query, per_window=True)
    assert (got.sum.dtype, got.min.dtype, got.max.dtype, got.per_window.dtype) == (np.uint64, np.uint32, np.uint32, np.uint32)
    for f in ("kmers", "valid", "found", "sum", "min", "max", "per_window"):
        g = getattr(got, f).tolist()
        assert g == want[f], (what, ix.info, ix.payload_info, f, g[:40], want[f][:40])
    bare = ix.abundance(query)
    assert bare.per_window is None and all(getattr(bare, f).tolist() == want[f] for f in ("kmers", "valid", "found", "sum", "min", "max")), what


def _check_colors(ix, query, want, what=""):
    got = ix.color_hits(query, per_window=True)
    assert (got.per_color.dtype, got.per_window.dtype) == (np.uint32, np.uint64) and got.per_color.shape == (len(query), ix.n_colors)
    for f in ("kmers", "valid", "found", "per_color", "per_window"):
        g = getattr(got, f).tolist()
        assert g == want[f], (what, ix.info, ix.payload_info, f, g[:40], want[f][:40])
    assert ix.color_hits(query).per_color.tolist() == want["per_color"], what


def _check_both(index, query, k, weights, masks, n_colors, m=None, limit=None, layouts=("dense", "runs"), what="", wants=None):
    want_a, want_c = wants or (KA.abundance(index, weights, query, k), KC.color_hits(index, masks, n_colors, query, k))
    info = None
    for layout in layouts:
        with api.TigIndex.annotated(index, k, m, bucket_limit=limit, weights=weights, colors=masks, n_colors=n_colors, payload_layout=layout) as ix:
            assert ix.weighted and ix.colored and ix.locating and ix.n_colors == n_colors
            if layout is not None:
                assert ix.payload_info["weights"]["layout"] == ix.payload_info["colors"]["layout"] == layout
            _check_abundance(ix, query, want_a, (what, layout))
            _check_colors(ix, query, want_c, (what, layout))
            info = ix.info
    return info


@pytest.mark.parametrize("k", KS)
def test_random_pairs(gpu, k):
    rng = random.Random(3140 + k)
    seen = dict.fromkeys(TP.SEEN + ("heavy", "light"), False)
    for i in range(PAIRS):
        index, query, weights, masks, n_colors = TP.payload_pair(rng, k)
        wants = KA.abundance(index, weights, query, k), KC.color_hits(index, masks, n_colors, query, k)
        for f, v in TP.seen_flags(index, weights, query, k).items():
            seen[f] |= v
        for m in cases.random_ms(k):
            for limit in (None, 1, 2):
                info = _check_both(index, query, k, weights, masks, n_colors, m, limit, what=f"pair {i} m={m} limit={limit}", wants=wants)
                seen["heavy"] |= info.heavy_windows > 0
                seen["light"] |= info.heavy_windows < info.occurrences
    assert all(seen.values()), (k, seen)


def _expected_info(values, kind, n_colors=None, layout=None):
    return TP.Payload(values, kind, n_colors, layout).info()


def test_payload_shapes(gpu):
    """All-equal values (one run), strictly alternating ones (R = W), R in {1, 2, 3, 7, 8, 9}, records shorter than k between the
    others, a run that crosses a record border, the last ordinal; every window is asked, on both strands."""
    k = 5
    rng = random.Random(31)
    index = [cases.dna(rng, 40), "ACG", cases.dna(rng, 9), "", cases.dna(rng, 5), "AC", cases.dna(rng, 33)]
    W = len(KA.windows(index, k))
    assert W == 36 + 5 + 1 + 29
    query = index + [synth.revcomp(s) for s in index] + ["".join(index)]
    shapes = {"all equal": [7] * W, "alternating": [1 + (i & 1) for i in range(W)], "last ordinal": [3] * (W - 1) + [9],
              "across the border": [1] * 30 + [2] * 8 + [3] * (W - 38)}  # (record 0 ends at ordinal 35: the run of 2s, 30 .. 37, crosses into record 2)
    for R in (1, 2, 3, 7, 8, 9):
        cut = sorted(rng.sample(range(1, W), R - 1))
        shapes[f"R={R}"] = [j for j, (a, b) in enumerate(zip([0] + cut, cut + [W])) for _ in range(b - a)]
    for name, values in shapes.items():
        masks = [v % 8 for v in values]
        for layout in ("dense", "runs", None):
            with api.TigIndex.annotated(index, k, weights=values, colors=masks, n_colors=3, payload_layout=layout) as ix:
                assert ix.payload_info["weights"] == _expected_info(values, "weights", layout=layout), (name, layout)
                assert ix.payload_info["colors"] == _expected_info(masks, "colors", 3, layout), (name, layout)
                _check_abundance(ix, query, KA.abundance(index, values, query, k), name)
                _check_colors(ix, query, KC.color_hits(index, masks, 3, query, k), name)
    assert TP.Payload(shapes["R=9"]).runs == 9 and TP.Payload(shapes["alternating"]).runs == W


@pytest.mark.parametrize("top", [255, 256, 65535, 65536, (1 << 32) - 1])
def test_weight_widths_and_sums_beyond_32_bits(gpu, top):
    k = 4
    rng = random.Random(top)
    s = cases.dna(rng, 200)
    W = len(s) - k + 1
    weights = [top if i % 3 else rng.randint(0, top) for i in range(W)]
    query = [s, synth.revcomp(s), s[:50]]
    want = KA.abundance([s], weights, query, k)
    assert top < 1 << 32 and (top < (1 << 32) - 1 or max(want["sum"]) > 1 << 32)  # several windows of 2^32 - 1 in one record
    for layout in ("dense", "runs"):
        with api.TigIndex.annotated([s], k, weights=weights, payload_layout=layout) as ix:
            assert ix.payload_info["weights"]["width"] == (1 if top < 256 else 2 if top < 65536 else 4)
            assert ix.weighted and not ix.colored and ix.n_colors == 0 and "colors" not in ix.payload_info
            _check_abundance(ix, query, want, (top, layout))
            with pytest.raises(ValueError):
                ix.color_hits(query)


@pytest.mark.parametrize("n_colors", [1, 8, 9, 16, 17, 32, 33, 64])
def test_mask_widths_and_the_empty_mask(gpu, n_colors):
    """The top bit set, and a mask of 0: found, and it touches no column."""
    k = 6
    rng = random.Random(n_colors)
    s = cases.dna(rng, 150)
    W = len(s) - k + 1
    full = (1 << n_colors) - 1
    masks = [(0, 1 << (n_colors - 1), full, rng.randint(0, full))[(i // 3) % 4] for i in range(W)]
    query = [s, synth.revcomp(s)[:80], "N" + s[:30]]
    want = KC.color_hits([s], masks, n_colors, query, k)
    assert want["found"][0] == W and want["per_color"][0][n_colors - 1] > 0 and sum(1 for x in masks if x == 0) > 0
    for layout in ("dense", "runs"):
        with api.TigIndex.annotated([s], k, colors=masks, n_colors=n_colors, payload_layout=layout) as ix:
            assert ix.payload_info["colors"]["width"] == TP.mask_width(n_colors)
            assert ix.colored and not ix.weighted and "weights" not in ix.payload_info
            _check_colors(ix, query, want, (n_colors, layout))
            with pytest.raises(ValueError):
                ix.abundance(query)


def test_auto_layout_and_the_memory_equalities(gpu):
    """Constant weights choose runs, alternating ones dense, a tie goes to dense; info.device_bytes == L + 8 (records + 1) + the payloads,
    L the locating index without payloads over the same text."""
    k = 9
    rng = random.Random(17)
    index = [cases.dna(rng, 300), cases.dna(rng, 4), cases.dna(rng, 120)]
    W = len(KA.windows(index, k))
    with api.TigIndex(index, k, locate=True) as plain:
        L = plain.info.device_bytes
        assert plain.payload_info == {} and not plain.weighted and not plain.colored
    tie_w = [70000] * 3 + [1] * 3  # 2 runs * 12 B == 6 windows * 4 B
    cases_ = [("constant", index, [5] * W, [3] * W, ("runs", "runs")), ("alternating", index, [1 + (i & 1) for i in range(W)], [i & 1 for i in range(W)], ("dense", "dense")),
              ("mixed", index, [5] * W, [i & 1 for i in range(W)], ("runs", "dense"))]
    for name, idx, weights, masks, layouts in cases_:
        with api.TigIndex.annotated(idx, k, weights=weights, colors=masks, n_colors=2) as ix:
            pw, pc = ix.payload_info["weights"], ix.payload_info["colors"]
            assert (pw["layout"], pc["layout"]) == layouts, name
            assert pw == _expected_info(weights, "weights") and pc == _expected_info(masks, "colors", 2), name
            assert pw["device_bytes"] == (12 * pw["runs"] if pw["layout"] == "runs" else pw["width"] * W)
            assert pc["device_bytes"] == (16 * pc["runs"] if pc["layout"] == "runs" else pc["width"] * W)
            assert ix.info.device_bytes == L + 8 * (len(idx) + 1) + pw["device_bytes"] + pc["device_bytes"], name
            assert {f: v for f, v in ix.info.__dict__.items() if f != "device_bytes"} == {f: v for f, v in plain.info.__dict__.items() if f != "device_bytes"}
    s = cases.dna(rng, 6 + k - 1)
    with api.TigIndex.annotated([s], k, weights=tie_w) as ix, api.TigIndex([s], k, locate=True) as bare:
        assert ix.payload_info["weights"] == {"layout": "dense", "width": 4, "windows": 6, "runs": 2, "device_bytes": 24}
        assert ix.info.device_bytes == bare.info.device_bytes + 16 + 24
        _check_abundance(ix, [s], KA.abundance([s], tie_w, [s], k), "tie")
    with api.TigIndex.annotated([s], k) as ix, api.TigIndex([s], k, locate=True) as bare:  # neither payload: a locating index
        assert ix.info == bare.info and ix.locating and ix.payload_info == {}
    t = api.last_tig_payload_times()
    assert set(t) == {"weights", "colors", "upload_ms", "pack_ms", "probe_ms", "gather_ms"} and set(t["weights"]) == {"upload_ms", "reduce_ms", "flag_scan_ms", "store_ms"}


@pytest.mark.parametrize("k,m", [(31, 19), (33, 19), (5, 2), (12, 4)])
def test_palindromes_with_differing_weights(gpu, k, m):
    """The two occurrences of a class inside a reverse-complement palindrome carry different weights: a gather at the first passing
    candidate's position instead of the smallest one reports the wrong weight."""
    rng = random.Random(100 * k + m)
    text, hard = TL.palindrome_case(rng, k, m)
    ref = TL.TigLocateRef([text], k, m)
    weights, pairs = TP.palindrome_weights(ref, text, hard)
    assert any(a != b for a, b in pairs)
    masks = [w % 7 for w in weights]
    query = [text, synth.revcomp(text)] + hard + [synth.revcomp(x) for x in hard]
    for limit in (None, 1):
        _check_both([text], query, k, weights, masks, 3, m, limit, what=f"palindrome limit={limit}")


def test_awkward_inputs(gpu):
    """tig_index_cases.engineered() with payloads (empty indexes and queries, records shorter than k, record borders), then junk bytes,
    flipped case, empty records and a query without a valid window."""
    rng = random.Random(71)
    for name, index, query, k, m, limit in cases.engineered():
        W = len(KA.windows(index, k))
        weights, masks = TP.runny(rng, W, [0, 1, 300, 70000]), TP.runny(rng, W, [0, 1, 2, 3])
        _check_both(index, query, k, weights, masks, 2, m, limit, layouts=(rng.choice(("dense", "runs")), None), what=name)
    s = cases.dna(rng, 300)
    junk = list(cases.flip_case(rng, s))
    for at in (0, 63, 64, 65, 150, 299):
        junk[at] = rng.choice(cases.JUNK)
    index = [s[:100], "", s[100:]]
    W = len(KA.windows(index, 21))
    query = ["".join(junk), synth.revcomp(s).lower(), cases.flip_case(rng, s), "", "N" * 100, cases.JUNK * 3, "ACGT"]
    _check_both(index, query, 21, TP.runny(rng, W, [1, 2, 500]), TP.runny(rng, W, [1, 2, 4, 7]), 3, what="junk and case")


def test_reuse_and_interference(gpu):
    rng = random.Random(9)
    genome = cases.dna(rng, 3000)
    a = [genome[i:i + 400] for i in range(0, 2700, 300)]  # neighbouring records share 100 bases: repeats with other payloads
    b = [synth.revcomp(genome[1000:2500]), cases.dna(rng, 500), "A" * 200]
    queries = [[genome[100:900], cases.dna(rng, 300), "ACGTN" * 50], [synth.revcomp(genome)[:-1] + "N", ""],
               [cases.dna(rng, 70)] * 5 + [genome[2000:2100].lower(), "a" * 100]]
    ka, kb = 21, 45
    wa, ca = TP.runny(rng, len(KA.windows(a, ka)), [1, 2, 3, 1000], 40), TP.runny(rng, len(KA.windows(a, ka)), [1, 2, 3], 40)
    wb, cb = TP.runny(rng, len(KA.windows(b, kb)), [5, 6], 9), TP.runny(rng, len(KA.windows(b, kb)), [0, 1 << 63], 9)
    ia = api.TigIndex.annotated(a, ka, weights=wa, colors=ca, n_colors=2)
    live = api.device_arena_stats(0)["live_bytes"]
    first = [(ia.abundance(q, per_window=True), ia.color_hits(q, per_window=True)) for q in queries]
    assert api.device_arena_stats(0)["live_bytes"] == live  # a call gives back what it took
    for q, (x, y) in zip(queries, first):
        _check_abundance(ia, q, KA.abundance(a, wa, q, ka), "first")
        _check_colors(ia, q, KC.color_hits(a, ca, 2, q, ka), "first")
    ib = api.TigIndex.annotated(b, kb, 15, weights=wb, colors=cb, n_colors=64)  # a second index, of another k, with a heavy bucket
    assert ib.info.heavy_buckets >= 1 and ia.info.heavy_buckets == 0

    def same(q, x, y):
        x2, y2 = ia.abundance(q, per_window=True), ia.color_hits(q, per_window=True)
        for f in ("kmers", "valid", "found", "sum", "min", "max", "per_window"):
            assert np.array_equal(getattr(x, f), getattr(x2, f)), f
        for f in ("kmers", "valid", "found", "per_color", "per_window"):
            assert np.array_equal(getattr(y, f), getattr(y2, f)), f

    for q, (x, y) in zip(queries, first):
        same(q, x, y)
        _check_abundance(ib, q, KA.abundance(b, wb, q, kb), "second index")
        _check_colors(ib, q, KC.color_hits(b, cb, 64, q, kb), "second index")
    api.release_device_memory(0)
    for q, (x, y) in zip(queries, first):
        same(q, x, y)
    with api.TigIndex(a, ka, locate=True) as plain:  # membership and locate do not see the payloads
        for q in queries:
            x, y = ia.query(q, bits=True), plain.query(q, bits=True)
            for f in ("kmers", "valid", "found", "valid_bits", "present_bits"):
                assert getattr(x, f).tobytes() == getattr(y, f).tobytes(), f
            x, y = ia.locate(q), plain.locate(q)
            for f in ("kmers", "valid", "found", "runs"):
                assert np.array_equal(getattr(x, f), getattr(y, f)), f
        with pytest.raises(ValueError) as e:
            plain.abundance(queries[0])
        assert str(e.value) == "abundance() needs an index built with weights"
    t = api.last_tig_payload_times()
    assert all(t[f] >= 0 for f in ("upload_ms", "pack_ms")) and t["probe_ms"] > 0 and t["gather_ms"] > 0
    ia.close()
    for call in (ia.abundance, ia.color_hits):
        with pytest.raises(ValueError) as e:
            call(queries[0])
        assert str(e.value) == "the index is closed"
    _check_abundance(ib, queries[0], KA.abundance(b, wb, queries[0], kb), "after the other closed")
    ib.close()


COMP = np.zeros(256, np.uint8)
for _a, _b in zip("ACGTN", "TGCAN"):
    COMP[ord(_a)] = ord(_b)


def test_size_against_the_table(gpu):
    """A random genome of 2 * 10^5 bases with 300 reverse-complemented pieces of it as further records (test_gpu_tig_locate.py's size
    case): every piece's class twice, with different payloads; both layouts return the annotated table's arrays, field for field."""
    k, m = 31, 19
    rng = np.random.default_rng(31)
    genome = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 200_000)]
    pieces = [genome]
    for _ in range(300):
        at, n = int(rng.integers(0, 199_000)), int(rng.integers(1, 1000))
        pieces.append(COMP[genome[at:at + n][::-1]])
    seq = np.concatenate(pieces)
    off = np.zeros(len(pieces) + 1, np.uint64)
    off[1:] = np.cumsum([len(p) for p in pieces])
    W = int(np.maximum(np.diff(off.astype(np.int64)) - (k - 1), 0).sum())
    weights = np.repeat(rng.integers(0, 1 << 32, W // 20 + 1, dtype=np.uint64), 20)[:W].astype(np.uint32)
    masks = np.repeat(rng.integers(0, 1 << 40, W // 50 + 1, dtype=np.uint64), 50)[:W]
    cuts = np.sort(rng.integers(0, len(seq), 2000))
    q_pieces = [seq[a:b] if rng.random() < 0.5 else COMP[seq[a:b][::-1]] for a, b in zip(np.r_[0, cuts], np.r_[cuts, len(seq)])]
    q_seq = np.concatenate(q_pieces)
    q_off = np.zeros(len(q_pieces) + 1, np.uint64)
    q_off[1:] = np.cumsum([len(p) for p in q_pieces])
    sub = rng.random(len(q_seq)) < 0.03
    q_seq[sub] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(sub.sum()))]
    q_seq[rng.random(len(q_seq)) < 1e-3] = ord("N")
    with api.KmerIndex((seq, off), k, weights=weights, colors=masks, n_colors=40) as table:
        want_a, want_c = table.abundance((q_seq, q_off), per_window=True), table.color_hits((q_seq, q_off), per_window=True)
        table_bytes = table.info.device_bytes
    assert 50_000 < int(want_a.found.sum()) < int(want_a.valid.sum()) and int(want_a.sum.max()) > 1 << 32
    for layout in ("dense", "runs", None):
        with api.TigIndex.annotated((seq, off), k, m, weights=weights, colors=masks, n_colors=40, payload_layout=layout) as ix:
            got_a, got_c = ix.abundance((q_seq, q_off), per_window=True), ix.color_hits((q_seq, q_off), per_window=True)
            for f in ("offsets", "kmers", "valid", "found", "sum", "min", "max", "per_window"):
                assert np.array_equal(getattr(got_a, f), getattr(want_a, f)), (layout, f)
            for f in ("offsets", "kmers", "valid", "found", "per_color", "per_window"):
                assert np.array_equal(getattr(got_c, f), getattr(want_c, f)), (layout, f)
            if layout is None:  # runs of 20 and 50 windows: 12 B / 20 < 4 B and 16 B / 50 < 8 B
                assert ix.payload_info["weights"]["layout"] == ix.payload_info["colors"]["layout"] == "runs"
                assert ix.info.device_bytes < table_bytes // 4


def test_through_the_product(gpu, tmp_path):
    """The 20 kb two-haplotype genome with reads: the three new files over the input, over the greedy tigs (gzipped) and over the Euler
    tigs are byte for byte the table run's --query-abundance-out, profile and --query-colors-out; --query-out never changes; with
    --query-index-locate-out alongside that file equals a run without the new flags."""
    k = 21
    rng = random.Random(31)
    haps = synth.random_genome(10_000, seed=31, haplotypes=2)
    reads = [[], []]
    for i in range(160):
        h = i % 2
        at = rng.randrange(0, len(haps[h]) - 300)
        s = list(haps[h][at:at + rng.randint(60, 300)])
        for j in range(len(s)):
            if rng.random() < 0.005:
                s[j] = rng.choice("ACGT")
        s = "".join(s)
        reads[h].append(synth.revcomp(s) if rng.random() < 0.5 else s)
    query = []
    for i in range(24):
        h = rng.choice(haps)
        at = rng.randrange(0, len(h) - 400)
        s = h[at:at + rng.randint(30, 400)]
        s = list(synth.revcomp(s) if rng.random() < 0.5 else s)
        for j in range(len(s)):
            if rng.random() < 0.01:
                s[j] = rng.choice("ACGTNn")
        query.append("".join(s))
    query += ["ACGT", cases.dna(rng, 100)]
    fas = []
    for h in (0, 1):
        fas.append(tmp_path / f"reads{h}.fa")
        fas[-1].write_text("".join(f">r{h}_{i}\n{s}\n" for i, s in enumerate(reads[h])))
    q_fa = tmp_path / "q.fa"
    q_fa.write_text("".join(f">q{i}\n{s}\n" for i, s in enumerate(query)))

    def run(tag, *extra):
        out = {x: tmp_path / f"{tag}.{x}" for x in ("tsv", "g.fa", "e.fa")}
        r = subprocess.run([sys.executable, "-m", "matchtigs_amd", "--seq-in", str(fas[0]), "--seq-in", str(fas[1]), "-k", str(k),
                            "--greedytigs-fa-out", str(out["g.fa"]), "--eulertigs-fa-out", str(out["e.fa"]), "--query-fa", str(q_fa),
                            "--query-out", str(out["tsv"]), *extra], capture_output=True, text=True, cwd=str(ROOT), timeout=600)
        assert r.returncode == 0, (tag, r.stderr[-2000:])
        return out, r.stderr

    def read(path):
        raw = Path(path).read_bytes()
        return gzip.decompress(raw) if str(path).endswith(".gz") else raw

    t = lambda name: str(tmp_path / name)
    table, _ = run("table", "--query-abundance-out", t("table.ab"), "--query-abundance-profile-out", t("table.pr"), "--query-colors-out", t("table.co"))
    want = [read(t("table.ab")), read(t("table.pr")), read(t("table.co"))]
    assert want[0].count(b"\n") == len(query) + 1 and want[2].count(b"\n") == len(query) + 1 and b"\t0\t0\t0\t0\t0\t0\t-\n" in want[0]
    located, _ = run("located", "--query-index", "minimizer", "--query-index-locate-out", t("plain.loc"))
    for over, ab, pr, co in (("input", "i.ab", "i.pr", "i.co"), ("greedytigs", "g.ab.gz", "g.pr.gz", "g.co.gz"), ("eulertigs", "e.ab", "e.pr", "e.co")):
        out, err = run(over, "--query-index", "minimizer", "--query-index-over", over, "--query-index-abundance-out", t(ab),
                       "--query-index-abundance-profile-out", t(pr), "--query-index-colors-out", t(co))
        assert [read(t(ab)), read(t(pr)), read(t(co))] == want, over
        assert out["tsv"].read_bytes() == table["tsv"].read_bytes(), over
        assert "weights by position:" in err and "colors by position:" in err, err[-1500:]
    out, _ = run("both", "--query-index", "minimizer", "--query-index-abundance-out", t("b.ab"), "--query-index-colors-out", t("b.co"),
                 "--query-index-locate-out", t("b.loc"), "--query-presence-out", t("b.pres"))
    assert read(t("b.loc")) == read(t("plain.loc")) and [read(t("b.ab")), read(t("b.co"))] == [want[0], want[2]]
    assert out["tsv"].read_bytes() == table["tsv"].read_bytes() == located["tsv"].read_bytes()
