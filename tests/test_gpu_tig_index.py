"""The sparse minimizer index on the GPU (tig_index_device.hip, api.TigIndex): kmers / valid / found of every record and
both bit arrays as exact integers against the k-mer index's restatement (kmer_query_ref.py), the anchors and the heavy windows against
the scheme's restatement (tig_index_ref.py), and on the larger cases against api.KmerIndex on the same inputs. Random pairs over k, m
and bucket_limit (the small limits send most windows down the heavy path), the engineered hazards of tig_index_cases.py,
low-complexity repeats at the default limit, an N at every position of a record that spans several thread runs, reuse of one index,
one case large enough for many workgroups and real buckets with the derived memory bound, and the path through the product."""
import itertools
import random
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import kmer_query_ref as R
import tig_index_cases as cases
import tig_index_ref as T
from matchtigs_amd import api, synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
KS = [1, 2, 3, 5, 16, 31, 32, 33, 64, 101]
FIELDS = ("kmers", "valid", "found", "valid_bits", "present_bits")


@pytest.fixture(scope="module")
def gpu(product_lib):
    import torch

    if product_lib.mtg_device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("these tests need a GPU: the tig index has no CPU path")
    return torch


def _assert_equals_ref(index, want, seqs, k, what=""):
    """One query with the bit arrays and one without: every output equals the restatement's `want`."""
    got = index.query(seqs, bits=True)
    for f in FIELDS:
        g = getattr(got, f)
        assert g.dtype == np.uint64 and g.tolist() == want[f], (what, k, index.info, f, g.tolist()[:20], want[f][:20])
    assert got.offsets.tolist() == list(itertools.accumulate((len(s) for s in seqs), initial=0))
    for i in range(min(len(seqs), 6)):
        assert got.presence(i) == R.presence(want, seqs, i), (what, k, i)
    plain = index.query(seqs)
    assert plain.valid_bits is None and plain.present_bits is None
    for f in ("kmers", "valid", "found"):
        assert getattr(plain, f).tolist() == want[f], (what, k, f)


def _assert_info(info, index, k, m, limit, ref=None):
    assert (info.k, info.m, info.bucket_limit) == (k, T.default_m(k) if m is None else m, limit or 64)
    assert info.records == len(index) and info.characters == sum(map(len, index))
    assert info.occurrences == sum(max(0, len(s) - k + 1) for s in index)
    assert info.buckets >= max(8, info.anchors) and info.buckets & (info.buckets - 1) == 0
    assert (info.table_slots >= 2 * info.heavy_windows) and (info.heavy_buckets > 0) == (info.heavy_windows > 0) == (info.table_slots > 0)
    if ref is not None:
        assert (info.anchors, info.buckets, info.heavy_buckets, info.heavy_windows) == (ref.anchors, ref.buckets, len(ref.heavy), ref.heavy_windows)


@pytest.mark.parametrize("k", KS)
def test_random_pairs(gpu, k):
    rng = random.Random(2900 + k)
    seen = dict.fromkeys(("all", "some", "none", "invalid", "heavy", "light"), False)
    for i in range(12):
        index, query = cases.random_pair(rng, k)
        want = R.query(R.index_set(index, k), query, k)
        for m in cases.random_ms(k):
            for limit in (None, 1, 2):
                ref = T.TigIndexRef(index, k, m, limit or 64) if k <= 33 else None  # (the restatement's build is slow for long windows)
                with api.TigIndex(index, k, m, bucket_limit=limit) as ix:
                    _assert_info(ix.info, index, k, m, limit, ref)
                    _assert_equals_ref(ix, want, query, k, f"pair {i} m={m} limit={limit}")
                    seen["heavy"] |= ix.info.heavy_windows > 0
                    seen["light"] |= ix.info.heavy_windows < ix.info.occurrences
        for n, v, f in zip(want["kmers"], want["valid"], want["found"]):
            seen["all"] |= n > 0 and f == n
            seen["some"] |= 0 < f < n
            seen["none"] |= v > 0 and f == 0
            seen["invalid"] |= v < n
    assert all(seen.values()), (k, seen)


def test_engineered_cases(gpu):
    for name, index, query, k, m, limit in cases.engineered():
        want = R.query(R.index_set(index, k), query, k)
        for lim in (limit, 1):
            with api.TigIndex(index, k, m, bucket_limit=lim) as ix:
                _assert_info(ix.info, index, k, m, lim, T.TigIndexRef(index, k, m, lim or 64))
                _assert_equals_ref(ix, want, query, k, name)
        if name.startswith("record borders k="):  # only the concatenation, or the padding behind the text, spells these
            assert want["found"][:3 * (k - 1)] == [0] * (3 * (k - 1)) and want["valid"][:3 * (k - 1)] == [1] * (3 * (k - 1)), name
        if name.startswith("empty index"):
            assert ix.info.anchors == ix.info.occurrences == 0 and ix.info.buckets == 8 and not any(want["found"])


@pytest.mark.parametrize("k,m", [(31, None), (33, 12)])
def test_repeats_take_the_heavy_path(gpu, k, m):
    """Poly-A and (AC)^n of 5 000 bases beside random sequence at the default limit."""
    n = 5000
    index, query = cases.repeats_case(n, k)
    want = R.query(R.index_set(index, k), query, k)
    n_neighbours = len(cases.neighbours("A" * k)[::3]) + len(cases.neighbours(("AC" * k)[:k])[::3])
    assert want["found"][:6] == [1, 1, 1, 1, k + 1, k + 1] and want["found"][6:6 + n_neighbours] == [0] * n_neighbours
    ref = T.TigIndexRef(index, k, m, 64)
    with api.TigIndex(index, k, m) as ix, api.KmerIndex(index, k) as table:
        _assert_info(ix.info, index, k, m, None, ref)
        assert ix.info.heavy_buckets >= 1 and ix.info.heavy_windows >= 2 * (n - k + 1) - 2 and ix.info.anchors > 0
        _assert_equals_ref(ix, want, query, k, "repeats")
        other = table.query(query, bits=True)
        got = ix.query(query, bits=True)
        for f in FIELDS:
            assert np.array_equal(getattr(got, f), getattr(other, f)), f


@pytest.mark.parametrize("k,m,limit", [(5, 2, None), (31, None, None), (33, 31, None), (31, 19, 1)])
def test_n_at_every_position(gpu, k, m, limit):
    """A record of 64 * 3 + k bases, one copy per position with that position replaced by N, all copies in one call: the N costs exactly
    the windows that cover it, whichever run border it sits at -- the minimizer walk starts afresh behind it."""
    rng = random.Random(k)
    L = 3 * 64 + k
    s = cases.dna(rng, L)
    query = [s[:j] + "N" + s[j + 1:] for j in range(L)]
    want = R.query(R.index_set([s], k), query, k)
    with api.TigIndex([s], k, m, bucket_limit=limit) as ix:
        got = ix.query(query, bits=True)
    covering = [min(j, L - k) - max(0, j - k + 1) + 1 for j in range(L)]
    assert got.kmers.tolist() == [L - k + 1] * L
    assert got.valid.tolist() == [L - k + 1 - c for c in covering]
    assert got.found.tolist() == got.valid.tolist()
    for f in FIELDS:
        assert getattr(got, f).tolist() == want[f], (k, f)


def test_reuse_and_determinism(gpu):
    rng = random.Random(9)
    genome = cases.dna(rng, 3000)
    a = [genome[i:i + 400] for i in range(0, 2700, 300)]
    b = [synth.revcomp(genome[1000:2500]), cases.dna(rng, 500), "A" * 200]
    queries = [[genome[100:900], cases.dna(rng, 300), "ACGTN" * 50], [synth.revcomp(genome)[:-1] + "N", ""],
               [cases.dna(rng, 70)] * 5 + [genome[2000:2100].lower(), "a" * 100]]
    ka, kb = 21, 45
    want_a = [R.query(R.index_set(a, ka), q, ka) for q in queries]
    want_b = [R.query(R.index_set(b, kb), q, kb) for q in queries]
    ia, ib = api.TigIndex(a, ka), api.TigIndex(b, kb, 15)  # two indexes of different k alive at once
    assert ib.info.heavy_buckets >= 1 and ia.info.heavy_buckets == 0

    def check():
        for i, q in enumerate(queries):
            _assert_equals_ref(ia, want_a[i], q, ka)
            _assert_equals_ref(ib, want_b[i], q, kb)

    first = ia.query(queries[0], bits=True)
    check()
    again = ia.query(queries[0], bits=True)
    for f in FIELDS:
        assert np.array_equal(getattr(first, f), getattr(again, f)), f
    api.release_device_memory(0)
    other = api.TigIndex([cases.dna(rng, 5000)], 33)  # another index built and closed in between
    other.close()
    other.close()
    api.release_device_memory(0)
    check()
    twin_a, twin_b = api.TigIndex(a, ka), api.TigIndex(b, kb, 15)
    assert twin_a.info == ia.info and twin_b.info == ib.info  # two builds of one input
    ia.close()
    with pytest.raises(ValueError) as e:
        ia.query(queries[0])
    assert str(e.value) == "the index is closed"
    _assert_equals_ref(twin_a, want_a[0], queries[0], ka)
    _assert_equals_ref(ib, want_b[0], queries[0], kb)
    for ix in (ib, twin_a, twin_b):
        ix.close()
    t = api.last_tig_index_times()
    assert set(t) == {"build_upload_ms", "build_pack_ms", "build_anchors_ms", "build_directory_ms", "build_heavy_ms", "query_upload_ms",
                      "query_pack_ms", "query_probe_ms"}
    assert all(v >= 0 for v in t.values()) and t["query_probe_ms"] > 0 and t["build_anchors_ms"] > 0 and t["build_directory_ms"] > 0


COMP = np.zeros(256, np.uint8)
for _a, _b in zip("ACGTN", "TGCAN"):
    COMP[ord(_a)] = ord(_b)


def test_size_and_memory(gpu):
    """A random genome of 2 * 10^5 bases with reverse-complemented pieces of it: many workgroups, real buckets. The memory cap is derived:
    the table keeps 16 B per window; the sparse index 0.25 B per base, 8 B x 0.143 per window of anchors and at most 16 B x 0.143 of
    directory -- under 4 B per window, and the bound of half the table leaves a factor of two for offsets and rounding."""
    k, m = 31, 19
    rng = np.random.default_rng(28)
    genome = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 200_000)]
    pieces = [genome]
    for _ in range(300):
        at, n = int(rng.integers(0, 199_000)), int(rng.integers(1, 1000))
        pieces.append(COMP[genome[at:at + n][::-1]])
    seq = np.concatenate(pieces)
    off = np.zeros(len(pieces) + 1, np.uint64)
    off[1:] = np.cumsum([len(p) for p in pieces])
    # the query: the index cut at random, half of the pieces reverse-complemented, 3 % substitutions, an N every ~10^3 bases
    cuts = np.sort(rng.integers(0, len(seq), 2000))
    q_pieces = [seq[a:b] if rng.random() < 0.5 else COMP[seq[a:b][::-1]] for a, b in zip(np.r_[0, cuts], np.r_[cuts, len(seq)])]
    q_seq = np.concatenate(q_pieces)
    q_off = np.zeros(len(q_pieces) + 1, np.uint64)
    q_off[1:] = np.cumsum([len(p) for p in q_pieces])
    sub = rng.random(len(q_seq)) < 0.03
    q_seq[sub] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(sub.sum()))]
    q_seq[rng.random(len(q_seq)) < 1e-3] = ord("N")
    with api.TigIndex((seq, off), k, m) as ix, api.KmerIndex((seq, off), k) as table:
        info = ix.info
        assert info.anchors == T.anchor_count_arrays(seq, off, k, m) and info.heavy_buckets == info.heavy_windows == info.table_slots == 0
        assert abs(info.anchors / info.occurrences - 2 / (k - m + 2)) < 0.01
        assert info.occurrences == table.info.occurrences and info.device_bytes <= table.info.device_bytes // 2
        assert info.device_bytes == 4 * ((len(seq) + 15) // 16 + 2) + 8 * (len(pieces) + 1) + 8 * (info.buckets + 1) + 8 * info.anchors
        assert info.bytes_per_kmer < 4.0
        got, want = ix.query((q_seq, q_off), bits=True), table.query((q_seq, q_off), bits=True)
    for f in FIELDS:
        assert np.array_equal(getattr(got, f), getattr(want, f)), f
    total, valid, found = int(got.kmers.sum()), int(got.valid.sum()), int(got.found.sum())
    assert 50_000 < found < valid < total


def test_through_the_product(gpu, tmp_path):
    """Reads of a small genome compacted, both tig sets written, the query asked of every index kind over every indexed set: the TSV
    and the presence file never change, and over the tigs the minimizer index is no larger per k-mer window than over the unitigs."""
    k = 21
    rng = random.Random(4)
    reads = [h[at:at + 150] for h in synth.random_genome(2500, seed=4) for at in range(0, len(h) - 149, 37)]  # (haplotypes: bubbles)
    reads = [synth.revcomp(r) if rng.random() < 0.5 else r for r in reads]
    query = []
    for i in range(30):
        s = list(rng.choice(reads) if rng.random() < 0.7 else cases.dna(rng, rng.randint(0, 80)))
        for j in range(len(s)):
            if rng.random() < 0.03:
                s[j] = rng.choice("ACGTNn")
        query.append("".join(s))
    r_fa, q_fa = tmp_path / "reads.fa", tmp_path / "q.fa"
    r_fa.write_text("".join(f">r{i}\n{s}\n" for i, s in enumerate(reads)))
    q_fa.write_text("".join(f">q{i}\n{s}\n" for i, s in enumerate(query)))

    def run(tag, *extra):
        out = [tmp_path / f"{tag}.{x}" for x in ("tsv", "txt", "g.fa", "e.fa")]
        r = subprocess.run([sys.executable, "-m", "matchtigs_amd", "--seq-in", str(r_fa), "-k", str(k), "--greedytigs-fa-out", str(out[2]),
                            "--eulertigs-fa-out", str(out[3]), "--query-fa", str(q_fa), "--query-out", str(out[0]), "--query-presence-out",
                            str(out[1]), *extra], capture_output=True, text=True, cwd=str(ROOT), timeout=600)
        assert r.returncode == 0, (tag, r.stderr[-2000:])
        return out[0].read_bytes(), out[1].read_bytes(), [l for l in r.stderr.splitlines() if l.startswith("Indexing the ")]

    tsv, pres, lines = run("plain")
    assert lines == [] and tsv.count(b"\n") == 1 + len(query)
    want = R.query(R.index_set(reads, k), query, k)
    assert [l.split("\t")[2:] for l in tsv.decode().splitlines()[1:]] == [[str(want[f][i]) for f in ("kmers", "valid", "found")] for i in range(len(query))]
    assert 0 < sum(want["found"]) < sum(want["valid"]) < sum(want["kmers"])
    per_kmer = {}
    for kind in ("table", "minimizer"):
        for over in ("input", "greedytigs", "eulertigs"):
            got_tsv, got_pres, lines = run(f"{kind}_{over}", "--query-index", kind, "--query-index-over", over)
            assert got_tsv == tsv and got_pres == pres, (kind, over)
            assert len(lines) == 1 and lines[0].startswith(f"Indexing the {over}: {'table index' if kind == 'table' else 'minimizer index (m = 14)'}: ")
            found = re.search(r" (\d+) bases in (\d+) records, (\d+) anchors.* (\d+) heavy buckets with (\d+) windows, (\d+) device bytes, "
                              r"([0-9.]+) bytes per k-mer window$", lines[0])
            assert found, lines[0]
            per_kmer[kind, over] = float(found.group(7))
    got_tsv, got_pres, lines = run("m9", "--query-index", "minimizer", "--query-minimizer-length", "9")
    assert got_tsv == tsv and got_pres == pres and lines[0].startswith("Indexing the input: minimizer index (m = 9): ")
    print("bytes per k-mer window:", per_kmer)
    for over in ("greedytigs", "eulertigs"):  # fewer bases spell the same k-mers
        assert per_kmer["minimizer", over] <= per_kmer["minimizer", "input"], per_kmer
    assert per_kmer["minimizer", "input"] < per_kmer["table", "input"] / 2
