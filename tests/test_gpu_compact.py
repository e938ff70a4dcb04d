"""The unitig compaction on the GPU (`--seq-in`, mtg_compact_unitigs): bytes, offsets and statistics of the device
against the restatement of the contract (compact_ref.py) on random haplotypes for narrow and wide k and on the special shapes; a
long unitig (the pointer jumping must not walk); invariance under record order and strand; determinism; the product path through
the CLI; the graph at size against the tree's torch compaction; and every rung of the ladder over every input form giving one answer."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import compact_ref as R
from matchtigs_amd import synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _device(seqs, k):
    from matchtigs_amd import api

    store, c = api.compact_unitigs(seqs, k)
    data, off = store.arrays()
    return data.tobytes().decode(), [int(x) for x in off], c


def _check(seqs, k):
    """Device output == restatement: bytes, offsets, statistics."""
    import dataclasses

    unitigs, stats, _ = R.compact(seqs, k)
    data, off, c = _device(seqs, k)
    assert dataclasses.asdict(c) == stats
    assert off == [0] + list(np.cumsum([len(u) for u in unitigs]))
    assert data == "".join(unitigs)
    return unitigs, stats


@pytest.mark.parametrize("k", [2, 3, 4, 15, 21, 31, 32, 33, 63, 64, 101])
def test_haplotypes_equal_the_restatement(product_lib, k):
    length = 40 if k <= 4 else 1500
    seqs = synth.random_genome(length, seed=k, haplotypes=4, sub_rate=0.02)
    _, stats = _check(seqs, k)
    assert stats["distinct_kmers"] > 0


@pytest.mark.parametrize("k", [4, 31, 32, 40])
def test_special_shapes(product_lib, k):
    g = synth.random_genome(300, seed=100 + k, haplotypes=1)[0]
    _check([g[:k]], k)                                            # one record of exactly k bases
    _check([g[:k - 1], g, "", g[5:k + 3], "A", g[7:k + 6]], k)    # records shorter than k mixed in
    u, s = _check(["A" * (k + 5)], k)                             # a homopolymer: a closed walk of length 1
    assert u == ["A" * k] and s["closed_walks"] == 1
    long_k = k >= 31  # (a random piece of 100 bases repeats no 30-mer: the shapes below are then exactly what their comments say)
    _check(["T" * (k + 5), g], k)
    if k % 2 == 0:                                                # an even-k palindromic k-mer
        half = g[:k // 2]
        pal = half + synth.revcomp(half)
        u, _ = _check([g[20:60] + pal + g[80:120], pal], k)
        assert pal in u or not long_k
    stem = g[:k + 6]                                              # a hairpin: a stem, a loop, the stem's reverse complement
    _check([stem + "ACG" + synth.revcomp(stem)], k)
    _check([stem + synth.revcomp(stem)], k)
    circ = g[:3 * k + 7]                                          # a circular sequence: one closed walk, starting at the leader
    u, s = _check([circ + circ[:k - 1]], k)
    assert not long_k or (s["closed_walks"] == 1 and u == [circ + circ[:k - 1]])
    u, s = _check([g[200:260], circ[k:] + circ[:k] + circ[k:2 * k - 1]], k)  # ... rotated, behind another record
    assert not long_k or s["closed_walks"] == 1
    u, s = _check([synth.revcomp(circ + circ[:k - 1]), circ[5:] + circ[:5 + k - 1]], k)  # ... and both strands, two rotations
    assert not long_k or (s["closed_walks"] == 1 and s["unitigs"] == 1)
    _check([g, synth.revcomp(g)], k)                              # the same set given as sequence plus reverse complement
    _check([g[:150], g[100:], g[:150], g[100:]], k)               # every record duplicated
    _check([g.lower(), g[:100]], k)                               # lower case
    assert _device([g.lower()], k)[0] == _device([g], k)[0]


def test_empty_inputs(product_lib):
    assert _device([], 5)[:2] == ("", [0])
    assert _device(["ACG", ""], 5)[:2] == ("", [0])
    _check(["ACG", ""], 5)


def test_non_acgt_aborts(product_lib):
    r = subprocess.run([sys.executable, "-c", "from matchtigs_amd import api; api.compact_unitigs(['ACGTNACGT'], 3)"],
                       capture_output=True, text=True, cwd=str(ROOT), timeout=300)
    assert r.returncode != 0 and "character at offset 4 is not in the DNA alphabet" in r.stderr, r.stderr[-500:]


def _random_ascii(length, seed, stream=10):
    return np.frombuffer(b"ACGT", np.uint8)[(synth.splitmix64(seed, length, stream) % np.uint64(4)).astype(np.int64)]


def _haplotype_arrays(length, seed, haplotypes=4, sub_rate=0.02):
    """synth.random_genome as one uint8 array plus offsets (the same splitmix64 streams, no Python strings)."""
    abc = np.frombuffer(b"ACGT", np.uint8)
    g = (synth.splitmix64(seed, length, 10) % np.uint64(4)).astype(np.int64)
    data = np.empty(haplotypes * length, np.uint8)
    data[:length] = abc[g]
    for h in range(1, haplotypes):
        mut = synth._uniform01(synth.splitmix64(seed, length, 20 + h)) < sub_rate
        shift = (synth.splitmix64(seed, length, 40 + h) % np.uint64(3)).astype(np.int64) + 1
        data[h * length:(h + 1) * length] = abc[np.where(mut, (g + shift) % 4, g)]
    return data, (np.arange(haplotypes + 1, dtype=np.uint64) * np.uint64(length))


def test_haplotype_arrays_equal_random_genome():
    data, off = _haplotype_arrays(500, 7)
    s = data.tobytes().decode()
    assert [s[int(off[i]):int(off[i + 1])] for i in range(4)] == synth.random_genome(500, 7)


def test_long_unitig(product_lib):
    """One random 4.6 Mbp sequence at k = 31: almost surely one unitig of 4.6 M k-mers. A chain walked sequentially would take
    minutes; pointer jumping takes ~23 rounds."""
    import time

    from matchtigs_amd import api

    k, n = 31, 4_600_000
    data = _random_ascii(n, 3)
    off = np.array([0, n], np.uint64)
    t0 = time.perf_counter()
    store, c = api.compact_unitigs((data, off), k)
    wall = time.perf_counter() - t0
    t = api.last_compact_times()
    print(f"long unitig: {c.describe()}; {t}; wall {wall:.2f}s")
    assert c.distinct_kmers == c.unitig_characters - (k - 1) * c.unitigs
    assert c.unitigs < 100 and c.longest_unitig_kmers > n // 100
    assert t["rounds"] <= 2 * 24
    cmp = api.compare_kmer_sets((data, off), store, k)
    assert cmp.equal and cmp.occurrences_b == cmp.distinct_b == c.distinct_kmers
    assert wall < 60


def test_invariance(product_lib):
    """Permuting the records or reverse-complementing some leaves the set of canonical unitig strings unchanged."""
    k = 21
    seqs = synth.random_genome(3000, seed=5, haplotypes=4)
    seqs = [s[i:i + 700] for s in seqs for i in range(0, 3000 - 680, 680)]  # overlapping pieces (k - 1 = 20 bases shared)
    base = sorted(synth.canonical(u) for u in R.compact(seqs, k)[0])
    rng = np.random.default_rng(1)
    for _ in range(3):
        perm = [seqs[i] for i in rng.permutation(len(seqs))]
        perm = [synth.revcomp(s) if rng.random() < 0.5 else s for s in perm]
        data, off, _ = _device(perm, k)
        got = sorted(synth.canonical(data[off[i]:off[i + 1]]) for i in range(len(off) - 1))
        assert got == base


def test_determinism(product_lib):
    seqs = synth.random_genome(200_000, seed=9, haplotypes=4)
    a, b = _device(seqs, 31), _device(seqs, 31)
    assert a == b
    a, b = _device(seqs, 45), _device(seqs, 45)
    assert a == b


def _cli(*a):
    return subprocess.run([sys.executable, "-m", "matchtigs_amd", *a], capture_output=True, text=True, cwd=str(ROOT), timeout=1200)


def test_product_path(product_lib, tmp_path):
    """Sequences in, tigs out, verified against the sequences; the unitig file fed back through --fa-in gives byte-identical tigs."""
    data, off = _haplotype_arrays(4_600_000, 1)
    s = data.tobytes()
    with open(tmp_path / "H.fa", "wb") as f:
        for h in range(4):
            f.write(b">hap%d\n" % h)
            rec = s[int(off[h]):int(off[h + 1])]
            for i in range(0, len(rec), 1 << 16):  # multi-line records
                f.write(rec[i:i + (1 << 16)] + b"\n")
    p = {n: str(tmp_path / n) for n in ("H.fa", "g.fa", "e.fa", "u.fa", "g2.fa", "e2.fa", "bad.fa")}
    r = _cli("--seq-in", p["H.fa"], "-k", "31", "--greedytigs-fa-out", p["g.fa"], "--eulertigs-fa-out", p["e.fa"], "--unitigs-fa-out", p["u.fa"],
             "--verify")
    print(r.stderr[-3000:])
    assert r.returncode == 0, r.stderr[-3000:]
    assert "compacted from 4 records" in r.stderr and r.stderr.count("k-mer sets equal") == 2
    r = _cli("--fa-in", p["u.fa"], "-k", "31", "--greedytigs-fa-out", p["g2.fa"], "--eulertigs-fa-out", p["e2.fa"])
    assert r.returncode == 0, r.stderr[-3000:]
    for a, b in (("g.fa", "g2.fa"), ("e.fa", "e2.fa")):
        assert Path(p[a]).read_bytes() == Path(p[b]).read_bytes(), f"{a} differs from {b}"
    # the unitigs spell the haplotypes' k-mer set; a damaged unitig file does not
    r = _cli("--seq-in", p["H.fa"], "-k", "31", "--verify-fa", p["u.fa"])
    assert r.returncode == 0 and "k-mer sets equal" in r.stderr, r.stderr[-3000:]
    u = bytearray(Path(p["u.fa"]).read_bytes())
    at = u.index(b"\n") + 1 + 40
    u[at] = ord("A") if u[at] != ord("A") else ord("C")
    Path(p["bad.fa"]).write_bytes(bytes(u))
    r = _cli("--seq-in", p["H.fa"], "-k", "31", "--verify-fa", p["bad.fa"])
    assert r.returncode == 1 and "k-mer sets DIFFER" in r.stderr, r.stderr[-3000:]


def test_at_size(product_lib):
    """G-seq 10^8 bp x 4 haplotypes, k = 31: the unitig and character counts of the tree's torch compaction (DESIGN.md 15 records
    9 645 478 and 528 639 068 for this graph), and the unitigs spell the haplotypes' k-mer set without a repeat."""
    import torch

    from matchtigs_amd import api

    k, n = 31, 100_000_000
    data, off = _haplotype_arrays(n, 1)
    store, c = api.compact_unitigs((data, off), k)
    t = api.last_compact_times()
    print(f"at size: {c.describe()}; {t}")
    assert c.distinct_kmers == c.unitig_characters - (k - 1) * c.unitigs
    assert len(store) == c.unitigs
    cmp = api.compare_kmer_sets((data, off), store, k)
    assert cmp.equal and cmp.occurrences_b == cmp.distinct_b == c.distinct_kmers
    del store
    api.release_device_memory(0)
    ua = synth.g_seq_arrays_torch(n, seed=1, k=k)
    torch.cuda.empty_cache()
    print(f"torch compaction: {ua.n_unitigs} unitigs, {int(ua.off[-1])} characters")
    assert (c.unitigs, c.unitig_characters) == (ua.n_unitigs, int(ua.off[-1]))
    assert len(ua.kmers) == c.distinct_kmers


@pytest.mark.parametrize("k", [4, 31, 32, 33, 34])
def test_every_rung_and_input_form_give_one_answer(product_lib, tmp_path, k):
    """compact_unitigs, _counted (without and with kmer_counts), _colored and _colored_classes(split=False), each over a list of str,
    (array, offsets) and a UnitigStore, are one computation at min_abundance = 1: the same store and Compaction fifteen times -- the
    restatement's --, the same Abundance, counts, masks and classes wherever a rung returns them."""
    import dataclasses

    from matchtigs_amd import api

    a, b, c = ("".join("ACGT"[x] for x in np.random.default_rng(10 * k + i).integers(0, 4, n)) for i, n in enumerate((100, 230, 300)))
    seqs = [a, b, "ACG", a, c[:150] + b[40:140]]  # a repeated: abundances differ; "ACG" is shorter than every k
    colors = [i % 3 for i in range(len(seqs))]
    (tmp_path / "in.fa").write_text("".join(f">r{i}\n{s}\n" for i, s in enumerate(seqs)))
    as_store = api.read_sequences(str(tmp_path / "in.fa"))
    assert as_store.sequences() == seqs
    forms = (seqs, (np.frombuffer("".join(seqs).encode(), np.uint8), np.cumsum([0] + [len(s) for s in seqs]).astype(np.uint64)), as_store)
    rungs = (lambda x: api.compact_unitigs(x, k),
             lambda x: api.compact_unitigs_counted(x, k, 1),
             lambda x: api.compact_unitigs_counted(x, k, 1, kmer_counts=True),
             lambda x: api.compact_unitigs_colored(x, k, colors, 3),
             lambda x: api.compact_unitigs_colored_classes(x, k, colors, 3, split=False))
    results = [rung(form) for rung in rungs for form in forms]
    assert len(results) == 15

    unitigs, stats, _ = R.compact(seqs, k)
    assert results[0][0].sequences() == unitigs and dataclasses.asdict(results[0][1]) == stats
    for r in results:
        assert r[0].sequences() == unitigs and r[1] == results[0][1]
    counted = [r[2] for r in results if len(r) >= 3]
    assert len(counted) == 12 and counted[0].distinct_kept == stats["distinct_kmers"] and counted[0].max_abundance >= 2
    for ab in counted:
        assert (ab.distinct_all, ab.distinct_kept, ab.max_abundance, ab.kept_occurrences) == (
            counted[0].distinct_all, counted[0].distinct_kept, counted[0].max_abundance, counted[0].kept_occurrences)
        assert np.array_equal(ab.spectrum, counted[0].spectrum) and np.array_equal(ab.unitig_sums, counted[0].unitig_sums)
    assert all(ab.kmer_counts is None for ab in counted[:3])
    per_kmer = [ab.kmer_counts for ab in counted[3:]]
    assert len(per_kmer[0]) == stats["distinct_kmers"] and all(np.array_equal(x, per_kmer[0]) for x in per_kmer)
    colored = [r[3] for r in results if len(r) >= 4]
    assert len(colored) == 6 and len(colored[0].kmer_colors) == stats["distinct_kmers"]
    for col in colored:
        assert col.n_colors == 3 and np.array_equal(col.kmer_colors, colored[0].kmer_colors)
        assert np.array_equal(col.per_color, colored[0].per_color) and np.array_equal(col.shared, colored[0].shared)
        assert np.array_equal(col.occupancy, colored[0].occupancy)
    classed = [r for r in results if len(r) == 5]
    assert len(classed) == 3
    for r in classed:
        assert np.array_equal(r[4].masks[r[4].kmer_class], r[3].kmer_colors)
        assert all(np.array_equal(getattr(r[4], f), getattr(classed[0][4], f)) for f in ("masks", "kmers", "runs", "first", "kmer_class"))
