"""The k-mer set comparison on the GPU (kmer_compare_device.hip) against its restatement (kmer_compare_ref.py): every
field of the struct, the witnesses included, as exact integers. Random sets over many k (both table forms, palindromes, repeats
in either orientation), invariance under reverse complement / case / cutting, damaged tig sets, determinism, the path through the
product (API, `--verify`, `--verify-fa`) and the check at G-seq 10^8 bp. Only the last may skip (memory), and says so."""
import dataclasses
import gzip
import json
import random
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import kmer_compare_ref as R
from matchtigs_amd import api, synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
NONE = 2 ** 64 - 1
KS = [1, 2, 3, 4, 5, 16, 31, 32, 33, 34, 63, 64, 65, 101]


@pytest.fixture(scope="module")
def gpu(product_lib):
    import torch

    if product_lib.mtg_device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("these tests need a GPU: the k-mer set comparison has no CPU path")
    return torch


def _assert_equals_ref(a, b, k, what=""):
    got = dataclasses.asdict(api.compare_kmer_sets(a, b, k))
    want = R.compare(a, b, k)
    assert got == want, (what, k, {f: (got[f], want[f]) for f in want if got[f] != want[f]})
    return api.KmerComparison(**got)


def _dna(rng, n, weights):
    return "".join(rng.choices("ACGT", weights, k=n))


def _flip_case(rng, s):
    return "".join(c.lower() if rng.random() < 0.3 else c for c in s)


def _random_pair(rng, k):
    """Two sets cut from one short genome and its reverse complement (so k-mers repeat, in both orientations, within and between
    the sets), with a palindrome planted for even k, a biased alphabet, foreign records, mixed case and lengths 0 .. 3 k."""
    weights = rng.choice([(1, 1, 1, 1), (6, 1, 1, 2), (5, 0, 0, 5), (1, 4, 4, 1)])
    half = _dna(rng, k // 2, weights)
    genome = _dna(rng, 2 * k + 2, weights) + (half + synth.revcomp(half) if k % 2 == 0 else "") + _dna(rng, 2 * k + 2, weights)
    sources = (genome, synth.revcomp(genome))

    def one_set():
        out = []
        for _ in range(rng.randint(0, 8)):
            n = rng.randint(0, 3 * k)
            x = rng.random()
            if x < 0.8:
                g = sources[x < 0.35]
                at = rng.randint(0, len(g) - n)
                s = g[at:at + n]
            else:
                s = _dna(rng, n, weights)
            out.append(_flip_case(rng, s))
        return out

    a = one_set()
    b = one_set() if rng.random() < 0.85 else [_flip_case(rng, synth.revcomp(s.upper())) for s in reversed(a)]
    return a, b


@pytest.mark.parametrize("k", KS)
def test_random_sets(gpu, k):
    rng = random.Random(1000 + k)
    seen = {"repeat": False, "rc_repeat": False, "palindrome": False}
    differ = equal = 0
    for i in range(200):
        a, b = _random_pair(rng, k)
        c = _assert_equals_ref(a, b, k, f"pair {i}")
        differ += not c.equal
        equal += c.equal and c.distinct_a > 0
        for f, v in R.kinds(a + b, k).items():
            seen[f] |= v
    # the generator really produces what the cases are for
    assert seen["repeat"] and seen["rc_repeat"] and seen["palindrome"] == (k % 2 == 0), (k, seen)
    assert differ >= 20 and equal >= 5, (k, differ, equal)


@pytest.mark.parametrize("k", KS)
def test_empty_and_short_sets(gpu, k):
    rng = random.Random(k)
    full = [_dna(rng, 2 * k + 3, (1, 1, 1, 1)), _dna(rng, k, (1, 1, 1, 1))]
    short = [_dna(rng, n, (1, 1, 1, 1)) for n in (k - 1, 0, k // 2, k - 1)]
    for a, b in (([], full), (full, []), ([], []), (short, short), (short, full), (full, short), ([""], [""]), (full, [""] + full + [""])):
        c = _assert_equals_ref(a, b, k)
        if not a or not b or a is short or b is short:
            assert c.common == 0


@pytest.mark.parametrize("k", KS)
def test_invariance(gpu, k):
    """B = A with every record reverse-complemented, its case flipped at random and cut into pieces that overlap by k - 1."""
    rng = random.Random(77 + k)
    a = [_dna(rng, rng.randint(0, 6 * k + 40), (3, 1, 1, 2)) for _ in range(30)]
    b = []
    for s in a:
        r = _flip_case(rng, synth.revcomp(s))
        at = 0
        while True:  # pieces of at least k bases; the next one starts k - 1 before this one's end
            n = rng.randint(k, 2 * k + 5)
            if at + n >= len(r):
                b.append(r[at:])
                break
            b.append(r[at:at + n])
            at += n - (k - 1)
    c = _assert_equals_ref(a, b, k)
    assert c.equal and c.occurrences_b == c.occurrences_a > 0
    assert (c.first_only_in_a_record, c.first_only_in_a_pos, c.first_only_in_b_record, c.first_only_in_b_pos) == (NONE,) * 4


def _tigs_of(ug, k, algorithm=5, euler_mode=api.EulerMode.HostReferenceOrder):
    G = api.Bigraph.from_unitig_links(ug.weights, ug.links)
    if algorithm == 5:
        tigs = api.GreedytigAlgorithm.compute_tigs(G, api.GreedytigAlgorithmConfiguration(1, k, euler_mode=euler_mode))
    else:
        tigs = api.EulertigAlgorithm.compute_tigs(G, api.EulertigAlgorithmConfiguration(k, euler_mode=euler_mode))
    fa = api.write_walks_text_device(G, tigs, ug.unitigs, k).decode()
    return G, tigs, fa.split("\n")[1::2]


@pytest.mark.parametrize("k", [21, 31, 41])
def test_damage(gpu, k):
    ug = synth.g_seq(20000, seed=k, k=k)
    _, _, tigs = _tigs_of(ug, k)
    assert _assert_equals_ref(ug.unitigs, tigs, k, "intact").equal
    rng = random.Random(k)
    longest = max(range(len(tigs)), key=lambda i: len(tigs[i]))
    t = tigs[longest]
    mid = len(t) // 2
    changed = t[:mid] + {"A": "C", "C": "G", "G": "T", "T": "A"}[t[mid]] + t[mid + 1:]
    cases = {
        "drop": tigs[:longest] + tigs[longest + 1:],
        "change": tigs[:longest] + [changed] + tigs[longest + 1:],
        "append": tigs + [_dna(rng, 3 * k, (1, 1, 1, 1))],
    }
    sa = synth.kmer_set_of_tigs(ug.unitigs, k)
    for name, b in cases.items():
        c = _assert_equals_ref(ug.unitigs, b, k, name)
        sb = synth.kmer_set_of_tigs(b, k)
        assert (c.only_in_a > 0) == (name in ("drop", "change")) and (c.only_in_b > 0) == (name in ("change", "append")), name
        if c.only_in_a:  # the witness window, read from the input text, really is absent from the other set
            w = api.kmer_at(ug.unitigs, c.first_only_in_a_record, c.first_only_in_a_pos, k)
            assert len(w) == k and synth.canonical(w) in sa and synth.canonical(w) not in sb, name
        if c.only_in_b:
            w = api.kmer_at(b, c.first_only_in_b_record, c.first_only_in_b_pos, k)
            assert len(w) == k and synth.canonical(w) in sb and synth.canonical(w) not in sa, name


_DETERMINISM_CHILD = """
import dataclasses, json, sys
sys.path.insert(0, sys.argv[1])
import test_gpu_kmer_compare as T
from matchtigs_amd import api
a, b = T._determinism_case()
print(json.dumps(dataclasses.asdict(api.compare_kmer_sets(a, b, 31))))
"""


def _determinism_case():
    """About 10^6 k-mers with differences on both sides: the unitigs of one genome with a second haplotype that differs from it in
    1 % of the bases, against the same genome with one that differs in 2 %."""
    ua = synth.g_seq_arrays(500_000, seed=5, k=31, haplotypes=2, sub_rate=0.01)
    ub = synth.g_seq_arrays(500_000, seed=5, k=31, haplotypes=2, sub_rate=0.02)
    return (ua.seq, ua.off), (ub.seq, ub.off)


def test_determinism(gpu):
    a, b = _determinism_case()
    runs = [dataclasses.asdict(api.compare_kmer_sets(a, b, 31)) for _ in range(3)]
    assert runs[0]["only_in_a"] > 0 and runs[0]["only_in_b"] > 0 and runs[0]["distinct_a"] + runs[0]["distinct_b"] > 1_000_000
    assert runs[0]["first_only_in_a_record"] != NONE and runs[0]["first_only_in_b_record"] != NONE
    assert runs[1] == runs[0] and runs[2] == runs[0]
    r = subprocess.run([sys.executable, "-c", _DETERMINISM_CHILD, str(ROOT / "tests")], capture_output=True, text=True, cwd=str(ROOT), timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == runs[0]
    # and the witnesses are what a plain scan of the codes says (numpy, k = 31)
    sa, sb = (synth.kmer_codes_of_sequences(x[0], x[1], 31) for x in (a, b))
    assert runs[0]["distinct_a"] == len(sa) and runs[0]["distinct_b"] == len(sb)
    assert runs[0]["common"] == len(np.intersect1d(sa, sb, assume_unique=True))


@pytest.mark.parametrize("route", ["bcalm2", "fasta"])
def test_through_the_product(gpu, tmp_path, route):
    k = 31
    ua = synth.g_seq_arrays(100_000, seed=3, k=k)
    units = ua.unitig_list()
    inp = tmp_path / "u.fa"
    if route == "bcalm2":
        inp.write_bytes(ua.bcalm2_text())
        G, store = api.read_bcalm2(str(inp), k)
    else:
        inp.write_text("".join(f">{i}\n{s}\n" for i, s in enumerate(units)))
        G, store = api.read_fasta(str(inp), k)
    for alg in (3, 5):
        for mode in (api.EulerMode.HostReferenceOrder, api.EulerMode.Device):
            if alg == 5:
                lim, ed = api.GreedytigAlgorithm.compute_tigs_np(G, api.GreedytigAlgorithmConfiguration(1, k, euler_mode=mode))
            else:
                lim, ed = api.EulertigAlgorithm.compute_tigs_np(G, api.EulertigAlgorithmConfiguration(k, euler_mode=mode))
            tigs = api.write_walks_text_device(G, (lim, ed), units, k).decode().split("\n")[1::2]
            c = api.compare_kmer_sets(store, tigs, k)
            assert c.equal and c.distinct_a == c.distinct_b == len(ua.kmers), (alg, mode, c)
            assert c.records_b == len(lim) and c.occurrences_a == c.distinct_a
            if alg == 3:
                assert c.repeated_b == 0
            else:
                bits = api.write_duplication_bitvector(G, (lim, ed))
                assert bits.count(b"1") == c.distinct_b and bits.count(b"0") == c.repeated_b and c.repeated_b > 0
            assert c == api.compare_kmer_sets((ua.seq, ua.off), (np.frombuffer("".join(tigs).encode(), np.uint8),
                                                                  np.concatenate([[0], np.cumsum([len(t) for t in tigs])]).astype(np.uint64)), k)
            G.reset()
    # the command line
    flag = "--bcalm-in" if route == "bcalm2" else "--fa-in"

    def run(*a):
        return subprocess.run([sys.executable, "-m", "matchtigs_amd", flag, str(inp), "-k", str(k), *a], capture_output=True, text=True,
                              cwd=str(ROOT), timeout=900)

    out, eout, gz = tmp_path / "g.fa", tmp_path / "e.fa", tmp_path / "g.fa.gz"
    r = run("--greedytigs-fa-out", str(out), "--eulertigs-fa-out", str(eout), "--verify")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stderr.splitlines() if l.startswith("Verifying ")]
    assert len(lines) == 2 and all("k-mer sets equal" in l and f"{len(ua.kmers)} distinct k-mers" in l for l in lines), r.stderr[-2000:]
    assert f"{int(ua.off[-1])} -> " in lines[0] and "(0 repeated)" in lines[0]  # (eulertigs come first)
    r = run("--greedytigs-fa-out", str(gz), "--verify")
    assert r.returncode == 0 and "k-mer sets equal" in r.stderr, r.stderr[-2000:]
    assert gzip.decompress(gz.read_bytes()) == out.read_bytes()
    r = run("--greedytigs-gfa-out", str(tmp_path / "g.gfa"), "--verify")
    assert r.returncode == 0 and "spelled in memory" in r.stderr and "k-mer sets equal" in r.stderr, r.stderr[-2000:]
    # a damaged copy: one base of the longest tig changed
    text = out.read_text().split("\n")
    i = max(range(1, len(text), 2), key=lambda j: len(text[j]))
    mid = len(text[i]) // 2
    text[i] = text[i][:mid] + {"A": "C", "C": "G", "G": "T", "T": "A"}[text[i][mid]] + text[i][mid + 1:]
    bad = tmp_path / "bad.fa"
    bad.write_text("\n".join(text))
    r = run("--verify-fa", str(out), "--verify-fa", str(bad))
    lines = [l for l in r.stderr.splitlines() if l.startswith("Verifying ")]
    assert r.returncode == 1 and len(lines) == 2 and "equal" in lines[0] and "DIFFER" in lines[1], r.stderr[-2000:]
    missing = lines[1].split("first missing k-mer: ")[1].split(";")[0].split()[-1]
    foreign = lines[1].split("first foreign k-mer: ")[1].split(";")[0].split()[-1]
    damaged = synth.kmer_set_of_tigs(text[1::2], k)
    assert len(missing) == k and synth.canonical(missing) in synth.kmer_set_of_tigs(units, k) and synth.canonical(missing) not in damaged
    assert len(foreign) == k and synth.canonical(foreign) in damaged and synth.canonical(foreign) not in synth.kmer_set_of_tigs(units, k)
    assert out.exists() and bad.exists()


def _free_memory_gb(torch):
    free_hbm = torch.cuda.mem_get_info()[0] / 2 ** 30
    with open("/proc/meminfo") as f:
        free_host = next(int(l.split()[1]) for l in f if l.startswith("MemAvailable")) / 2 ** 20
    return free_hbm, free_host


def fasta_sequence_arrays(fa: bytes):
    """(uint8 bases, uint64 offsets) of a FASTA with one header and one sequence line per record, by numpy."""
    a = np.frombuffer(fa, np.uint8)
    nl = np.nonzero(a == 10)[0]
    assert len(nl) % 2 == 0 and (len(a) == 0 or a[0] == ord(">"))
    starts, ends = nl[0::2] + 1, nl[1::2]
    off = np.zeros(len(starts) + 1, np.uint64)
    off[1:] = np.cumsum(ends - starts)
    d = np.zeros(len(a) + 1, np.int32)  # +1 where a sequence line starts, -1 where it ends: the running sum marks its bytes
    d[starts] += 1
    d[ends] -= 1
    return a[np.cumsum(d[:-1], dtype=np.int32) > 0], off


def test_at_size_gseq_1e8(gpu):
    """G-seq 10^8 bp, k = 31, greedy matchtigs in device order: the spelled tigs hold exactly the unitigs' k-mers. The only case of
    this file that may skip: it needs 60 GB of free HBM and of host memory."""
    torch = gpu
    free_hbm, free_host = _free_memory_gb(torch)
    if free_hbm < 60 or free_host < 60:
        pytest.skip(f"the 10^8 bp case needs 60 GB of HBM and of host memory; this box has {free_hbm:.0f} / {free_host:.0f} (the only case of this file that may skip)")
    k = 31
    ua = synth.g_seq_arrays_torch(100_000_000, seed=1, k=k)
    torch.cuda.empty_cache()
    G = api.Bigraph.from_unitig_links_arrays(ua.weights, ua.links)
    lim, ed = api.GreedytigAlgorithm.compute_tigs_np(G, api.GreedytigAlgorithmConfiguration(1, k, euler_mode=api.EulerMode.Device))
    fa = api.write_walks_text_device(G, (lim, ed), (ua.seq, ua.off), k)
    del G
    seq, off = fasta_sequence_arrays(fa)
    del fa
    c = api.compare_kmer_sets((ua.seq, ua.off), (seq, off), k)
    t = api.last_kmer_compare_times()
    api.release_device_memory(0)
    print(f"G-seq 1e8: {c.describe()}; {t}")
    assert c.equal and c.distinct_a == c.distinct_b == len(ua.kmers)
    assert c.records_a == ua.n_unitigs and c.records_b == len(lim) and c.characters_b == int(off[-1]) < c.characters_a
    codes, n_occ = synth.kmer_codes_of_sequences_torch(seq, off, k)
    assert c.occurrences_b == n_occ and np.array_equal(codes, ua.kmers)
