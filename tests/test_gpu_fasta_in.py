"""Plain unitig FASTA input (`--fa-in X -k K`): the graph of the (k-1)-mer overlaps of the unitig ends, joined on the GPU
(fasta_in_device.hip). Every array the library builds must equal an independent restatement of the contract
(tests/fasta_in_ref.py) exactly; against the link route (`--bcalm-in` / the clib.rs builder) the partition of unitig ends may only
differ by the documented merge of ends that share an oriented (k-1)-mer and are all in-ends or all out-ends."""
import gzip
import random
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import fasta_in_ref as R
from matchtigs_amd import api, synth

ROOT = Path(__file__).resolve().parent.parent
FIELDS = ("mirror", "edge_from", "edge_to", "edge_weight", "edge_unitig", "edge_forwards")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(product_lib):
    if product_lib.mtg_device_count() < 1:
        pytest.fail("these tests need a GPU: the plain-FASTA join has no CPU fallback")
    return product_lib


def _assert_graph(got: dict, want: dict, what=""):
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), (what, f)
    assert not got["edge_dummy_id"].any()


def _rng_dna(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _overlapping_pieces(rng, genome: str, k: int, n: int, min_len: int, max_len: int) -> list[str]:
    """Pieces of `genome` that chain with (k-1)-overlaps, some reverse-complemented, plus repeats of some of them."""
    pieces, pos = [], 0
    while pos + max_len < len(genome) and len(pieces) < n:
        ln = rng.randint(min_len, max_len)
        p = genome[pos:pos + ln]
        pieces.append(R.revcomp(p) if rng.random() < 0.4 else p)
        pos += ln - (k - 1)
    pieces += [pieces[i] for i in rng.sample(range(len(pieces)), min(5, len(pieces)))]
    return pieces


@pytest.mark.parametrize("k", [15, 21, 31])
@pytest.mark.parametrize("form", ["plain", "gz"])
def test_gseq_arrays_equal_the_restatement(tmp_path, gpu, k, form):
    ug = synth.g_seq(6000, seed=k, k=k, haplotypes=3, sub_rate=0.03)
    seqs = ug.unitigs
    recs = [s.lower() if i % 3 == 1 else s for i, s in enumerate(seqs)]               # lower case
    headers = [f"{i} LN:i:{len(s)} L:+:{(i + 1) % len(seqs)}:- junk\t|x|" for i, s in enumerate(seqs)]  # any text, L: ignored
    text = R.fasta_text(recs, width=7, headers=headers)                                   # multi-line records
    text = text.replace("\n>", "\n\n>", 5)                                                # empty lines
    p = tmp_path / ("u.fa.gz" if form == "gz" else "u.fa")
    if form == "gz":
        with gzip.open(p, "wt") as f:
            f.write(text)
    else:
        p.write_text(text)
    G, store = api.read_fasta(str(p), k)
    assert store.sequences() == seqs
    _assert_graph(G.export(), R.graph_dict(seqs, k), (k, form))
    t = api.last_fasta_in_times()
    assert t["kernel_ms"] > 0 and t["bytes"] > 0 and t["parse_ms"] > 0
    # the in-memory entry builds the same graph, from a list and from (data, offsets)
    _assert_graph(api.Bigraph.from_sequences(recs, k).export(), R.graph_dict(seqs, k))
    data = "".join(seqs).encode()
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    _assert_graph(api.Bigraph.from_sequences((data, off), k).export(), R.graph_dict(seqs, k))


@pytest.mark.parametrize("k", [63, 101])
def test_long_k_crosses_word_boundaries(gpu, k):
    rng = random.Random(k)
    genome = _rng_dna(rng, 40 * k)
    # a second haplotype with point changes: (k-1)-mers that differ in one base at varied positions inside the 32-base words
    g2 = list(genome)
    for i in range(0, len(g2), k // 2 + 3):
        g2[i] = "ACGT"[("ACGT".index(g2[i]) + 1) % 4]
    g2 = "".join(g2)
    seqs = _overlapping_pieces(rng, genome, k, 60, k, 3 * k) + _overlapping_pieces(rng, g2, k, 30, k, 2 * k)
    assert min(map(len, seqs)) >= k
    want = R.graph_dict(seqs, k)
    _assert_graph(api.Bigraph.from_sequences(seqs, k).export(), want, k)
    assert len(want["mirror"]) < 4 * len(seqs)  # (the pieces do share ends)


def test_hand_made_shapes(gpu):
    cases = [
        (5, ["ACGTA", "TACGT", "ACGTC", "GACGT"]),        # palindromic (k-1)-mer ACGT at both kinds of end (odd k)
        (4, ["ACGACG", "ACGTTACG"]),                     # prefix == own suffix
        (4, ["AACGTT", "AACTGCAGTT"]),                   # prefix == rc(own suffix)
        (6, ["ACGTAC", "ACGTAC", "GTACGT", "ACGTACG"]),   # records of length exactly k, duplicates
        (5, ["AAACG", "AAACT", "AAACA", "AAACC", "TGTTT", "CGTTT", "GAAAC", "AAAC" + "GGGG"]),  # many records share AAAC
        (3, ["ATA", "TAT", "ATAT"]),                     # k - 1 = 2: palindrome AT, self-loops
    ]
    for k, seqs in cases:
        want = R.graph_dict(seqs, k)
        _assert_graph(api.Bigraph.from_sequences(seqs, k).export(), want, (k, seqs))


def test_random_small_sets_many_k(gpu):
    rng = random.Random(7)
    for k in (2, 3, 4, 9, 17, 32, 33, 34, 64, 65, 66):
        genome = _rng_dna(rng, 30 * k + 200)
        seqs = _overlapping_pieces(rng, genome, k, 40, k, 2 * k + 5)
        seqs += [_rng_dna(rng, k + rng.randint(0, 5)) for _ in range(10)]
        _assert_graph(api.Bigraph.from_sequences(seqs, k).export(), R.graph_dict(seqs, k), k)


def test_scale_gseq_1e8(gpu):
    ua = synth.g_seq_arrays_torch(100_000_000, seed=1, k=31)
    assert ua.n_unitigs > 9_000_000
    G = api.Bigraph.from_sequences((ua.seq, ua.off), 31)
    t = api.last_fasta_in_times()
    got = G.export()
    del G
    want = R.graph_np(ua.seq, ua.off, 31)
    _assert_graph(got, want, "G-seq 1e8")
    print(f"G-seq 1e8: {ua.n_unitigs} unitigs -> {len(want['mirror'])} nodes; {t}")


@pytest.mark.parametrize("k", [15, 21])
def test_against_the_link_route(gpu, k):
    for seed in (2, 3):
        ug = synth.g_seq(8000, seed=seed, k=k, haplotypes=4, sub_rate=0.03)
        link = api.Bigraph.from_unitig_links(ug.weights, ug.links).export()
        fa = api.Bigraph.from_sequences(ug.unitigs, k).export()
        ok, predicted = R.end_partitions_agree(link, fa)
        assert ok and predicted == len(link["mirror"]), (k, seed)


def test_out_end_merge_differs_from_the_link_route(tmp_path, gpu):
    """Two unitigs start with AAAC, none ends in it: one edge-centric node here, two node pairs on the link route."""
    k = 5
    p = tmp_path / "u.fa"
    p.write_text(">a\nAAACG\n>b\nAAACT\n")
    G, _ = api.read_fasta(str(p), k)
    fa = G.export()
    link = api.Bigraph.from_unitig_links([1, 1], []).export()
    assert len(fa["mirror"]) == 6 and len(link["mirror"]) == 8
    assert fa["edge_from"][0] == fa["edge_from"][2] == 0 and fa["edge_to"][1] == fa["edge_to"][3] == 1
    assert link["edge_from"][0] != link["edge_from"][2]
    ok, predicted = R.end_partitions_agree(link, fa)
    assert ok and predicted == 8


def _fasta_records(text: bytes):
    lines = [l for l in text.split(b"\n") if l]
    seqs = [l for l in lines if not l.startswith(b">")]
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer(b"".join(seqs), np.uint8), off


def test_cli_end_to_end_gseq_4p6m(tmp_path, gpu, oracle):
    k = 31
    ua = synth.g_seq_arrays_torch(4_600_000, seed=1, k=k, haplotypes=4, sub_rate=0.02)
    s = ua.seq.tobytes()
    o = ua.off.astype(np.int64)
    inp = tmp_path / "u.fa"
    inp.write_bytes(b"".join(b">%d\n%s\n" % (u, s[o[u]:o[u + 1]]) for u in range(ua.n_unitigs)))
    out, eout = tmp_path / "o.fa", tmp_path / "e.fa"
    r = subprocess.run([sys.executable, "-m", "matchtigs_amd", "--fa-in", str(inp), "-k", str(k), "--greedytigs-fa-out", str(out),
                        "--eulertigs-fa-out", str(eout)], capture_output=True, text=True, cwd=str(ROOT), timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    for path in (out, eout):
        seq, off = _fasta_records(path.read_bytes())
        assert np.array_equal(synth.kmer_codes_of_sequences(seq, off, k), ua.kmers), path.name
    # the greedy pairs on the --fa-in graph equal the oracle's on the same graph
    G, store = api.read_fasta(str(inp), k)
    assert len(store) == ua.n_unitigs
    ex = G.export()
    _assert_graph(ex, R.graph_np(ua.seq, ua.off, k))
    dev = api.DeviceGraph(G, k)
    dev.classify()
    got = api.compute_pairs([dev])
    want, _ = oracle.OracleGraph.from_arrays(ex["mirror"], ex["edge_from"], ex["edge_to"], ex["edge_weight"]).greedy_pairs_np(k)
    assert len(got) == len(want) and all(np.array_equal(got[f], want[f]) for f in ("out", "in", "dist"))
