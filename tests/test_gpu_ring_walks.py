"""The closed-walk path of the unitig compaction on the GPU (compact_device.hip, DESIGN.md 16 under rank: the check after
log2_ceil(n_or) + 2 jump rounds, cycle_list, cycle_min_init, the ping-pong cycle_min rounds, cycle_cut, the second pointer jumping,
the `succ == head` tail in walk_kernel, the head with a predecessor in leader_kernel) on the rings of ring_cases.py: many cycles of
very different lengths at once, both parities of the ping-pong, C = 2^m exactly, cycles across waves and workgroups, ids that run
against the walk and jump inside it -- each against its restatement or a closed form that test_ring_cases.py has held to the
restatement, as exact bytes and integers, every call twice. Then every rung above it on the coloured worlds, a chromosome of
4.6 M bases and a ring of 2^20 (C = 2^21), 50 000 plasmids, and the rings through the join, the finish and the command line."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import fasta_in_ref as FA
import ring_cases as RC
import test_ring_cases as T
from matchtigs_amd import api
from test_gpu_color_split import _assert_classes, _same
from test_gpu_fasta_in import _assert_graph
from test_gpu_hash_collisions import _assert_store, _store
from test_gpu_kmer_color import _assert_colors_equal_ref

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def gpu(product_lib):
    import torch

    if product_lib.mtg_device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("these tests need a GPU: the compaction has no CPU path")
    return torch


def _assert_rounds(C, n_or):
    """The last call took the cycle path (more rounds than the first pointer jumping is given) and stayed within the code's budget."""
    lo, hi = RC.round_limits(C, n_or)
    rounds = api.last_compact_times()["rounds"]
    assert lo < rounds <= hi, (rounds, lo, hi)
    return rounds


# ---- plain compaction against the restatement ----
@pytest.mark.parametrize("name,k", T.PLAIN)
def test_rings_equal_the_restatement(gpu, name, k):
    recs = T.world(name, k)[0]
    unitigs, stats, closed, C, n_or = T.compacted(name, k)
    # the branch this case is here for, asserted where it is used
    parity = {"odd": 1, "even": 0, "2048": 0, "2049": 1, "small": 1}[name]
    assert RC.log2_ceil(C) % 2 == parity and stats["closed_walks"] == T.WANT[name, k][0] and (name != "2048" or C == n_or == 1 << 12)
    runs = []
    for _ in range(2):
        runs.append(api.compact_unitigs(recs, k))
        _assert_rounds(C, n_or)
    _assert_store(runs[0], unitigs, stats)
    assert _store(runs[1]) == _store(runs[0]) and runs[1][1] == runs[0][1]
    assert runs[0][1].closed_walks == sum(closed) and runs[0][1].longest_unitig_kmers == max(len(u) - k + 1 for u in unitigs)


# ---- every rung on the coloured worlds ----
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("m", [1, 2])
@pytest.mark.parametrize("k", T.COLOUR_KS)
@pytest.mark.parametrize("name", ["odd", "even"])
def test_every_rung_on_the_coloured_worlds(gpu, name, k, m, split):
    recs, colors, _ = T.world(name, k, True)
    unitigs, stats, closed, ab, col, classes = T.classed(name, k, m, split)
    C, n_or = RC.listed(k, unitigs, stats, closed)
    n_rings = len(T.WORLDS[name])
    assert stats["closed_walks"] == {(1, False): n_rings, (1, True): n_rings - 5, (2, False): 6, (2, True): 6}[m, split]
    assert stats["unitigs"] == 11 or m == 1
    runs = []
    for _ in range(2):
        runs.append(api.compact_unitigs_colored_classes(recs, k, colors, 3, min_abundance=m, split=split))
        _assert_rounds(C, n_or)
    store, c, a, co, cc = runs[0]
    _assert_store(runs[0], unitigs, stats)
    for f in ("distinct_all", "distinct_kept", "max_abundance", "kept_occurrences"):
        assert getattr(a, f) == ab[f], f
    assert a.spectrum.tolist() == ab["spectrum"] and a.unitig_sums.dtype == np.uint64 and a.unitig_sums.tolist() == ab["unitig_sums"]
    assert a.kmer_counts.dtype == np.uint32 and a.kmer_counts.tolist() == ab["kmer_counts"]
    _assert_colors_equal_ref(co, col, 3)
    _assert_classes(cc, classes, co.kmer_colors, c.unitigs, split)
    _same(runs[0], runs[1])
    if split:
        return
    # the rungs below on the same input: one store, one set of arrays
    counted = api.compact_unitigs_counted(recs, k, m, kmer_counts=True)
    _assert_rounds(C, n_or)
    coloured = api.compact_unitigs_colored(recs, k, colors, 3, m)
    _assert_rounds(C, n_or)
    _same(runs[0], coloured)
    _same(runs[0], counted + (co,))
    if m == 1:
        assert _store(api.compact_unitigs(recs, k)) == _store(runs[0])


# ---- at size, against closed forms ----
def _random_ring(n, seed):
    return RC.dna(np.random.default_rng(seed), n)


def test_a_chromosome(gpu):
    """One ring of 4.6 M bases at k = 31, behind the reverse complement of an arc of a million of its windows: the leader is the arc's
    last window, the walk runs against the ring as written, the ids descend along the arc and jump where the ring's record begins."""
    k, n = 31, 4_600_000
    recs, unitig = RC.ring_with_arc(_random_ring(n, 46), k, arc_rot=1_234_567, arc_n=1_000_000, ring_rot=3_000_000)
    store, c = api.compact_unitigs(recs, k)
    rounds = _assert_rounds(2 * n, 2 * n)
    print(f"chromosome: {c.describe()}; rounds {rounds} in {RC.round_limits(2 * n, 2 * n)}")
    assert c.closed_walks == c.unitigs == 1 and c.longest_unitig_kmers == c.distinct_kmers == n and c.windows == n + 1_000_000
    data, off = store.arrays()
    assert off.tolist() == [0, n + k - 1] and data.tobytes() == unitig.encode()
    cmp = api.compare_kmer_sets(recs, store, k)
    assert cmp.equal and cmp.occurrences_b == cmp.distinct_b == n


def test_a_ring_of_two_to_the_twenty(gpu):
    """C = 2^21 exactly: the last doubling window is the whole list."""
    k, n = 31, 1 << 20
    rec = RC.ring_record(_random_ring(n, 20), k)
    store, c = api.compact_unitigs([rec], k)
    assert RC.log2_ceil(2 * n) == 21 and 2 * c.distinct_kmers == 1 << 21
    rounds = _assert_rounds(2 * n, 2 * n)
    print(f"2^20 ring: {c.describe()}; rounds {rounds} in {RC.round_limits(2 * n, 2 * n)}")
    assert c.closed_walks == c.unitigs == 1 and c.longest_unitig_kmers == c.distinct_kmers == n
    assert store.arrays()[0].tobytes() == rec.encode()
    cmp = api.compare_kmer_sets([rec], store, k)
    assert cmp.equal and cmp.occurrences_b == cmp.distinct_b == n


@pytest.fixture(scope="module")
def plasmid_rings():
    rings = RC.plasmids(50_000, 50)
    lens = np.bincount([len(c) for c in rings], minlength=401)
    assert lens[:20].sum() == 0 and lens[20:].min() > 0 and min(lens[L] for L in (63, 64, 65, 255, 256, 257)) >= 50
    return rings


def _assert_store_is(store, want):
    data, off = store.arrays()
    assert np.array_equal(off, np.concatenate([[0], np.cumsum([len(s) for s in want])]).astype(np.uint64))
    assert data.tobytes() == "".join(want).encode()


def test_a_plasmid_collection_comes_out_as_it_went_in(gpu, plasmid_rings):
    """50 000 disjoint rings of 20 .. 400 bases, each one record: 100 000 cycles in one list, every length around the wave and the
    workgroup many times over; ids ascend along each walk and the store is the input."""
    k = 31
    recs = [RC.ring_record(c, k) for c in plasmid_rings]
    n = sum(len(c) for c in plasmid_rings)
    store, c = api.compact_unitigs(recs, k)
    _assert_rounds(2 * n, 2 * n)
    assert c.closed_walks == c.unitigs == 50_000 and c.distinct_kmers == c.windows == n and c.longest_unitig_kmers == 400
    _assert_store_is(store, recs)


def test_a_plasmid_collection_behind_arcs(gpu, plasmid_rings):
    """The same rings, each behind the reverse complement of an arc of a third of it: every walk runs against its ring's record."""
    k = 31
    both = [RC.ring_with_arc(c, k, len(c) // 2, len(c) // 3, 0) for c in plasmid_rings]
    recs = [r for pair, _ in both for r in pair]
    n = sum(len(c) for c in plasmid_rings)
    store, c = api.compact_unitigs(recs, k)
    _assert_rounds(2 * n, 2 * n)
    assert c.records == 100_000 and c.closed_walks == c.unitigs == 50_000 and c.distinct_kmers == n
    _assert_store_is(store, [u for _, u in both])


# ---- downstream: the join, the finish, the command line ----
def _flat(tigs):
    return np.cumsum([len(t) for t in tigs]).astype(np.uint64), np.concatenate([np.asarray(t, np.uint32) for t in tigs])


def test_closed_unitigs_are_self_loops_of_the_join_and_isolated_components_of_the_finish(gpu, oracle):
    import gpu_props

    k = 31
    recs = T.world("even", k)[0]
    unitigs, stats, closed, _, _ = T.compacted("even", k)
    store, _ = api.compact_unitigs(recs, k)
    assert store.sequences() == unitigs
    want = FA.graph_dict(unitigs, k)
    G = api.Bigraph.from_sequences(store.arrays(), k)
    ex = G.export()
    _assert_graph(ex, want, "rings")
    loops = ex["edge_from"] == ex["edge_to"]
    assert loops[0::2].tolist() == closed and loops[1::2].tolist() == closed and loops.sum() == 2 * 17  # one self-loop edge pair each
    assert (ex["mirror"][ex["edge_from"][loops]] != ex["edge_from"][loops]).all()                       # ... on a node that is not its own mirror
    assert len(ex["mirror"]) == 2 * 17 + 4 * 17  # nothing is joined: a node pair per ring, two per chain
    arrays = (ex["mirror"], ex["edge_from"], ex["edge_to"], ex["edge_weight"])
    # reference order: the oracle's tigs on the exported arrays
    g_cfg, e_cfg = api.GreedytigAlgorithmConfiguration.new(1, k), api.EulertigAlgorithmConfiguration(k)
    greedy = api.GreedytigAlgorithm.compute_tigs(api.Bigraph.from_edges(*arrays), g_cfg)
    assert greedy == oracle.OracleGraph.from_arrays(*arrays).compute_greedytigs(k)[0]
    euler = api.EulertigAlgorithm.compute_tigs(api.Bigraph.from_edges(*arrays), e_cfg)
    assert euler == oracle.OracleGraph.from_arrays(*arrays).compute_eulertigs(k)
    assert len(greedy) == len(euler) == len(unitigs) and sorted(len(t) for t in greedy) == [1] * len(unitigs)
    # device order: valid tigs that spell the input's k-mer set
    for algorithm, cfg in ((api.GreedytigAlgorithm, api.GreedytigAlgorithmConfiguration(1, k, euler_mode=api.EulerMode.Device)),
                           (api.EulertigAlgorithm, api.EulertigAlgorithmConfiguration(k, euler_mode=api.EulerMode.Device))):
        G = api.Bigraph.from_sequences(store.arrays(), k)
        tigs = algorithm.compute_tigs(G, cfg)
        cum, dummy_kmers = gpu_props.check_tigs(gpu, G, *_flat(tigs), k)
        assert len(tigs) == len(unitigs) and dummy_kmers == 0 and cum == stats["unitig_characters"]
        text = api.write_walks_fasta(G, tigs, unitigs, k).decode()
        spelled = [l for l in text.splitlines() if l and not l.startswith(">")]
        cmp = api.compare_kmer_sets(recs, spelled, k)
        assert cmp.equal and cmp.occurrences_b == cmp.distinct_b == stats["distinct_kmers"]


def _cli(*a):
    return subprocess.run([sys.executable, "-m", "matchtigs_amd", *a], capture_output=True, text=True, cwd=str(ROOT), timeout=600)


def test_one_pass_through_the_product(gpu, tmp_path):
    k = 31
    recs = T.world("even", k)[0]
    unitigs = T.compacted("even", k)[0]
    p = {n: str(tmp_path / n) for n in ("rings.fa", "u.fa", "g.fa", "e.fa", "g2.fa", "e2.fa")}
    Path(p["rings.fa"]).write_text(FA.fasta_text(recs, width=70))
    r = _cli("--seq-in", p["rings.fa"], "-k", str(k), "--unitigs-fa-out", p["u.fa"], "--greedytigs-fa-out", p["g.fa"], "--eulertigs-fa-out",
             p["e.fa"], "--verify")
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stderr.count("k-mer sets equal") == 2 and "17 closed" in r.stderr, r.stderr[-3000:]
    assert Path(p["u.fa"]).read_text().split("\n")[1::2] == unitigs
    r = _cli("--fa-in", p["u.fa"], "-k", str(k), "--greedytigs-fa-out", p["g2.fa"], "--eulertigs-fa-out", p["e2.fa"])
    assert r.returncode == 0, r.stderr[-3000:]
    for a, b in (("g.fa", "g2.fa"), ("e.fa", "e2.fa")):
        assert Path(p[a]).read_bytes() == Path(p[b]).read_bytes() and len(Path(p[a]).read_bytes()) > sum(map(len, unitigs)), f"{a} differs from {b}"
