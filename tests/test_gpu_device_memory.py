"""The device stage of the matching path gives back to the device arena what it took (api.device_arena_stats: live_bytes). A DeviceGraph
created, stepped (classify, search over all sources, resident claim replay) and deleted; a second identical step on a live DeviceGraph,
which reuses the arrays it keeps by capacity; a search over a quarter of the sources and then over all, which grows the overflow and
post-pass lists once; and the one-shot compute_tigs_np -- the single-use path: search arrays dropped before the replay, pairs taken
over by the finish. The edge cache belongs to the graph, so every case ends with Bigraph.release_device_cache(). G-csr graphs of a few
thousand unitigs at k = 31 (8:8 blocks, lists of searchable sources) and k = 300 (16-bit weights, no such lists), the empty graph and
one ring (every node balanced: no source). Every call is warmed once (test_gpu_compact_memory.py's _gives_back) and holds its answer
to the oracle's, as test_gpu_parity.py does: candidate lists, ordered pairs, tigs.

Not reached here: the retry of the candidate pool in device_pairs (the first pool, two keys per source plus the waves' chunk slack, holds
the candidates of graphs this small, as far as reading shows); the graphs are not enlarged to force it."""
import gc

import numpy as np
import pytest

from matchtigs_amd import api, synth, torch_glue
from test_gpu_compact_memory import _gives_back

pytestmark = pytest.mark.gpu
SHAPES = ["k31", "k300", "empty", "ring"]
WITH_SOURCES = ["k31", "k300"]


@pytest.fixture(scope="module")
def gpu(product_lib):
    import torch

    if product_lib.mtg_device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("these tests need a GPU: the matchtigs_amd hot path has no CPU fallback")
    return torch


def _ring(n, k):
    """n unitigs in one closed walk: unitig u runs node 2u -> node 2(u + 1), its mirror back."""
    u = np.arange(n, dtype=np.uint32)
    head, tail = 2 * u, 2 * ((u + 1) % n)
    e_from = np.stack([head, tail ^ 1], axis=1).reshape(-1)
    e_to = np.stack([tail, head ^ 1], axis=1).reshape(-1)
    return synth.Bigraph(np.arange(2 * n, dtype=np.uint32) ^ 1, e_from, e_to, np.full(2 * n, 3, np.uint64), k)


def _shape(name):
    if name == "k31":
        return synth.g_csr(2000, seed=21, k=31)
    if name == "k300":
        return synth.g_csr(2000, seed=22, k=300, mean_weight=50.0)
    if name == "ring":
        return _ring(1500, 31)
    return synth.Bigraph(np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint64), 31)


@pytest.fixture(scope="module")
def cases(oracle):
    """Per shape the graph and the oracle's answers, computed once: sources, candidate lists, ordered pairs, tigs."""
    out = {}
    for name in SHAPES:
        bg = _shape(name)
        og = lambda: oracle.OracleGraph.from_arrays(bg.mirror, bg.edge_from, bg.edge_to, bg.edge_weight)
        on, off, keys, _ = og().candidate_lists(bg.k)
        out[name] = dict(bg=bg, sources=on, off=off, keys=keys, pairs=og().greedy_pairs_np(bg.k)[0], tigs=og().compute_greedytigs(bg.k)[0])
    assert len(out["empty"]["sources"]) == 0 and len(out["ring"]["sources"]) == 0 and out["ring"]["bg"].n_edges == 3000
    assert all(len(out[n]["sources"]) > 100 and len(out[n]["pairs"]) > 0 for n in WITH_SOURCES)
    return out


def _graph(bg):
    return api.Bigraph.from_edges(bg.mirror, bg.edge_from, bg.edge_to, bg.edge_weight)


def _search(dev, case, hi):
    """Candidate lists of the sources [0, hi) -> the buffers, once held to the oracle's lists."""
    bufs = torch_glue.run_sssp(dev, 0, hi)
    start, count, pool = torch_glue.candidates_to_numpy(bufs)
    off, keys = case["off"], case["keys"]
    assert np.array_equal(count.astype(np.uint64), np.diff(off)[:hi])
    got = [pool[int(s):int(s) + int(c)] for s, c in zip(start, count)]
    assert np.array_equal(np.concatenate(got) if got else np.zeros(0, np.uint64), keys[:int(off[hi])])
    return bufs


def _step(dev, case, first_hi=None):
    """classify, search (over [0, first_hi) first if given), resident claim replay: every answer equals the oracle's."""
    S = dev.classify(torch_glue.current_stream_ptr())
    on, _, _ = dev.classify_download()
    assert S == len(case["sources"]) and np.array_equal(on, case["sources"])
    if first_hi is not None:
        _search(dev, case, first_hi)
    bufs = _search(dev, case, S)
    n = dev.replay_claims_resident(bufs.start.data_ptr(), bufs.count.data_ptr(), bufs.pool.data_ptr(), torch_glue.current_stream_ptr())
    pairs = dev.download_resident_pairs()
    assert n == len(pairs) == len(case["pairs"])
    for f in ("out", "in", "dist"):
        assert np.array_equal(pairs[f], case["pairs"][f]), f


def _create_step_delete(case, first_hi=None):
    G = _graph(case["bg"])
    dev = api.DeviceGraph(G, case["bg"].k, reserve_work=False)
    _step(dev, case, first_hi)
    del dev
    G.release_device_cache()


@pytest.mark.parametrize("shape", SHAPES)
def test_create_step_delete(gpu, cases, shape):
    _gives_back(lambda: _create_step_delete(cases[shape]), lambda: _create_step_delete(cases[shape]))


@pytest.mark.parametrize("shape", WITH_SOURCES)
def test_a_second_step_takes_nothing_more(gpu, cases, shape):
    case = cases[shape]

    def run():
        G = _graph(case["bg"])
        dev = api.DeviceGraph(G, case["bg"].k, reserve_work=False)
        _step(dev, case)  # takes the arrays that are kept by capacity
        first_left = api.device_arena_stats(0)["live_bytes"]
        _step(dev, case)
        assert api.device_arena_stats(0)["live_bytes"] == first_left
        del dev
        G.release_device_cache()

    _gives_back(run, run)


@pytest.mark.parametrize("shape", WITH_SOURCES)
def test_a_growing_search_range(gpu, cases, shape):
    case = cases[shape]
    quarter = len(case["sources"]) // 4
    assert 0 < quarter < len(case["sources"])  # the lists sized for a quarter of the sources are too small for all: they grow once
    _gives_back(lambda: _create_step_delete(case, quarter), lambda: _create_step_delete(case, quarter))


@pytest.mark.parametrize("shape", SHAPES)
def test_the_one_shot_call(gpu, cases, shape):
    case = cases[shape]

    def run():
        G = _graph(case["bg"])
        lim, ed = api.GreedytigAlgorithm.compute_tigs_np(G, api.GreedytigAlgorithmConfiguration.new(1, case["bg"].k))
        want = case["tigs"]
        assert np.array_equal(lim, np.cumsum([len(t) for t in want], dtype=np.uint64))
        assert np.array_equal(ed, np.array([e for t in want for e in t], dtype=np.uint32))
        del lim, ed
        G.release_device_cache()
        gc.collect()

    _gives_back(run, run)
