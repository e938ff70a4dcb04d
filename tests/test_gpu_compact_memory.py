"""A compaction gives back to the device arena what it took (api.device_arena_stats: live_bytes), on every way through the driver of
compact_device.hip: the exits without bases, without windows, with no k-mer behind the abundance filter and with nothing left after
a round; rounds that end because one removed nothing (with and without the extra pass that splits at colour changes) or because the
last allowed one removed something; closed walks in more than one ranking; bubble rounds with no short walk, with none that is an arm,
and with an arm that goes; and the classed calls. k = 5 and k = 34: the narrow and the wide insert, node keys with k - 1 <= 32 and
k - 1 > 32. Every case first states, on the restatement's answer, that its input reaches the branch it is named for; the device's
answer is then held to the restatement in every field (test_gpu_pop_bubbles.py's check for the simplified calls)."""
import gc
import random

import pytest

import bubble_ref as B
import compact_ref as R
import tip_clip_ref as T
from matchtigs_amd import api
from test_gpu_pop_bubbles import _call, _check, _dna

pytestmark = pytest.mark.gpu
KS = [5, 34]
SEEDS = {5: 3136, 34: 3134}  # (k = 5: the first seed from 3105 on whose random parts meet nothing else; every test asserts that they do not)


@pytest.fixture(scope="module")
def gpu(product_lib):
    import torch

    if product_lib.mtg_device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("these tests need a GPU: the compaction has no CPU path")
    return torch


def _gives_back(warm_up, check):
    """warm_up(): the device call alone; check(): the call again with its assertions -> check()'s result, once the arena's live bytes
    have been seen to be the same before and after it."""
    warm_up()  # (chunks taken from the driver, code objects loaded)
    gc.collect()
    before = api.device_arena_stats(0)["live_bytes"]
    out = check()
    after = api.device_arena_stats(0)["live_bytes"]
    assert after == before, f"the call left {after - before} bytes of the arena live"
    return out


def _simplified(records, k, **kw):
    """-> (the device's, the restatement's) of a simplified call, compared in every field."""
    return _gives_back(lambda: _call(records, k, **kw), lambda: _check(records, k, **kw))


def _plain(records, k):
    def check():
        unitigs, stats, closed = R.compact(records, k)
        store, c = api.compact_unitigs(records, k)
        assert store.sequences() == unitigs and c == api.Compaction(**stats) and c.closed_walks == sum(closed)
        return c

    return _gives_back(lambda: api.compact_unitigs(records, k), check)


def _classed(records, k, colors, n_colors, split):
    def check():
        unitigs, stats, _, ab, col, classes, _ = T.compact_cleaned(records, k, record_colors=colors, n_colors=n_colors, split=split)
        store, c, a, co, cc = api.compact_unitigs_colored_classes(records, k, colors, n_colors, split=split)
        assert store.sequences() == unitigs and c == api.Compaction(**stats)
        assert a.unitig_sums.tolist() == ab["unitig_sums"] and a.kmer_counts.tolist() == ab["kmer_counts"] and a.spectrum.tolist() == ab["spectrum"]
        assert co.kmer_colors.tolist() == col["kmer_colors"]
        for f in ("per_color", "shared", "occupancy"):
            assert getattr(co, f).tolist() == col[f], f
        for f in ("masks", "kmers", "runs", "first", "kmer_class"):
            assert getattr(cc, f).tolist() == classes[f], f
        return c

    return _gives_back(lambda: api.compact_unitigs_colored_classes(records, k, colors, n_colors, split=split), check)


def _parts(k):
    """g (one open unitig), [g, tip], [g, snp], a ring of its own, a hairpin on g and a lone record of two k-mers."""
    rng = random.Random(SEEDS[k])
    dna = _dna(rng)
    g = T.genome(rng, 6 * k + 12, k)
    tip = T.plant_tips(rng, g, k, 1, dna)[0]
    for _ in range(200):  # a ring that stays a closed walk of its own beside g and the tip (at k = 5 most draws touch them)
        ring = dna(2 * k + 3)
        ring += ring[:k - 1]
        if R.compact(tip + [ring], k)[2] == [False, False, False, True]:
            break
    p = len(g) // 2
    u = g[p:p + k - 1]
    return dict(g=g, tip=tip, snp=B.plant_snps(rng, g, k, 1)[0], ring=ring, hairpin=u + B.other_base(rng, g[p + k - 1]) + dna(2) + R.revcomp(u),
                lone=dna(k + 1))


@pytest.fixture(scope="module")
def parts():
    return {k: _parts(k) for k in KS}


@pytest.mark.parametrize("k", KS)
def test_the_exits_in_front_of_the_rounds(gpu, parts, k):
    p = parts[k]
    assert _plain([], k).records == 0  # no bases: no device call at all
    assert _plain([""], k).characters == 0
    assert _plain([p["g"][:k - 1]], k).windows == 0  # uploaded and packed, then no window
    _, want = _simplified(p["tip"], k, m=3, record_colors=[0, 1], n_colors=2)  # no k-mer occurs three times
    assert want[3]["distinct_all"] > 0 and want[3]["distinct_kept"] == 0
    _, want = _simplified([p["lone"]], k, remove_isolated=3, record_colors=[0], n_colors=1)  # the whole input is isolated
    assert want[1]["distinct_kmers"] == 0 and want[6]["rounds_run"] == 1 and want[6]["isolated_kmers"] == want[3]["distinct_kept"] > 0


@pytest.mark.parametrize("k", KS)
def test_the_ways_the_rounds_end(gpu, parts, k):
    p = parts[k]
    g = p["g"]
    halves, colors = [g, g[:len(g) // 2]], [0, 1]  # one unitig whose colour set changes half way
    for split in (False, True):  # the first round removes nothing; split: succ and rank once more on the kept node table
        _, want = _simplified(halves, k, clip_tips=k, record_colors=colors, n_colors=2, split=split)
        assert want[6]["rounds_run"] == 1 and want[6]["tips"] == 0 and want[1]["unitigs"] == (2 if split else 1)
    _, want = _simplified(p["tip"], k, clip_tips=k, rounds=1)  # the last allowed round removed something: the final pass follows
    assert want[6]["rounds_run"] == 1 and want[6]["tips"] == 1 and want[0] == [g]
    _, want = _simplified(p["tip"], k, clip_tips=k, rounds=3)  # the second round removes nothing
    assert want[6]["rounds_run"] == 2 and want[6]["tips"] == 1 and want[0] == [g]
    got, want = _simplified(p["tip"] + [p["ring"]], k, clip_tips=k, rounds=2)  # a closed walk in the rankings of both rounds
    assert want[6]["rounds_run"] == 2 and want[6]["tips"] == 1 and want[1]["closed_walks"] == 1 and got[1].closed_walks == 1


def _short_open_walks(records, k, l_bub):
    """Per short open walk of the input's unitigs, the walk and its mirror once: whether the restatement turns it away as an arm."""
    _, reading, _, _, _, _ = R.graph_of(records, k)
    walks, _, _ = T.walks_over(reading)
    seen, out = set(), []
    for walk, closed in walks:
        ident = frozenset(e[0] for e in walk)
        if ident not in seen and not closed and len(walk) < l_bub:
            out.append(B.excluded(*B.arm_ends(reading, walk)))
        seen.add(ident)
    return out


@pytest.mark.parametrize("k", KS)
def test_the_bubble_rounds(gpu, parts, k):
    p = parts[k]
    L = k + 3
    assert _short_open_walks([p["g"]], k, L) == []  # no list slot at all
    _, want = _simplified([p["g"]], k, pop_bubbles=L)
    assert want[7]["arms"] == 0 and want[6]["rounds_run"] == 1
    hair = [p["g"], p["hairpin"]]
    short = _short_open_walks(hair, k, L)
    assert short and all(short)  # list slots, every one a hole: no arm k-mer, no sums, no table
    _, want = _simplified(hair, k, pop_bubbles=L)
    assert want[7]["arms"] == 0
    _, want = _simplified(p["snp"], k, pop_bubbles=L, rounds=2)  # one arm goes, the second round finds nothing
    assert want[7]["arms"] == 1 and want[6]["rounds_run"] == 2 and want[0] == [p["g"]]


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("k", KS)
def test_the_classed_calls(gpu, parts, k, split):
    g = parts[k]["g"]
    c = _classed([g, g[:len(g) // 2], parts[k]["ring"]], k, [0, 1, 2], 3, split)
    assert c.unitigs == (3 if split else 2) and c.closed_walks == 1
