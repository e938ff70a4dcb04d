"""The restatement of the monochromatic compaction and the colour classes (color_split_ref.py) against itself, on the
CPU: the split unitigs are monochromatic, spell S_m with every k-mer once and cannot be joined; with one colour the split changes
nothing; the dictionary from dicts equals the one from np.unique; and the fixture holds the five cases it was built for."""
import random

import numpy as np
import pytest

import color_split_ref as S
import compact_ref as CR
import kmer_abundance_ref as KA
import kmer_color_ref as KC
from test_gpu_kmer_color import KS, PALETTE, _case, _dna

CS = [3, 64]


def split_case(k, C):
    """-> (records, colours, the four periodic units): test_gpu_kmer_color.py's case plus color_split_ref.split_cases."""
    recs, colors = _case(k, C)
    rng = random.Random(900 + k)
    more, units = S.split_cases(k, lambda n: _dna(rng, n), PALETTE[C][:3] if C == 64 else [0, 1, 2])
    return recs + [r for r, _ in more], colors + [c for _, c in more], units


@pytest.fixture(scope="module", params=[(k, C) for k in KS for C in CS], ids=lambda p: f"k{p[0]}-C{p[1]}")
def case(request):
    k, C = request.param
    recs, colors, units = split_case(k, C)
    return k, C, recs, colors, units, {(m, split): S.compact_classes(recs, colors, C, k, m, split) for m in (1, 2) for split in (False, True)}


def _kmers_of(unit, k):
    return {CR.canonical((unit * 3)[i:i + k]) for i in range(len(unit))}


def _canon(unitig, k):
    return [CR.canonical(w) for w in KA.windows([unitig], k)]


@pytest.mark.parametrize("m", [1, 2])
def test_split_unitigs_are_monochromatic_spell_the_set_and_cannot_be_joined(case, m):
    k, C, recs, colors, _, want = case
    unsplit, split = want[(m, False)], want[(m, True)]
    masks = KC.kmer_masks(recs, colors, k)
    on = [x for u in split[0] for x in _canon(u, k)]
    assert len(on) == len(set(on)) and set(on) == {x for u in unsplit[0] for x in _canon(u, k)}  # S_m, each k-mer once
    assert all(len({masks[x] for x in _canon(u, k)}) == 1 for u in split[0])
    assert split[4]["kmer_colors"] == [masks[x] for x in on] and split[5]["n_runs"] == len(split[0])
    # no two can be joined: at either end of an open split unitig the node is not passable under the new item 3
    _, reading, _, _, _, _ = CR.graph_of(recs, k)
    kept = set(on)
    out, into = {}, {}
    for x in reading:
        if x in kept:
            for o, s in ((0, reading[x]), (1, CR.revcomp(reading[x]))):
                out.setdefault(s[:-1], []).append((x, o))
                into.setdefault(s[1:], []).append((x, o))
    for u, closed in zip(split[0], split[2]):
        ends = [u[:k - 1], u[-(k - 1):]]
        assert closed == all(S.passable_split(v, out, into, masks) for v in ends)
        if not closed:
            assert not any(S.passable_split(v, out, into, masks) for v in ends)
    # what is a function of the k-mer set does not move
    for f in ("distinct_all", "distinct_kept", "max_abundance", "kept_occurrences", "spectrum"):
        assert split[3][f] == unsplit[3][f]
    for f in ("per_color", "shared", "occupancy"):
        assert split[4][f] == unsplit[4][f]
    assert sum(split[3]["unitig_sums"]) == sum(unsplit[3]["unitig_sums"]) and len(split[0]) >= len(unsplit[0])


@pytest.mark.parametrize("k", KS)
def test_one_colour_splits_nothing(k):
    recs, colors, _ = split_case(k, 3)
    a, b = S.compact_classes(recs, [0] * len(recs), 1, k, 1, False), S.compact_classes(recs, [0] * len(recs), 1, k, 1, True)
    assert a == b and a[0] == CR.compact(recs, k)[0]
    assert a[5]["masks"] == [1] and a[5]["runs"] == [len(a[0])] and a[5]["first"] == [0] and set(a[5]["kmer_class"]) == {0}


@pytest.mark.parametrize("m", [1, 2])
@pytest.mark.parametrize("split", [False, True])
def test_the_dictionary_from_dicts_equals_numpy(case, m, split):
    k, C, _, _, _, want = case
    unitigs, colours, classes = want[(m, split)][0], want[(m, split)][4], want[(m, split)][5]
    n = [len(u) - k + 1 for u in unitigs]
    got = S.class_dictionary_np(n, colours["kmer_colors"])
    for f in ("masks", "kmers", "runs", "first", "kmer_class"):
        assert got[f].tolist() == classes[f], f
        assert got[f].dtype == (np.uint32 if f == "kmer_class" else np.uint64)
    assert got["n_runs"] == classes["n_runs"] == sum(classes["runs"]) and sum(classes["kmers"]) == sum(n)
    assert [classes["masks"][c] for c in classes["kmer_class"]] == colours["kmer_colors"]
    assert all(a < b for a, b in zip(classes["first"], classes["first"][1:])) and len(set(classes["masks"])) == len(classes["masks"])
    # the runs are the items `--unitig-colors-out` writes
    assert classes["n_runs"] == sum(len(l.split()) for l in KC.unitig_color_lines(unitigs, colours["kmer_colors"], k))
    assert S.unitig_class_lines(unitigs, classes["kmer_class"], k) == [
        " ".join(f"{item.split(':')[0]}:{classes['masks'].index(int(item.split(':')[1], 16))}" for item in l.split())
        for l in KC.unitig_color_lines(unitigs, colours["kmer_colors"], k)]


def test_the_cases_hold_what_they_are_for(case):
    """Counted at k >= 31. At k = 4 a period of 10 bases repeats its 3-mers and nearly every node branches, so the numbered cases do not
    form there; the fixture still splits a few unitigs, which is all that is asserted."""
    k, C, recs, colors, units, want = case
    unsplit, split = want[(1, False)], want[(1, True)]
    if k == 4:
        assert len(split[0]) > len(unsplit[0])
        return
    p = k + 6
    assert len(split[0]) > len(unsplit[0]) and sum(unsplit[2]) >= 2
    own = [_kmers_of(u, k) for u in units]
    assert all(len(s) == p for s in own)

    def chains(which, i):
        return sorted((len(u) - k + 1, c) for u, c in zip(which[0], which[2]) if set(_canon(u, k)) & own[i])

    assert all(chains(unsplit, i) == [(p, True)] for i in range(4))  # each unit: one closed walk of p k-mers of its own
    assert chains(split, 0) == [(3, False), (k + 3, False)]                            # 1
    assert chains(split, 1) == sorted([(2, False), (3, False), (3, False), (k - 2, False)])  # 2
    assert chains(split, 2) == [(3, False), (k + 3, False)]                            # 3 ...
    whole = next(u for u in unsplit[0] if set(_canon(u, k)) & own[2])
    flipped = [u for u in split[0] if set(_canon(u, k)) & own[2] and u not in whole + whole and CR.revcomp(u) in whole]
    assert len(flipped) == 1 and len(flipped[0]) - k + 1 == k + 3  # ... and the long chain is the reverse complement of a stretch
    across = [u for u in split[0] if set(_canon(u, k)) & own[1] and u not in next(w for w in unsplit[0] if set(_canon(w, k)) & own[1])]
    assert across  # 2: a chain that spells across the unsplit spelling's wrap-around
    assert chains(split, 3) == [(p, True)]                                              # 4
    last = [i for i, u in enumerate(split[0]) if recs[-1].upper().endswith(u) or recs[-2].upper().startswith(u) or recs[-1].upper().startswith(u)]
    classes = S.class_dictionary([len(u) - k + 1 for u in split[0]], split[4]["kmer_colors"])
    ids = {classes["kmer_class"][sum(len(u) - k + 1 for u in split[0][:i])] for i in last}
    assert len(last) == 3 and len(ids) == 1 and classes["runs"][ids.pop()] >= 3         # 5: three unitigs, one class
