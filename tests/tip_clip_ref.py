"""tip_clip_ref.py -- the contract of the cleaned unitig compaction (mtg_compact_unitigs_cleaned) restated with Python
dicts and strings on top of compact_ref.py, abundance_ref.py, kmer_color_ref.py and color_split_ref.py. Independent of the device
code; slow (small inputs only). Not a test module.

T starts as S_m. Over the oriented edges out(v) / into(v) of G(T), an OPEN walk e_1 .. e_n of the contract has two ends: its head
node (the suffix of e_n) and the head node of its mirror walk (the reverse complement of the prefix of e_1). For an end with head
node v: beyond = |out(v)|, beside = |into(v)| - 1; at a self-mirror node beyond = beside = |out(v)| - 1. FREE: beyond = beside = 0;
ANCHORED: beside >= 1; THROUGH: anything else. A TIP has n < L_tip, one free and one anchored end; an ISOLATED walk n < L_iso and
two free ends. A round decides every walk on one snapshot and removes the k-mers of the tips and the isolated walks; rounds repeat
until one removes nothing or R have run. The result is the counted / coloured / classed contract over the final T, creators,
readings, abundances and masks taken over all windows; with split the rounds decide on the unsplit walks."""
from __future__ import annotations

import abundance_ref as A
import color_split_ref as CS
import compact_ref as R
import kmer_color_ref as KC

FREE, ANCHORED, THROUGH = "free", "anchored", "through"


def graph_over(reading):
    """Item 2 of the compaction's contract over the k-mers of `reading` (canonical k-mer -> reading): (edges, out, into)."""
    out, into, edges = {}, {}, []
    for x, w in reading.items():
        for o, s in ((0, w), (1, R.revcomp(w))):
            edges.append((x, o))
            out.setdefault(s[:-1], []).append((x, o))
            into.setdefault(s[1:], []).append((x, o))
    return edges, out, into


def walks_over(reading, mask_of=None):
    """Item 4: every maximal walk of G(reading), the mirror of each included -> ([(walk, closed)], out, into). mask_of: the split
    rule of DESIGN.md 23 (a passable node's two k-mers have equal masks)."""
    edges, out, into = graph_over(reading)

    def passable(v):
        return R.passable(v, out, into) and (mask_of is None or mask_of[into[v][0][0]] == mask_of[out[v][0][0]])

    def succ(e):
        v = R.edge_string(reading, e)[1:]
        return out[v][0] if passable(v) else None

    def pred(e):
        v = R.edge_string(reading, e)[:-1]
        return into[v][0] if passable(v) else None

    seen, walks = set(), []
    for e0 in edges:
        if e0 in seen:
            continue
        start, closed = e0, False
        while True:
            p = pred(start)
            if p is None:
                break
            if p == e0:
                closed = True
                break
            start = p
        walk = [e0 if closed else start]
        while True:
            s = succ(walk[-1])
            if s is None or s == walk[0]:
                break
            walk.append(s)
        assert not (set(walk) & seen)
        seen.update(walk)
        walks.append((walk, closed))
    return walks, out, into


def end_state(v, out, into):
    """The state of the end whose head node is v."""
    if v == R.revcomp(v):
        beyond = beside = len(out.get(v, ())) - 1  # our own mirror leaves v
    else:
        beyond, beside = len(out.get(v, ())), len(into.get(v, ())) - 1
    assert beyond >= 0 and beside >= 0
    if beyond == 0 and beside == 0:
        return FREE
    return ANCHORED if beside >= 1 else THROUGH


def walk_ends(reading, walk, out, into):
    """The states of the two ends of an open walk: (its own head node, the head node of its mirror walk)."""
    head = R.edge_string(reading, walk[-1])[1:]
    mirror_head = R.revcomp(R.edge_string(reading, walk[0])[:-1])
    return end_state(head, out, into), end_state(mirror_head, out, into)


def verdict(reading, walk, closed, out, into, l_tip, l_iso):
    """None, "tip" or "isolated"."""
    if closed:
        return None
    n, ends = len(walk), sorted(walk_ends(reading, walk, out, into))
    if n < l_tip and ends == sorted((FREE, ANCHORED)):
        return "tip"
    if n < l_iso and ends == [FREE, FREE]:
        return "isolated"
    return None


def one_round(reading, count, l_tip, l_iso):
    """-> (the k-mers to remove, {tips, tip_kmers, isolated, isolated_kmers, removed_occurrences}) on the snapshot `reading`."""
    walks, out, into = walks_over(reading)
    gone, c = set(), {"tips": 0, "tip_kmers": 0, "isolated": 0, "isolated_kmers": 0, "removed_occurrences": 0}
    for walk, closed in walks:
        if walk[0][0] in gone:
            continue  # the mirror walk: the same k-mers, the same two ends, the same verdict
        v = verdict(reading, walk, closed, out, into, l_tip, l_iso)
        if v is None:
            continue
        assert len({e[0] for e in walk}) == len(walk)
        gone.update(e[0] for e in walk)
        c["tips" if v == "tip" else "isolated"] += 1
        c["tip_kmers" if v == "tip" else "isolated_kmers"] += len(walk)
        c["removed_occurrences"] += sum(count[e[0]] for e in walk)
    return gone, c


def emitted_walks(reading, creator, mask_of=None):
    """Items 4 and 5 over `reading`: [(walk, closed)] of the emitted walks in contract order."""
    walks, _, _ = walks_over(reading, mask_of)
    emitted = []
    for walk, closed in walks:
        j = min(range(len(walk)), key=lambda i: creator[walk[i][0]])
        if walk[j][1] != 0:
            continue  # the mirror walk holds reading(leader)
        if closed:
            walk = walk[j:] + walk[:j]
        emitted.append((creator[walk[0][0]] if closed else creator[walk[j][0]], walk, closed))
    emitted.sort(key=lambda t: t[0])
    assert sorted(e[0] for _, w, _ in emitted for e in w) == sorted(reading), "every k-mer of T lies on exactly one emitted walk"
    return [(w, c) for _, w, c in emitted]


def compact_cleaned(records, k, clip_tips=0, remove_isolated=0, rounds=1, m=1, record_colors=None, n_colors=0, split=False):
    """-> (unitigs, statistics dict, closed flags, abundance dict, colours dict or None, classes dict or None, cleaning dict). The
    dicts are those of abundance_ref / kmer_color_ref / color_split_ref over the final T, except that the abundance dict's scalars
    describe S_m; the cleaning dict: rounds_run, tips, tip_kmers, isolated, isolated_kmers, removed_occurrences."""
    if k < 2:
        raise ValueError("k must be >= 2")
    if m < 1:
        raise ValueError("min_abundance must be >= 1")
    if not 1 <= rounds <= 64:
        raise ValueError("rounds must be in 1..64")
    if split and record_colors is None:
        raise ValueError("split needs colours")
    creator, reading_all, windows, _, _, _ = R.graph_of(records, k)  # item 1 over all windows
    count = A.abundances(records, k)
    mask_of = None
    if record_colors is not None:
        KC.check_colors(record_colors, n_colors, len(records))
        mask_of = KC.kmer_masks(records, record_colors, k)
    reading = {x: w for x, w in reading_all.items() if count[x] >= m}  # T = S_m, in creator order
    kept = len(reading)
    kept_occurrences = sum(count[x] for x in reading)
    cleaning = {"rounds_run": 0, "tips": 0, "tip_kmers": 0, "isolated": 0, "isolated_kmers": 0, "removed_occurrences": 0}
    if clip_tips or remove_isolated:
        while cleaning["rounds_run"] < rounds and reading:
            gone, c = one_round(reading, count, clip_tips, remove_isolated)
            cleaning["rounds_run"] += 1
            for name, v in c.items():
                cleaning[name] += v
            if not gone:
                break
            reading = {x: w for x, w in reading.items() if x not in gone}
    emitted = emitted_walks(reading, creator, mask_of if split else None)
    unitigs = [R.edge_string(reading, w[0]) + "".join(R.edge_string(reading, e)[-1] for e in w[1:]) for w, _ in emitted]  # item 6
    stats = {
        "records": len(records),
        "characters": sum(len(r) for r in records),
        "windows": windows,
        "distinct_kmers": len(reading),
        "unitigs": len(unitigs),
        "unitig_characters": sum(len(u) for u in unitigs),
        "closed_walks": sum(1 for _, c in emitted if c),
        "longest_unitig_kmers": max((len(w) for w, _ in emitted), default=0),
    }
    assert stats["distinct_kmers"] == stats["unitig_characters"] - (k - 1) * stats["unitigs"]
    assert kept - len(reading) == cleaning["tip_kmers"] + cleaning["isolated_kmers"]
    abundance = {
        "distinct_all": len(count),
        "distinct_kept": kept,
        "dropped": len(count) - kept,
        "max_abundance": max(count.values(), default=0),
        "kept_occurrences": kept_occurrences,
        "spectrum": A.spectrum_of(count),
        "unitig_sums": [sum(count[e[0]] for e in w) for w, _ in emitted],
        "kmer_counts": [count[e[0]] for w, _ in emitted for e in w],
    }
    assert sum(abundance["unitig_sums"]) == kept_occurrences - cleaning["removed_occurrences"]
    colours = classes = None
    if mask_of is not None:
        kmer_colors = [mask_of[e[0]] for w, _ in emitted for e in w]
        per_color, shared, occupancy = KC.statistics(kmer_colors, n_colors)
        colours = {"n_colors": n_colors, "kmer_colors": kmer_colors, "per_color": per_color, "shared": shared, "occupancy": occupancy}
        classes = CS.class_dictionary([len(w) for w, _ in emitted], kmer_colors)
        assert not split or classes["n_runs"] == len(unitigs)
    return unitigs, stats, [c for _, c in emitted], abundance, colours, classes, cleaning


# ---- inputs the tests share ----
def genome(rng, n, k):
    """n bases in which no (k-1)-mer repeats on either strand and none is its own reverse complement: one open unitig at k.
    Greedy: every base is the first of a random order of ACGT that shows a new (k-1)-mer."""
    for _ in range(100):
        g, seen = "", set()
        while len(g) < n:
            for c in rng.sample("ACGT", 4):
                v = (g + c)[-(k - 1):]
                if len(g) + 1 < k - 1 or (R.canonical(v) not in seen and v != R.revcomp(v)):
                    break
            else:
                break  # a dead end: start again
            g += c
            if len(g) >= k - 1:
                seen.add(R.canonical(g[-(k - 1):]))
        if len(g) == n:
            return g
    raise AssertionError("no such sequence found")


def plant_tips(rng, g, k, n_tips, dna):
    """-> (records, the planted tips' k-mers in total): g plus n_tips records, each a tip of 1 .. k - 1 k-mers on g. Tip i hangs at a
    site of its own, at least k + 2 bases from the next (the stretch of g between two forks has no free end, whatever its length)
    and 2 k + 2 from g's ends (those two stretches do, and are longer than any tip length up to 2 k); even i leave g (k - 1 bases of g, a base that differs
    from g's, random bases), odd i enter it (the mirror image); every third is given as its reverse complement. dna(n): n random
    bases. A tip is drawn again, up to 200 times, until its (k-1)-mers are new on either strand, so that it touches nothing but its
    site (at a tiny k there may be no such tip: the last draw is taken)."""
    step = (len(g) - 2 * (2 * k + 2)) // n_tips
    assert step >= k + 2, "the sites must lie apart"
    seen = {R.canonical(g[i:i + k - 1]) for i in range(len(g) - k + 2)}
    records, total = [g], 0
    for i in range(n_tips):
        at = 2 * k + 2 + i * step  # the fork's node is g[at : at + k - 1]
        n = rng.randrange(1, k)
        node = g[at:at + k - 1]
        for _ in range(200):
            if i % 2 == 0:  # leaves g behind the node: differs from g[at + k - 1]
                rec = node + rng.choice([c for c in "ACGT" if c != g[at + k - 1]]) + dna(n - 1)
                nodes = [R.canonical(rec[j:j + k - 1]) for j in range(1, n + 1)]
            else:  # enters g in front of the node: differs from g[at - 1]
                rec = dna(n - 1) + rng.choice([c for c in "ACGT" if c != g[at - 1]]) + node
                nodes = [R.canonical(rec[j:j + k - 1]) for j in range(n)]
            if len(set(nodes)) == n and not (set(nodes) & seen) and all(v != R.revcomp(v) for v in nodes):
                break
        seen.update(nodes)
        assert len(rec) == k - 1 + n
        records.append(R.revcomp(rec) if i % 3 == 0 else rec)
        total += n
    return records, total


def hand_cases(rng, dna):
    """name -> (records, k, keyword arguments of compact_cleaned): the hand-derivable cases of test_tip_clip_ref.py, which states
    what each must give. dna(n): n random bases. g is always the first record, so that its k-mers keep their creators."""
    cases = {}
    k = 11
    g = genome(rng, 400, k)
    node = g[200:200 + k - 1]

    def off(c):
        return rng.choice([x for x in "ACGT" if x != c])

    tip6 = node + off(g[200 + k - 1]) + dna(5)  # 6 k-mers that leave g behind g[200 : 210]
    cases["tip6_stays"] = ([g, tip6], k, dict(clip_tips=6))
    cases["tip6_goes"] = ([g, tip6], k, dict(clip_tips=7))
    stem = node + off(g[200 + k - 1]) + dna(4)  # 5 k-mers, then a fork into twigs of 3 and 4 k-mers
    a = dna(1)
    twig3, twig4 = stem[-(k - 1):] + a + dna(2), stem[-(k - 1):] + off(a) + dna(3)
    cases["y_one_round"] = ([g, stem, twig3, twig4], k, dict(clip_tips=k, rounds=1))
    cases["y_two_rounds"] = ([g, stem, twig3, twig4], k, dict(clip_tips=k, rounds=2))
    cases["y_many_rounds"] = ([g, stem, twig3, twig4], k, dict(clip_tips=k, rounds=16))
    lone = dna(k + 3)
    cases["isolated_goes"] = ([g, lone], k, dict(remove_isolated=k))
    cases["isolated_stays"] = ([g, lone], k, dict(remove_isolated=4))
    short_stem = dna(k + 2)  # 3 k-mers in front of a fork of two arms of 3 k k-mers each
    b = dna(1)
    cases["stem_kept"] = ([short_stem + b + dna(3 * k), short_stem + off(b) + dna(3 * k)], k, dict(clip_tips=k, remove_isolated=k, rounds=4))
    merge_tail = dna(k + 2)  # the mirror image: two arms that merge into 3 k-mers
    cases["merge_kept"] = ([dna(3 * k) + b + merge_tail, dna(3 * k) + off(b) + merge_tail], k, dict(clip_tips=k, remove_isolated=k, rounds=4))
    cases["lone_palindrome"] = (["ACGT"], 4, dict(clip_tips=10, remove_isolated=10, rounds=4))
    ring = dna(3 * k + 7)
    ring_rec = ring + ring[:k - 1]
    at = 17
    ring_tip = ring_rec[at:at + k - 1] + off(ring_rec[at + k - 1]) + dna(3)  # 4 k-mers
    cases["ring_tip"] = ([ring_rec, ring_tip], k, dict(clip_tips=k))
    cases["_parts"] = {"g": g, "ring_rec": ring_rec, "stem": stem, "twig3": twig3, "twig4": twig4}
    return cases
