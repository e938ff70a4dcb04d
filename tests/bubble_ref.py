"""bubble_ref.py -- the contract of the simplified unitig compaction (mtg_compact_unitigs_simplified) restated with Python
dicts and strings on top of tip_clip_ref.py. Independent of the device code; slow (small inputs only). Not a test module.

Over the current set T an OPEN walk e_1 .. e_n has the tail node u (the prefix of e_1 as read) and the head node v (the suffix of
e_n); its mirror runs from rc(v) to rc(u) and is the same arm. It is a CANDIDATE ARM iff n < L_bub, u != rc(u), v != rc(v), u != v
and u != rc(v). The candidates with one (u, v) -- an arm and its mirror once -- are a BUNDLE. Arm a is better than b iff
sum_a n_b > sum_b n_a (sum: the abundances of the arm's k-mers), on equality the one with the smaller min(creator(e_1), creator(e_n)).
Every arm a but the best B goes iff sum_B n_a >= R sum_a n_B. A round decides tips, isolated walks and arms on one snapshot and
removes them together; rounds repeat until one removes nothing or `rounds` have run."""
from __future__ import annotations

import abundance_ref as A
import color_split_ref as CS
import compact_ref as R
import kmer_color_ref as KC
import tip_clip_ref as T

BUBBLE_KEYS = ("arms", "arm_kmers", "removed_occurrences")


def arm_ends(reading, walk):
    """(u, v): the tail node and the head node of an open walk."""
    return R.edge_string(reading, walk[0])[:-1], R.edge_string(reading, walk[-1])[1:]


def excluded(u, v):
    """A self-mirror end, a loop at one node, or a hairpin: never an arm."""
    return u == R.revcomp(u) or v == R.revcomp(v) or u == v or u == R.revcomp(v)


def bundles_of(reading, walks, l_bub):
    """-> ({key: [walk]}, the short open walks turned away as a loop at one node or a hairpin). key = the smaller of (u, v) and
    (rc(v), rc(u)); of a walk and its mirror the first met stands for both."""
    bundles, turned_away, seen = {}, 0, set()
    for walk, closed in walks:
        ident = frozenset(e[0] for e in walk)
        if ident in seen:
            continue
        seen.add(ident)
        if closed or len(walk) >= l_bub:
            continue
        u, v = arm_ends(reading, walk)
        if excluded(u, v):
            turned_away += u != R.revcomp(u) and v != R.revcomp(v)
            continue
        bundles.setdefault(min((u, v), (R.revcomp(v), R.revcomp(u))), []).append(walk)
    return bundles, turned_away


def one_round(reading, count, creator, l_tip, l_iso, l_bub, ratio, info=None):
    """-> (the k-mers to remove, the cleaning counters of tip_clip_ref.one_round, the bubble counters) on the snapshot `reading`.
    info: a dict that takes max_bundle (the arms of the largest bundle) and turned_away (short open loops and hairpins)."""
    gone, c = T.one_round(reading, count, l_tip, l_iso)
    b = dict.fromkeys(BUBBLE_KEYS, 0)
    if not l_bub:
        return gone, c, b
    walks, _, _ = T.walks_over(reading)
    bundles, turned_away = bundles_of(reading, walks, l_bub)
    if info is not None:
        info["max_bundle"] = max(info.get("max_bundle", 0), max((len(a) for a in bundles.values()), default=0))
        info["turned_away"] = info.get("turned_away", 0) + turned_away
    popped = set()
    for arms in bundles.values():
        facts = []
        for w in arms:
            kmers = [e[0] for e in w]
            assert len(set(kmers)) == len(kmers)
            facts.append((sum(count[x] for x in kmers), len(w), min(creator[kmers[0]], creator[kmers[-1]]), kmers))
        best = facts[0]
        for f in facts[1:]:
            if f[0] * best[1] > best[0] * f[1] or (f[0] * best[1] == best[0] * f[1] and f[2] < best[2]):
                best = f
        assert sum(1 for f in facts if f[2] == best[2]) == 1, "arms of one bundle share no k-mer"
        for f in facts:
            if f is not best and best[0] * f[1] >= ratio * f[0] * best[1]:
                assert not (set(f[3]) & gone), "an arm is never a tip or isolated"
                assert not (set(f[3]) & popped)
                popped.update(f[3])
                b["arms"] += 1
                b["arm_kmers"] += f[1]
                b["removed_occurrences"] += f[0]
    return gone | popped, c, b


def compact_simplified(records, k, pop_bubbles=0, bubble_ratio=1, clip_tips=0, remove_isolated=0, rounds=1, m=1, record_colors=None,
                       n_colors=0, split=False, info=None):
    """-> tip_clip_ref.compact_cleaned's tuple plus the bubbles dict (arms, arm_kmers, removed_occurrences)."""
    if k < 2:
        raise ValueError("k must be >= 2")
    if m < 1:
        raise ValueError("min_abundance must be >= 1")
    if not 1 <= rounds <= 64:
        raise ValueError("rounds must be in 1..64")
    if not 1 <= bubble_ratio <= 255:
        raise ValueError("bubble_ratio must be in 1..255")
    if split and record_colors is None:
        raise ValueError("split needs colours")
    creator, reading_all, windows, _, _, _ = R.graph_of(records, k)
    count = A.abundances(records, k)
    mask_of = None
    if record_colors is not None:
        KC.check_colors(record_colors, n_colors, len(records))
        mask_of = KC.kmer_masks(records, record_colors, k)
    reading = {x: w for x, w in reading_all.items() if count[x] >= m}
    kept = len(reading)
    kept_occurrences = sum(count[x] for x in reading)
    cleaning = {"rounds_run": 0, "tips": 0, "tip_kmers": 0, "isolated": 0, "isolated_kmers": 0, "removed_occurrences": 0}
    bubbles = dict.fromkeys(BUBBLE_KEYS, 0)
    if clip_tips or remove_isolated or pop_bubbles:
        while cleaning["rounds_run"] < rounds and reading:
            gone, c, b = one_round(reading, count, creator, clip_tips, remove_isolated, pop_bubbles, bubble_ratio, info)
            cleaning["rounds_run"] += 1
            for name, v in c.items():
                cleaning[name] += v
            for name, v in b.items():
                bubbles[name] += v
            if not gone:
                break
            reading = {x: w for x, w in reading.items() if x not in gone}
    emitted = T.emitted_walks(reading, creator, mask_of if split else None)
    unitigs = [R.edge_string(reading, w[0]) + "".join(R.edge_string(reading, e)[-1] for e in w[1:]) for w, _ in emitted]
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
    assert kept - len(reading) == cleaning["tip_kmers"] + cleaning["isolated_kmers"] + bubbles["arm_kmers"]
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
    assert sum(abundance["unitig_sums"]) == kept_occurrences - cleaning["removed_occurrences"] - bubbles["removed_occurrences"]
    colours = classes = None
    if mask_of is not None:
        kmer_colors = [mask_of[e[0]] for w, _ in emitted for e in w]
        per_color, shared, occupancy = KC.statistics(kmer_colors, n_colors)
        colours = {"n_colors": n_colors, "kmer_colors": kmer_colors, "per_color": per_color, "shared": shared, "occupancy": occupancy}
        classes = CS.class_dictionary([len(w) for w, _ in emitted], kmer_colors)
        assert not split or classes["n_runs"] == len(unitigs)
    return unitigs, stats, [c for _, c in emitted], abundance, colours, classes, cleaning, bubbles


# ---- inputs the tests share ----
def other_base(rng, c):
    return rng.choice([x for x in "ACGT" if x != c])


def snp_record(rng, g, k, p, seen=None):
    """g[p - k + 1 : p + k] with base p changed: k k-mers between two nodes of g. Drawn again, up to 200 times, until its k - 1 inner
    nodes are new on both strands (`seen`: the canonical (k-1)-mers in use, updated); at a tiny k there may be no such record: the
    last draw is taken."""
    assert k - 1 <= p and p + k <= len(g)
    if seen is None:
        seen = {R.canonical(g[i:i + k - 1]) for i in range(len(g) - k + 2)}
    for _ in range(200):
        rec = g[p - k + 1:p] + other_base(rng, g[p]) + g[p + 1:p + k]
        nodes = [R.canonical(rec[j:j + k - 1]) for j in range(1, k)]
        if len(set(nodes)) == k - 1 and not (set(nodes) & seen) and all(v != R.revcomp(v) for v in nodes):
            break
    seen.update(nodes)
    return rec


def plant_snps(rng, g, k, n, dna=None):
    """-> (records, sites): g plus n SNP records (snp_record) at sites at least 2 k + 2 apart and as far from g's ends; every third
    record is given as its reverse complement. dna is unused (the signature of plant_tips)."""
    step = (len(g) - 2 * (2 * k + 2)) // n
    assert step >= 2 * k + 2, "the sites must lie apart"
    seen = {R.canonical(g[i:i + k - 1]) for i in range(len(g) - k + 2)}
    records, sites = [g], []
    for i in range(n):
        p = 2 * k + 2 + i * step
        rec = snp_record(rng, g, k, p, seen)
        records.append(R.revcomp(rec) if i % 3 == 0 else rec)
        sites.append(p)
    return records, sites


def hand_cases(rng, dna, k=11):
    """name -> (records, k, keyword arguments of compact_simplified): the hand-derivable cases of test_bubble_ref.py, which states what
    each must give. g is always the first record, so that its k-mers keep the smallest creators."""
    cases = {}
    g = T.genome(rng, max(400, 14 * k), max(k, 8))  # (a tiny k has no such genome: the cases then only compare)
    p = len(g) // 2
    L = k + 1
    seen = {R.canonical(g[i:i + k - 1]) for i in range(len(g) - k + 2)}
    snp = snp_record(rng, g, k, p, seen)
    cases["snp_short_L"] = ([g, snp], k, dict(pop_bubbles=k))
    cases["snp_tie"] = ([g, snp], k, dict(pop_bubbles=L))
    cases["snp_variant_wins"] = ([g, snp, snp, R.revcomp(snp)], k, dict(pop_bubbles=L))
    cases["ratio2_even"] = ([g, snp], k, dict(pop_bubbles=L, bubble_ratio=2))
    cases["ratio2_3to1"] = ([g, g, g, snp], k, dict(pop_bubbles=L, bubble_ratio=2))
    # a one-base deletion: g without base dp, k - 1 k-mers beside g's k (dp: the first base from p on that differs from both of its
    # neighbours -- inside a run of equal bases a deletion shifts the run and changes fewer k-mers)
    dp = next(i for i in range(p, len(g)) if g[i - 1] != g[i] != g[i + 1])
    deletion = g[dp - k + 1:dp] + g[dp + 1:dp + k]
    cases["deletion_goes"] = ([g, g, deletion], k, dict(pop_bubbles=L))  # means 2 against 1
    cases["deletion_wins"] = ([g, deletion, deletion], k, dict(pop_bubbles=L))  # means 1 against 2
    for _ in range(200):  # a third allele at the site
        snp2 = snp_record(rng, g, k, p, set(seen))
        if snp2[k - 1] != snp[k - 1]:
            break
    assert snp2[k - 1] not in (snp[k - 1], g[p])
    cases["three_alleles"] = ([g, snp, snp2], k, dict(pop_bubbles=L))
    # a long arm beside two short ones: g's own stretch replaced by an insertion (k + 7 k-mers), a SNP, and g
    third = next(c for c in "ACGT" if c not in (g[p], snp[k - 1]))
    insertion = g[p - k + 1:p] + third + dna(6) + third + g[p + 1:p + k]
    cases["long_arm"] = ([g, snp, insertion], k, dict(pop_bubbles=L))
    # a hairpin u x rc(u) hanging off g
    u = g[p:p + k - 1]
    hairpin = u + other_base(rng, g[p + k - 1]) + dna(2) + R.revcomp(u)
    cases["hairpin"] = ([g, hairpin], k, dict(pop_bubbles=4 * k))
    # a ring with a SNP
    ring = T.genome(rng, 6 * k + 7, k)
    ring_rec = ring + ring[:k - 1]
    ring_snp = snp_record(rng, ring_rec, k, 3 * k)
    cases["ring_snp"] = ([ring_rec, ring_snp], k, dict(pop_bubbles=L))
    # a SNP next to a planted tip of 4 k-mers
    at = p + 3 * k
    tip = g[at:at + k - 1] + other_base(rng, g[at + k - 1]) + dna(3)
    cases["snp_and_tip"] = ([g, snp, tip], k, dict(pop_bubbles=L, clip_tips=k))
    # a bubble whose stem is another bubble's arm: `wide` changes two bases of g that lie k - 1 apart (every window over either: an
    # arm of 2 k - 1 k-mers beside g's), `inner` a base between them (its k windows all hold a changed base of wide, and so do its
    # two end nodes: a bubble inside wide's arm, which is three walks until inner is gone)
    q0 = p - 5 * k
    q1 = q0 + k - 1
    wide = g[q0 - k + 1:q0] + other_base(rng, g[q0]) + g[q0 + 1:q1] + other_base(rng, g[q1]) + g[q1 + 1:q1 + k]
    mid = k - 1 + k // 2
    inner = wide[mid - k + 1:mid] + other_base(rng, wide[mid]) + wide[mid + 1:mid + k]
    cases["nested_one_round"] = ([g, g, wide, wide, inner], k, dict(pop_bubbles=4 * k, rounds=1))
    cases["nested_two_rounds"] = ([g, g, wide, wide, inner], k, dict(pop_bubbles=4 * k, rounds=3))
    cases["_parts"] = {"g": g, "snp": snp, "snp2": snp2, "deletion": deletion, "insertion": insertion, "ring_rec": ring_rec, "ring_snp": ring_snp,
                       "tip": tip, "wide": wide, "inner": inner, "p": p, "dp": dp}
    return cases


def fuzz_input(rng, k):
    """One tiny input for the fuzz: a random backbone, SNP-like variants (some sites with two of them), hairpins and loose reads, each
    given one to three times, on either strand."""
    def dna(n):
        return "".join(rng.choice("ACGT") for _ in range(n))

    g = dna(rng.randrange(3 * k + 6, 5 * k + 12))
    records = [g] * rng.randrange(1, 3)
    for _ in range(rng.randrange(1, 4)):
        p = rng.randrange(k - 1, len(g) - k + 1)
        for _ in range(rng.choice((1, 1, 2, 3))):
            rec = g[p - k + 1:p] + other_base(rng, g[p]) + g[p + 1:p + k]
            records += [rec if rng.random() < 0.5 else R.revcomp(rec)] * rng.randrange(1, 4)
    if rng.random() < 0.4:
        p = rng.randrange(0, len(g) - k + 1)
        u = g[p:p + k - 1]
        records.append(u + dna(rng.randrange(1, 4)) + R.revcomp(u))
    if rng.random() < 0.3:
        records.append(dna(rng.randrange(k, 2 * k)))
    rng.shuffle(records)
    return records


FUZZ_SEED, FUZZ_INPUTS = 20251, 300


def fuzz_cases():
    """[(records, k, keyword arguments)]: the 300 inputs of the fuzz (the CPU test module asserts what they must contain)."""
    import random

    rng = random.Random(FUZZ_SEED)
    cases = []
    for i in range(FUZZ_INPUTS):
        k = (4, 5, 6)[i % 3]
        cases.append((fuzz_input(rng, k), k, dict(pop_bubbles=rng.choice((k + 1, 2 * k)), bubble_ratio=rng.choice((1, 2)), rounds=rng.randrange(1, 5),
                                                  clip_tips=rng.choice((0, k)), m=rng.choice((1, 1, 2)))))
    return cases
