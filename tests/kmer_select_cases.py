"""The inputs of the k-mer selection's tests, shared by test_kmer_select_ref.py (CPU: the restatement's own assertions
run over every one of them) and test_gpu_kmer_select.py. Plain Python; not a test module.

The main records and their colours are test_gpu_kmer_color.py's (a genome in pieces of either strand and case, a run of short records
whose colours change inside a thread's run of 64 positions, a closed walk, records shorter than k, colour 63 in use). The filter
records are cut from the main ones, so that they hit: on either strand, in either case, some of them several times (for A and B up
to 3), with an `N` inside, beside records shorter than k and records of other bases that hit nothing."""
import random

import collision_cases as CC
import test_gpu_kmer_color as TC
from matchtigs_amd import synth

KS = TC.KS
COLORS = (1, 3, 64)
# per number of colours: (forbid, require) as colour lists -- colours that have windows (TC.PALETTE)
MASKS = {1: ([0], [0]), 3: ([2], [0]), 64: ([63, 17], [0, 32])}


def _dna(rng, n, letters="ACGT"):
    return "".join(rng.choice(letters) for _ in range(n))


def filters(k, recs):
    """-> (subtract records, intersect records, records without a hit)."""
    rng = random.Random(7000 + k)
    long_ones = [r.upper() for r in recs if len(r) >= k + 3]
    a, b, c, d = long_ones[0], long_ones[1], long_ones[2], long_ones[-1]
    subtract = [a, synth.revcomp(a).lower(), a[2:k + 2], b[:len(b) // 2] + "N" + b[len(b) // 2:], _dna(rng, k - 1), "", d.upper()]
    intersect = [c, synth.revcomp(c), b.lower(), a[1:], synth.revcomp(a[1:]), _dna(rng, k // 2), "NN" + d + "n"]
    intersect += [r for r in recs[10:50] if len(r) >= k][:12]
    main = {synth.canonical(r[i:i + k].upper()) for r in recs for i in range(len(r) - k + 1)}
    none = [_dna(rng, k - 1)]
    while len(none) < 4:  # (at k = 4 nearly every k-mer is in the main records: short records of A and T)
        s = _dna(rng, k + 2, "AT") if k == 4 else _dna(rng, k + 20)
        if not any(synth.canonical(s[i:i + k]) in main for i in range(len(s) - k + 1)):
            none.append(s)
    return subtract, intersect, none


def alternating(k, recs):
    """Filter records of k .. k + 5 bases with the role changing from record to record: a thread's run of 64 positions holds about
    64 / (k + 3) of them (at k = 4 nine or so, at k = 33 two)."""
    rng = random.Random(7100 + k)
    long_ones = [r.upper() for r in recs if len(r) >= k + 6]
    out = []
    for i in range(40):
        r = long_ones[i % len(long_ones)]
        at = rng.randint(0, len(r) - k - 5)
        s = r[at:at + k + rng.randint(0, 5)]
        out.append(("intersect" if i % 2 else "subtract", synth.revcomp(s) if i % 3 == 0 else s))
    return out


def rule_sets(k, C, recs):
    """-> [(name, keyword arguments of kmer_select_ref.compact_selected, filter_records for api.KmerSelection or None)]."""
    subtract, intersect, none = filters(k, recs)
    forbid, require = (sum(1 << c for c in cs) for cs in MASKS[C])
    out = [("trivial", {}, None), ("forbid", {"forbid": forbid}, None), ("require", {"require": require}, None)]
    if C > 1:
        out.append(("carriers", {"min_colors": 2, "max_colors": C - 1}, None))
    out += [(f"subtract-A{a}", {"subtract": subtract, "A_": a}, None) for a in (1, 2, 3)]
    out += [(f"intersect-B{b}", {"intersect": intersect, "B": b}, None) for b in (1, 2)]
    five = {"subtract": subtract[:3], "A_": 3, "intersect": intersect, "B": 1}
    if C > 1:
        five.update(forbid=1 << MASKS[C][0][0], require=1 << MASKS[C][1][0], min_colors=2 if C == 64 else 1, max_colors=3 if C == 64 else C - 1)
    out.append(("all-five", five, None))
    alt = alternating(k, recs)
    out.append(("alternating", {"subtract": [s for r, s in alt if r == "subtract"], "A_": 2, "intersect": [s for r, s in alt if r == "intersect"]}, alt))
    out.append(("empty-filter", {"subtract": [], "intersect": ["N", ""]}, None))
    out.append(("no-hit", {"subtract": none}, None))
    out.append(("everything-rejected", {"intersect": none}, None))
    return out


def grid():
    """-> [(k, C, m, rule set name)]: every rule set at every k with three colours and m = 1; one and 64 colours and m = 2 on fewer."""
    out = []
    for k in KS:
        names = [name for name, _, _ in rule_sets(k, 3, TC._case(k, 3)[0])]
        out += [(k, 3, 1, name) for name in names]
        out += [(k, 64, 2, name) for name in ("forbid", "require", "carriers", "all-five", "subtract-A2")] + [(k, 64, 1, "all-five")]
        out += [(k, 1, 2 if k == 31 else 1, name) for name in ("forbid", "require", "intersect-B2", "all-five")]
        out += [(k, 3, 2, name) for name in ("subtract-A1", "alternating")]
    return out


def case(k, C, name):
    recs, colors = TC._case(k, C)
    kwargs, filter_records = next((kw, fr) for n, kw, fr in rule_sets(k, C, recs) if n == name)
    return recs, colors, kwargs, filter_records


def collision_case():
    """k = 1025: the main record P + X + S; P + Y + S, whose windows that hold the whole block collide with the main record's in all 64
    hash bits and are other k-mers; and the main record again."""
    rng = random.Random(1025)
    p, s = _dna(rng, 40), _dna(rng, 40)
    return 1025, p + CC.X + s, p + CC.Y + s


SIZE_KS = (5, 9)


def size_case(k):
    """About 200 kb: ten thousand reads of 20 bases from a genome of 8 000 bases, over three colours, and a filter of four thousand
    reads (80 000 positions: five workgroups of 256 threads with 64 positions each). At k = 5 there are only 512 canonical k-mers, so
    the scans of the selection stay inside one tile of 2 048 items; k = 9 is the same input with some 8 000 k-mers before and more
    than 2 048 after the selection."""
    rng = random.Random(55)
    genome = _dna(rng, 8000)
    recs = []
    for _ in range(10000):
        at = rng.randint(0, 8000 - 20)
        recs.append(genome[at:at + 20] if rng.random() < 0.5 else synth.revcomp(genome[at:at + 20]))
    colors = [i % 3 for i in range(len(recs))]
    subtract = [genome[at:at + 20] for at in (rng.randint(0, 1500) for _ in range(2000))]
    intersect = [genome[at:at + 20] for at in (rng.randint(0, 7980) for _ in range(2000))]
    return recs, colors, subtract, intersect
