"""abundance_ref.py -- the contract of the counted unitig compaction (mtg_compact_unitigs_counted) restated with Python
dicts and strings on top of compact_ref.py: abundance(x) = the windows whose k-mer is x or rc(x); S_m = the k-mers with abundance >= m;
creators and readings over ALL windows; items 2-7 of the compaction's contract over S_m. Independent of the device code; slow (small
inputs only). Not a test module."""
from __future__ import annotations

import compact_ref as R

SPECTRUM_BINS = 256


def abundances(records, k: int) -> dict:
    """canonical k-mer -> number of windows that show it or its reverse complement (a palindromic window counts once)."""
    count: dict[str, int] = {}
    for rec in records:
        rec = rec.upper()
        for i in range(len(rec) - k + 1):
            x = R.canonical(rec[i:i + k])
            count[x] = count.get(x, 0) + 1
    return count


def spectrum_of(count: dict) -> list:
    """[c] = distinct k-mers with abundance c for 1 <= c <= 254, [255] = those with 255 or more, [0] = 0."""
    spectrum = [0] * SPECTRUM_BINS
    for c in count.values():
        spectrum[min(c, SPECTRUM_BINS - 1)] += 1
    return spectrum


def compact_counted(records, k: int, m: int):
    """-> (unitigs in contract order, statistics dict as compact_ref.compact's, per unitig whether its walk is closed, abundance dict:
    distinct_all, distinct_kept, dropped, max_abundance, kept_occurrences, spectrum[256], unitig_sums)."""
    if k < 2:
        raise ValueError("k must be >= 2")
    if m < 1:
        raise ValueError("min_abundance must be >= 1")
    creator, reading_all, windows, _, _, _ = R.graph_of(records, k)  # item 1 over all windows
    count = abundances(records, k)
    assert set(count) == set(creator) and sum(count.values()) == windows
    reading = {x: w for x, w in reading_all.items() if count[x] >= m}  # S_m, in creator order
    out: dict[str, list] = {}
    into: dict[str, list] = {}
    edges = []
    for x, w in reading.items():  # item 2 over S_m: the removed k-mers take their edges with them
        for o, s in ((0, w), (1, R.revcomp(w))):
            edges.append((x, o))
            out.setdefault(s[:-1], []).append((x, o))
            into.setdefault(s[1:], []).append((x, o))

    def succ(e):
        v = R.edge_string(reading, e)[1:]
        return out[v][0] if R.passable(v, out, into) else None

    def pred(e):
        v = R.edge_string(reading, e)[:-1]
        return into[v][0] if R.passable(v, out, into) else None

    seen = set()
    emitted = []
    for e0 in edges:  # item 4
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
        j = min(range(len(walk)), key=lambda i: creator[walk[i][0]])  # item 5
        if walk[j][1] != 0:
            continue
        if closed:
            walk = walk[j:] + walk[:j]
        emitted.append((creator[walk[j][0]] if not closed else creator[walk[0][0]], walk, closed))
    emitted.sort(key=lambda t: t[0])
    assert sorted(e[0] for _, w, _ in emitted for e in w) == sorted(reading), "every kept k-mer lies on exactly one emitted walk"
    unitigs = [R.edge_string(reading, w[0]) + "".join(R.edge_string(reading, e)[-1] for e in w[1:]) for _, w, _ in emitted]  # item 6
    stats = {
        "records": len(records),
        "characters": sum(len(r) for r in records),
        "windows": windows,
        "distinct_kmers": len(reading),
        "unitigs": len(unitigs),
        "unitig_characters": sum(len(u) for u in unitigs),
        "closed_walks": sum(1 for _, _, c in emitted if c),
        "longest_unitig_kmers": max((len(w) for _, w, _ in emitted), default=0),
    }
    abundance = {
        "distinct_all": len(count),
        "distinct_kept": len(reading),
        "dropped": len(count) - len(reading),
        "max_abundance": max(count.values(), default=0),
        "kept_occurrences": sum(count[x] for x in reading),
        "spectrum": spectrum_of(count),
        "unitig_sums": [sum(count[e[0]] for e in w) for _, w, _ in emitted],
    }
    assert sum(abundance["unitig_sums"]) == abundance["kept_occurrences"]
    return unitigs, stats, [c for _, _, c in emitted], abundance
