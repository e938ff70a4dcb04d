"""compact_ref.py -- the contract of the unitig compaction (mtg_compact_unitigs) restated with Python dicts and
strings, item by item: creators and readings, the bigraph G(S) with mirror edges, passable nodes, maximal walks, leaders, emitted
orientation, start of closed walks, order, spelling, statistics. Independent of the device code and of synth.g_seq; slow (small
inputs only). Not a test module."""
from __future__ import annotations

_COMP = str.maketrans("ACGT", "TGCA")


def revcomp(s: str) -> str:
    return s.translate(_COMP)[::-1]


def canonical(s: str) -> str:
    r = revcomp(s)
    return s if s <= r else r


def graph_of(records, k: int):
    """Items 1 and 2: (creator, reading, windows, edges, out, into). An edge is (x, o): the canonical k-mer x read as reading(x)
    (o = 0) or as its reverse complement (o = 1); out / into map an oriented (k-1)-mer to the edges that leave / enter it."""
    creator: dict[str, int] = {}
    reading: dict[str, str] = {}
    pos = windows = 0
    for rec in records:
        rec = rec.upper()
        if set(rec) - set("ACGT"):
            raise ValueError("character outside ACGT")
        for i in range(len(rec) - k + 1):
            w = rec[i:i + k]
            windows += 1
            x = canonical(w)
            if x not in creator:  # (positions ascend: the first window seen is the smallest)
                creator[x] = pos + i
                reading[x] = w
        pos += len(rec)
    out: dict[str, list] = {}
    into: dict[str, list] = {}
    edges = []
    for x, w in reading.items():
        for o, s in ((0, w), (1, revcomp(w))):  # a palindromic k-mer: two edges with the same string, a double edge
            edges.append((x, o))
            out.setdefault(s[:-1], []).append((x, o))
            into.setdefault(s[1:], []).append((x, o))
    return creator, reading, windows, edges, out, into


def edge_string(reading, e) -> str:
    return reading[e[0]] if e[1] == 0 else revcomp(reading[e[0]])


def passable(v: str, out, into) -> bool:
    """Item 3."""
    return v != revcomp(v) and len(into.get(v, ())) == 1 and len(out.get(v, ())) == 1


def compact(records, k: int):
    """-> (unitigs in contract order, statistics dict, per unitig whether its walk is closed)."""
    if k < 2:
        raise ValueError("k must be >= 2")
    creator, reading, windows, edges, out, into = graph_of(records, k)

    def succ(e):
        v = edge_string(reading, e)[1:]
        return out[v][0] if passable(v, out, into) else None

    def pred(e):
        v = edge_string(reading, e)[:-1]
        return into[v][0] if passable(v, out, into) else None

    seen = set()
    emitted = []
    for e0 in edges:  # item 4: the maximal walk through e0
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
        # item 5: leader, direction, start
        j = min(range(len(walk)), key=lambda i: creator[walk[i][0]])
        if walk[j][1] != 0:
            continue  # the mirror walk holds reading(leader)
        if closed:
            walk = walk[j:] + walk[:j]
        emitted.append((creator[walk[0][0]] if closed else creator[walk[j][0]], walk, closed))
    emitted.sort(key=lambda t: t[0])
    on_walks = [e[0] for _, w, _ in emitted for e in w]
    assert sorted(on_walks) == sorted(reading), "every k-mer lies on exactly one emitted walk"
    unitigs = []
    for _, walk, _ in emitted:  # item 6
        unitigs.append(edge_string(reading, walk[0]) + "".join(edge_string(reading, e)[-1] for e in walk[1:]))
    stats = {  # item 7
        "records": len(records),
        "characters": sum(len(r) for r in records),
        "windows": windows,
        "distinct_kmers": len(reading),
        "unitigs": len(unitigs),
        "unitig_characters": sum(len(u) for u in unitigs),
        "closed_walks": sum(1 for _, _, c in emitted if c),
        "longest_unitig_kmers": max((len(w) for _, w, _ in emitted), default=0),
    }
    assert stats["distinct_kmers"] == stats["unitig_characters"] - (k - 1) * stats["unitigs"]
    return unitigs, stats, [c for _, _, c in emitted]
