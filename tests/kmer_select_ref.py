"""The k-mer selection's contract (compact_device.hip; DESIGN.md 37, mtg_compact_unitigs_selected) restated in plain Python on top of
compact_ref.py, abundance_ref.py and kmer_color_ref.py: string windows, dictionaries, Python integers as masks. It knows no slots and
no ids. Independent of the device code; slow (small inputs only). Not a test module.

pieces(records): the records cut at whatever is outside ACGT, empty pieces dropped (what the readers hand to the library).
filter_counts(records, k): canonical k-mer -> the windows of the records that show it or its reverse complement (sub / int).
verdicts(...): canonical k-mer of S_m -> None (selected) or the first rule it fails.
compact_selected(...): the compaction of S_sel with creators and readings over the main windows, the statistics over S_m and the
selection's counts.
selection_lines(names, colours, selection): the `--selection-out` file."""
import re

from matchtigs_amd import synth

import abundance_ref as A
import compact_ref as R
import kmer_abundance_ref as KA
import kmer_color_ref as KC

RULES = ("forbid", "require", "carriers", "subtract", "intersect")
MAX_COLORS = 64
_NOT_ACGT = re.compile("[^ACGTacgt]+")


def pieces(records):
    return [p for r in records for p in _NOT_ACGT.split(r) if p]


def filter_counts(records, k):
    """(a palindromic window counts once: the dictionary is keyed by the canonical form)"""
    return A.abundances(pieces(records), k)


def windows_of(records, k):
    return sum(max(0, len(p) - k + 1) for p in pieces(records))


def check(require=0, forbid=0, min_colors=0, max_colors=MAX_COLORS, A_=1, B=1, n_colors=0):
    if require & forbid:
        raise ValueError("require and forbid overlap")
    if min_colors > max_colors or max_colors > MAX_COLORS:
        raise ValueError("min_colors > max_colors")
    if A_ < 1 or B < 1:
        raise ValueError("a filter abundance below 1")
    if (require | forbid) >> n_colors if n_colors else (require or forbid or min_colors > 0 or max_colors < MAX_COLORS):
        raise ValueError("a colour the call does not have")


def first_failure(mask, sub, inter, require, forbid, min_colors, max_colors, A_, B):
    """sub / inter: the k-mer's counts, None where the role has no record."""
    if mask & forbid:
        return "forbid"
    if mask & require != require:
        return "require"
    if not min_colors <= bin(mask).count("1") <= max_colors:
        return "carriers"
    if sub is not None and sub >= A_:
        return "subtract"
    if inter is not None and inter < B:
        return "intersect"
    return None


def compact_kept(records, k, keep):
    """compact_ref.compact's items 2-7 over the k-mers x with keep(x), creators and readings over ALL windows of `records` ->
    (unitigs in contract order, statistics dict, closed flags)."""
    creator, reading_all, windows, _, _, _ = R.graph_of(records, k)
    reading = {x: w for x, w in reading_all.items() if keep(x)}  # in creator order
    out, into, edges = {}, {}, []
    for x, w in reading.items():
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

    seen, emitted = set(), []
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
        j = min(range(len(walk)), key=lambda i: creator[walk[i][0]])
        if walk[j][1] != 0:
            continue
        if closed:
            walk = walk[j:] + walk[:j]
        emitted.append((creator[walk[0][0]] if closed else creator[walk[j][0]], walk, closed))
    emitted.sort(key=lambda t: t[0])
    assert sorted(e[0] for _, w, _ in emitted for e in w) == sorted(reading), "every selected k-mer lies on exactly one emitted walk"
    unitigs = [R.edge_string(reading, w[0]) + "".join(R.edge_string(reading, e)[-1] for e in w[1:]) for _, w, _ in emitted]
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
    assert stats["distinct_kmers"] == stats["unitig_characters"] - (k - 1) * stats["unitigs"]
    return unitigs, stats, [c for _, _, c in emitted]


def compact_selected(records, k, m=1, record_colors=None, n_colors=0, require=0, forbid=0, min_colors=0, max_colors=MAX_COLORS, subtract=None,
                     A_=1, intersect=None, B=1):
    """records: the main records (ACGT, either case). subtract / intersect: None or lists of strings (anything outside ACGT cuts).
    -> dict: unitigs, stats, closed, abundance (abundance_ref's scalars and spectrum over S_m, unitig_sums and kmer_counts over the
    output), colours (None without colours; kmer_colors over the output, per_color / shared / occupancy over S_m), selection."""
    check(require, forbid, min_colors, max_colors, A_, B, n_colors if record_colors is not None else 0)
    count = A.abundances(records, k)
    masks = KC.kmer_masks(records, record_colors, k) if record_colors is not None else {}
    sub = filter_counts(subtract, k) if subtract is not None and pieces(subtract) else None
    inter = filter_counts(intersect, k) if intersect is not None and pieces(intersect) else None
    s_m = [x for x in count if count[x] >= m]
    verdict = {x: first_failure(masks.get(x, 0), None if sub is None else sub.get(x, 0), None if inter is None else inter.get(x, 0), require, forbid,
                                min_colors, max_colors, A_, B) for x in s_m}
    selected = {x for x in s_m if verdict[x] is None}
    unitigs, stats, closed = compact_kept(records, k, lambda x: x in selected)
    ordered = [synth.canonical(w) for w in KA.windows(unitigs, k)]
    assert sorted(ordered) == sorted(selected)
    kmer_counts = [count[x] for x in ordered]
    cuts = [0]
    for u in unitigs:
        cuts.append(cuts[-1] + len(u) - k + 1)
    abundance = {
        "distinct_all": len(count),
        "distinct_kept": len(s_m),
        "max_abundance": max(count.values(), default=0),
        "kept_occurrences": sum(count[x] for x in s_m),
        "spectrum": A.spectrum_of(count),
        "unitig_sums": [sum(kmer_counts[lo:hi]) for lo, hi in zip(cuts[:-1], cuts[1:])],
        "kmer_counts": kmer_counts,
    }
    colours = None
    if record_colors is not None:
        KC.check_colors(record_colors, n_colors, len(records))
        per_color, shared, occupancy = KC.statistics([masks[x] for x in s_m], n_colors)
        colours = {"n_colors": n_colors, "kmer_colors": [masks[x] for x in ordered], "per_color": per_color, "shared": shared, "occupancy": occupancy}
    selection = {"input_kmers": len(s_m), "selected": len(selected), "selected_occurrences": sum(count[x] for x in selected)}
    for rule in RULES:
        selection["rejected_" + rule] = sum(1 for x in s_m if verdict[x] == rule)
    assert sum(selection["rejected_" + rule] for rule in RULES) + selection["selected"] == len(s_m)
    for name, recs, counts in (("subtract", subtract, sub), ("intersect", intersect, inter)):
        selection[name + "_windows"] = windows_of(recs, k) if recs is not None else 0
        selection[name + "_hits"] = sum(n for x, n in counts.items() if x in count) if counts is not None else 0
    selection["per_color_selected"] = [sum(1 for x in selected if (masks[x] >> c) & 1) for c in range(n_colors)] if record_colors is not None else []
    return {"unitigs": unitigs, "stats": stats, "closed": closed, "abundance": abundance, "colours": colours, "selection": selection,
            "selected_set": selected, "verdict": verdict}


def selection_lines(names, colours, selection):
    """The `--selection-out` file: name<TAB>k-mers for the input, what the abundance threshold kept, the five rules and the selected
    set; then per colour its file, its k-mers in S_m and its selected k-mers. `input`: the distinct k-mers of all windows."""
    lines = [f"input\t{selection['distinct_all']}", f"abundance_kept\t{selection['input_kmers']}"]
    lines += [f"{rule}\t{selection['rejected_' + rule]}" for rule in RULES]
    lines.append(f"selected\t{selection['selected']}")
    if colours is not None:
        lines += [f"color\t{names[c]}\t{colours['per_color'][c]}\t{selection['per_color_selected'][c]}" for c in range(colours["n_colors"])]
    return lines
