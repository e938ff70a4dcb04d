"""The monochromatic compaction and the colour classes (compact_device.hip) restated in plain Python on top of
compact_ref.py, abundance_ref.py and kmer_color_ref.py: string windows, dictionaries, Python integers as masks. Independent of the
device code; slow (small inputs only). Not a test module.

compact_split(records, record_colors, n_colors, k, m): abundance_ref.compact_counted's walk over S_m with item 3 replaced -- a node
is passable iff it is not its own mirror, has in-degree 1 and out-degree 1, AND the k-mer that enters it and the k-mer that leaves it
have equal masks --, and kmer_color_ref.compact_colored's outputs over the split unitigs.
compact_classes(..., split): either compaction plus class_dictionary of its store.
class_dictionary(unitig_kmers, kmer_colors): the classes in first-appearance order from dicts; class_dictionary_np: the same from
np.unique, for stores too large for the dict walk to be worth its time.
class_lines / unitig_class_lines: the `--color-classes-out` and `--unitig-color-classes-out` files."""
import numpy as np

import abundance_ref as A
import compact_ref as R
import kmer_abundance_ref as KA
import kmer_color_ref as KC


def passable_split(v, out, into, mask_of):
    """Item 3 of the split compaction."""
    return R.passable(v, out, into) and mask_of[into[v][0][0]] == mask_of[out[v][0][0]]


def compact_split(records, record_colors, n_colors, k, m=1):
    """-> (unitigs, statistics dict, closed flags, abundance dict, colours dict) as kmer_color_ref.compact_colored, over the split walks."""
    KC.check_colors(record_colors, n_colors, len(records))
    if k < 2:
        raise ValueError("k must be >= 2")
    if m < 1:
        raise ValueError("min_abundance must be >= 1")
    creator, reading_all, windows, _, _, _ = R.graph_of(records, k)  # item 1 over all windows
    count = A.abundances(records, k)
    mask_of = KC.kmer_masks(records, record_colors, k)
    reading = {x: w for x, w in reading_all.items() if count[x] >= m}  # S_m, in creator order
    out, into, edges = {}, {}, []
    for x, w in reading.items():  # item 2 over S_m
        for o, s in ((0, w), (1, R.revcomp(w))):
            edges.append((x, o))
            out.setdefault(s[:-1], []).append((x, o))
            into.setdefault(s[1:], []).append((x, o))

    def succ(e):
        v = R.edge_string(reading, e)[1:]
        return out[v][0] if passable_split(v, out, into, mask_of) else None

    def pred(e):
        v = R.edge_string(reading, e)[:-1]
        return into[v][0] if passable_split(v, out, into, mask_of) else None

    seen, emitted = set(), []
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
        emitted.append((creator[walk[0][0]] if closed else creator[walk[j][0]], walk, closed))
    emitted.sort(key=lambda t: t[0])
    assert sorted(e[0] for _, w, _ in emitted for e in w) == sorted(reading), "every kept k-mer lies on exactly one emitted walk"
    assert all(len({mask_of[e[0]] for e in w}) == 1 for _, w, _ in emitted), "every split unitig is monochromatic"
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
    assert stats["distinct_kmers"] == stats["unitig_characters"] - (k - 1) * stats["unitigs"]
    abundance = {
        "distinct_all": len(count),
        "distinct_kept": len(reading),
        "dropped": len(count) - len(reading),
        "max_abundance": max(count.values(), default=0),
        "kept_occurrences": sum(count[x] for x in reading),
        "spectrum": A.spectrum_of(count),
        "unitig_sums": [sum(count[e[0]] for e in w) for _, w, _ in emitted],
        "kmer_counts": [count[e[0]] for _, w, _ in emitted for e in w],
    }
    kmer_colors = [mask_of[e[0]] for _, w, _ in emitted for e in w]
    assert all(kmer_colors)
    per_color, shared, occupancy = KC.statistics(kmer_colors, n_colors)
    return unitigs, stats, [c for _, _, c in emitted], abundance, {"n_colors": n_colors, "kmer_colors": kmer_colors, "per_color": per_color,
                                                                   "shared": shared, "occupancy": occupancy}


def class_dictionary(unitig_kmers, kmer_colors):
    """-> dict: masks, kmers, runs, first (per class, first-appearance order), kmer_class (per window), n_runs."""
    ids, masks, kmers, runs, first, kmer_class = {}, [], [], [], [], []
    i = 0
    for n in unitig_kmers:
        prev = None  # (kept masks are never 0, and None equals no mask: a unitig's first window opens a run)
        for _ in range(n):
            x = kmer_colors[i]
            if x not in ids:
                ids[x] = len(masks)
                masks.append(x)
                kmers.append(0)
                runs.append(0)
                first.append(i)
            c = ids[x]
            kmers[c] += 1
            runs[c] += x != prev
            kmer_class.append(c)
            prev = x
            i += 1
    assert i == len(kmer_colors) and sum(kmers) == i and first == sorted(set(first))
    return {"masks": masks, "kmers": kmers, "runs": runs, "first": first, "kmer_class": kmer_class, "n_runs": sum(runs)}


def class_dictionary_np(unitig_kmers, kmer_colors):
    """class_dictionary from np.unique over the masks and run heads from the unitig lengths, as numpy arrays of the library's dtypes."""
    masks = np.asarray(kmer_colors, np.uint64)
    n = np.asarray(unitig_kmers, np.int64)
    assert int(n.sum()) == len(masks)
    if not len(masks):
        z = np.zeros(0, np.uint64)
        return {"masks": z, "kmers": z, "runs": z, "first": z, "kmer_class": np.zeros(0, np.uint32), "n_runs": 0}
    values, index, inverse, counts = np.unique(masks, return_index=True, return_inverse=True, return_counts=True)
    order = np.argsort(index)  # classes by their first window
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    kmer_class = rank[inverse]
    head = np.ones(len(masks), bool)
    head[1:] = masks[1:] != masks[:-1]
    head[(np.cumsum(n) - n)] = True
    runs = np.bincount(kmer_class[head], minlength=len(order))
    return {"masks": values[order], "kmers": counts[order].astype(np.uint64), "runs": runs.astype(np.uint64), "first": index[order].astype(np.uint64),
            "kmer_class": kmer_class.astype(np.uint32), "n_runs": int(head.sum())}


def compact_classes(records, record_colors, n_colors, k, m=1, split=False):
    """-> (unitigs, statistics, closed, abundance, colours, classes). The abundance dict gains kmer_counts in either case."""
    if split:
        out = compact_split(records, record_colors, n_colors, k, m)
    else:
        out = KC.compact_colored(records, record_colors, n_colors, k, m)
        count = A.abundances(records, k)
        out[3]["kmer_counts"] = [count[R.canonical(w)] for w in KA.windows(out[0], k)]
    classes = class_dictionary([len(u) - k + 1 for u in out[0]], out[4]["kmer_colors"])
    assert not split or classes["n_runs"] == len(out[0])
    return out + (classes,)


def class_lines(classes):
    """The `--color-classes-out` file."""
    lines = ["class\tmask\tcarriers\tkmers\truns"]
    lines += [f"{c}\t{int(m):x}\t{bin(int(m)).count('1')}\t{int(n)}\t{int(r)}" for c, (m, n, r) in enumerate(zip(
        classes["masks"], classes["kmers"], classes["runs"]))]
    return lines


def unitig_class_lines(unitigs, kmer_class, k):
    """The `--unitig-color-classes-out` file: per unitig its k-mers' classes, left to right, as runs count:class."""
    lines, at = [], 0
    for u in unitigs:
        runs = []
        for c in kmer_class[at:at + len(u) - k + 1]:
            if runs and runs[-1][1] == c:
                runs[-1][0] += 1
            else:
                runs.append([1, int(c)])
        lines.append(" ".join(f"{n}:{c}" for n, c in runs))
        at += len(u) - k + 1
    return lines


# ---- the fixture: what the colour cases of test_gpu_kmer_color.py do not reach ----
def _cyclic(unit, k, first, n):
    """The record that shows the n cyclic k-mers first, first + 1, ... of the periodic sequence unit unit unit ..."""
    p = len(unit)
    text = unit * (2 + (k + n) // p + 1)
    return text[first % p:first % p + k + n - 1]


def split_cases(k, dna, colours):
    """-> ([(record, colour)], the four units) -- five numbered cases, each on sequence of its own (dna(n): n random bases; colours:
    three colours). The periodic records have period p = k + 6, so each is a closed walk of p k-mers on its own:
    1. unit 1 in colours[0] plus colours[1] over 3 of its k-mers: chains of k + 3 and 3 k-mers, none closed;
    2. unit 2 in colours[0], colours[1] over k-mers 4 .. 6 given as the reverse complement, colours[2] over k-mers p - 1 and 0, across
       the wrap-around: chains of 3, 3, k - 2 and 2 k-mers;
    3. the covering record BEFORE the periodic one and as its reverse complement: its stretch owns the smallest creator, the unsplit
       unitig follows it, and the rest of the cycle, read as the periodic record has it, is the reverse complement of a stretch of it;
    4. unit 4 in one colour alone: one closed walk, split or not;
    5. two records of one colour that share their second half: three unitigs of one mask around a branching node."""
    p = k + 6
    units = [dna(p) for _ in range(4)]
    out = [(_cyclic(units[0], k, 0, p), colours[0]), (_cyclic(units[0], k, 5, 3), colours[1])]
    out += [(_cyclic(units[1], k, 0, p), colours[0]), (R.revcomp(_cyclic(units[1], k, 4, 3)), colours[1]), (_cyclic(units[1], k, p - 1, 2), colours[2])]
    out += [(R.revcomp(_cyclic(units[2], k, 7, 3)), colours[1]), (_cyclic(units[2], k, 0, p), colours[0])]
    out += [(_cyclic(units[3], k, 0, p), colours[2])]
    shared = dna(k + 9)
    out += [(dna(k + 4) + shared, colours[2]), (dna(k + 2) + shared, colours[2])]
    return out, units
