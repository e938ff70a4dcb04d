"""The coloured k-mer set's contract (compact_device.hip, kmer_query_device.hip) restated in plain Python on top of
abundance_ref.py, compact_ref.py, kmer_query_ref.py and kmer_abundance_ref.py: string windows, dictionaries, Python integers as masks.
Independent of the device code; slow (small inputs only). Not a test module.

kmer_masks(records, record_colors, k): canonical k-mer -> the mask with bit c for every colour c that has a window showing the k-mer or
its reverse complement, over ALL windows.
compact_colored(records, record_colors, n_colors, k, m): abundance_ref.compact_counted's outputs plus, over the kept k-mers, kmer_colors
(window order of the unitigs), per_color, shared, occupancy.
class_colors(index, colors, k): canonical k-mer -> the mask of its first window in window order.
color_hits(index, colors, n_colors, query, k): per query record kmers / valid / found (kmer_query_ref.query) and per_color[r][c]; per_window
over the global base positions of the query, 0 wherever no found window starts."""
from matchtigs_amd import synth

import abundance_ref as A
import kmer_abundance_ref as KA
import kmer_query_ref as Q

MAX_COLORS = 64


def check_colors(record_colors, n_colors, n_records):
    if not 1 <= n_colors <= MAX_COLORS:
        raise ValueError(f"{n_colors} colours")
    if len(record_colors) != n_records:
        raise ValueError(f"{len(record_colors)} colours for {n_records} records")
    if any(not 0 <= c < n_colors for c in record_colors):
        raise ValueError("a colour outside 0 .. n_colors - 1")


def kmer_masks(records, record_colors, k):
    masks = {}
    for rec, c in zip(records, record_colors):
        rec = rec.upper()
        for i in range(len(rec) - k + 1):
            x = synth.canonical(rec[i:i + k])
            masks[x] = masks.get(x, 0) | (1 << c)
    return masks


def statistics(masks, n_colors):
    """per_color, shared, occupancy over an iterable of masks (one per kept k-mer)."""
    masks = list(masks)
    per_color = [sum(1 for m in masks if (m >> c) & 1) for c in range(n_colors)]
    shared = [[sum(1 for m in masks if (m >> i) & 1 and (m >> j) & 1) for j in range(n_colors)] for i in range(n_colors)]
    occupancy = [0] * (MAX_COLORS + 1)
    for m in masks:
        occupancy[bin(m).count("1")] += 1
    return per_color, shared, occupancy


def compact_colored(records, record_colors, n_colors, k, m=1):
    """-> (unitigs, statistics dict, closed flags, abundance dict -- all four abundance_ref.compact_counted's --, colours dict: n_colors,
    kmer_colors, per_color, shared, occupancy)."""
    check_colors(record_colors, n_colors, len(records))
    unitigs, stats, closed, abundance = A.compact_counted(records, k, m)
    masks = kmer_masks(records, record_colors, k)
    kmer_colors = [masks[synth.canonical(w)] for w in KA.windows(unitigs, k)]  # every kept k-mer once: the unitigs spell S_m
    assert len(kmer_colors) == abundance["distinct_kept"] and all(kmer_colors)
    per_color, shared, occupancy = statistics(kmer_colors, n_colors)
    assert occupancy[0] == 0 and sum(occupancy) == len(kmer_colors) and all(shared[c][c] == per_color[c] for c in range(n_colors))
    return unitigs, stats, closed, abundance, {"n_colors": n_colors, "kmer_colors": kmer_colors, "per_color": per_color, "shared": shared,
                                              "occupancy": occupancy}


def class_colors(index, colors, k):
    ws = KA.windows(index, k)
    if len(ws) != len(colors):
        raise ValueError(f"{len(colors)} masks for {len(ws)} windows")
    out = {}
    for w, x in zip(ws, colors):
        out.setdefault(synth.canonical(w), int(x))  # the first occurrence wins
    return out


def color_hits(index, colors, n_colors, query, k):
    if not 1 <= n_colors <= MAX_COLORS or any(int(x) >> n_colors for x in colors):
        raise ValueError("a colour outside 0 .. n_colors - 1")
    color = class_colors(index, colors, k)
    out = Q.query(set(color), query, k)
    out = {f: out[f] for f in ("kmers", "valid", "found")}
    out.update(per_color=[], per_window=[0] * sum(len(s) for s in query))
    base = 0
    for r, s in enumerate(query):
        row, hits = [0] * n_colors, 0
        for i in range(len(s) - k + 1):
            w = s[i:i + k]
            if all(c in Q.ACGT for c in w) and synth.canonical(w.upper()) in color:
                m = color[synth.canonical(w.upper())]
                hits += 1  # (a mask of 0 is a mask: found, no column)
                out["per_window"][base + i] = m
                for c in range(n_colors):
                    row[c] += (m >> c) & 1
        assert hits == out["found"][r]
        out["per_color"].append(row)
        base += len(s)
    return out


def jaccard(per_color, shared):
    """|i and j| / |i or j|; None where both colours are empty."""
    n = len(per_color)
    return [[shared[i][j] / (per_color[i] + per_color[j] - shared[i][j]) if per_color[i] + per_color[j] - shared[i][j] else None
             for j in range(n)] for i in range(n)]


def matrix_lines(names, colours):
    """The `--color-matrix-out` file: header, one row per colour, the closing occupancy row."""
    n = colours["n_colors"]
    lines = ["\t".join(["color", "kmers"] + list(names))]
    lines += ["\t".join([names[i], str(colours["per_color"][i])] + [str(x) for x in colours["shared"][i]]) for i in range(n)]
    lines.append("\t".join(["#occupancy"] + [str(x) for x in colours["occupancy"][1:n + 1]]))
    return lines


def unitig_color_lines(unitigs, kmer_colors, k):
    """The `--unitig-colors-out` file: per unitig its k-mers' masks, left to right, as runs count:hexmask."""
    lines, at = [], 0
    for u in unitigs:
        runs = []
        for m in kmer_colors[at:at + len(u) - k + 1]:
            if runs and runs[-1][1] == m:
                runs[-1][0] += 1
            else:
                runs.append([1, m])
        lines.append(" ".join(f"{n}:{m:x}" for n, m in runs))
        at += len(u) - k + 1
    return lines


def query_color_lines(names, record_names, result):
    """The `--query-colors-out` file."""
    lines = ["\t".join(["record", "kmers", "valid", "found"] + list(names))]
    lines += ["\t".join([name, str(n), str(v), str(f)] + [str(x) for x in row]) for name, n, v, f, row in zip(
        record_names, result["kmers"], result["valid"], result["found"], result["per_color"])]
    return lines
