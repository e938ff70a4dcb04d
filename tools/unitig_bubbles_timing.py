"""unitig_bubbles_timing.py -- what calling variants from the bubbles of the unitig graph (`--bubbles-out`, mtg_unitig_bubbles;
DESIGN.md 38) costs, phase by phase, on the cost input of DESIGN.md 25 (tools/pop_bubbles_timing.py: the four haplotypes of G-seq plus
about 1 % of planted tips and about 1 % of planted SNP records, k = 31, m = 2), compacted with the tips clipped and nothing popped: the
uploads with the pack, keys + group + number, the allele kernel and the carrier kernel (HIP events), the download, the bubbles and
arms by kind, the bytes the allele kernel must move at the least and the peak of live device-arena bytes. The input has one colour, so
the carrier kernel is timed on made-up masks (every k-mer carried by all of --colors colours) in repetitions of their own. The
yardsticks run in the same process on the same graph: the link stage (`api.unitig_links`: it reads the same edge arrays), and a
grouping on the host -- numpy.unique over the canonical keys of the exported end-node pairs -- which must find the same bubbles and arms.

usage: python tools/unitig_bubbles_timing.py [--length 100000000] [--k 31] [--max-arm-kmers 62] [--colors 4] [--reps 3] [--device 0]
                                             [--out profiles/unitig_bubbles_gseq_1e8.json]
One JSON line per measurement (the first repetition also pays the arena's first chunks and is left out of the summary); --out writes
all of it as one JSON document."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def host_grouping(graph, kmers, L):
    """-> (bubbles, arms, seconds) by numpy on the exported graph: the contract's candidates and keys, numpy.unique over the keys."""
    ex = graph.export()
    U = len(kmers)
    t0 = time.perf_counter()
    mirror = ex["mirror"].astype(np.uint64)
    x, y = ex["edge_from"][:2 * U:2].astype(np.uint64), ex["edge_to"][:2 * U:2].astype(np.uint64)
    mx, my = mirror[x], mirror[y]
    cand = (kmers < np.uint64(L)) & (x != mx) & (y != my) & (x != y) & (x != my)
    key = np.minimum((x << np.uint64(32)) | y, (my << np.uint64(32)) | mx)[cand]
    _, counts = np.unique(key, return_counts=True)
    seconds = time.perf_counter() - t0
    return int((counts >= 2).sum()), int(counts[counts >= 2].sum()), seconds


def main() -> None:
    from clip_tips_timing import M
    from matchtigs_amd import api
    from pop_bubbles_timing import bubbled_arrays

    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=100_000_000)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--tips-per-cent", type=float, default=1.0)
    ap.add_argument("--snps-per-cent", type=float, default=1.0)
    ap.add_argument("--max-arm-kmers", type=int)
    ap.add_argument("--colors", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out")
    args = ap.parse_args()
    k, dev = args.k, args.device
    L = 2 * k if args.max_arm_kmers is None else args.max_arm_kmers

    data, off, n_tips, n_snps = bubbled_arrays(args.length, k, args.tips_per_cent, args.snps_per_cent)
    store, c, abundance, _, _, cleaning = api.compact_unitigs_cleaned((data, off), k, clip_tips=k, min_abundance=M, device_id=dev)
    del data, off
    U = len(store)
    graph = api.Bigraph.from_sequences(store.arrays(), k, dev)
    kmers = (np.diff(store.arrays()[1]) - np.uint64(k - 1)).astype(np.uint64)
    doc = {"tool": "unitig_bubbles_timing", "length": args.length, "haplotypes": 4, "k": k, "min_abundance": M, "clip_tips": k, "planted_tips": n_tips,
           "planted_snps": n_snps, "max_arm_kmers": L, "unitigs": U, "kmers": int(kmers.sum()), "nodes": graph.node_count(), "edges": graph.edge_count(),
           "bubbles": [], "bubbles_with_masks": [], "links": [], "host": []}

    def emit(kind, row):
        row = {f: (round(v, 3) if isinstance(v, float) else v) for f, v in row.items()}
        doc[kind].append(row)
        print(json.dumps({kind: row}), flush=True)

    found = None
    for rep in range(args.reps):
        t0 = time.perf_counter()
        got = api.unitig_bubbles(graph, store, k, L, kc=abundance.unitig_sums, device_id=dev)
        wall = time.perf_counter() - t0
        emit("bubbles", {"rep": rep, **api.last_unitig_bubbles_times(), "wall_ms": 1e3 * wall})
        assert found is None or all(np.array_equal(getattr(got, f), getattr(found, f)) for f in ("arm_off", "arm_unitig", "arm_strand", "prefix", "suffix"))
        found = got
    masks = np.full(int(kmers.sum()), (1 << args.colors) - 1, np.uint64)
    for rep in range(max(2, args.reps - 1)):
        t0 = time.perf_counter()
        got = api.unitig_bubbles(graph, store, k, L, kc=abundance.unitig_sums, kmer_colors=masks, n_colors=args.colors, device_id=dev)
        wall = time.perf_counter() - t0
        emit("bubbles_with_masks", {"rep": rep, "n_colors": args.colors, **api.last_unitig_bubbles_times(), "wall_ms": 1e3 * wall})
        assert np.array_equal(got.carried, np.repeat(got.arm_kmers[:, None], args.colors, axis=1)) and np.array_equal(got.arm_unitig, found.arm_unitig)
    del masks
    kinds = found.kinds()
    doc["describe"] = found.describe()
    doc["kinds"] = {name: kinds.count(name) for name in ("ref", "snp", "mnp", "ins", "del", "complex", "identical")}
    doc["arms_on_minus"] = int(found.arm_strand.sum())
    # what the allele kernel must move at the least: the packed bases of every other arm and of its reference arm once (suffix, prefix
    # and the span between them cover both records where the lengths agree), per arm its unitig, reference, strand and four offsets in,
    # three words out
    other = np.ones(len(found.arm_unitig), bool)
    other[found.arm_off[:-1].astype(np.int64)] = False
    first = np.repeat(found.arm_off[:-1], np.diff(found.arm_off).astype(np.int64)).astype(np.int64)
    bases = (found.arm_kmers[other].astype(np.int64) + found.arm_kmers[first][other].astype(np.int64) + 2 * (k - 1)).sum()
    doc["allele_min_bytes"] = int(bases // 4 + len(found.arm_unitig) * (4 + 4 + 1 + 4 * 8 + 3 * 4))
    for rep in range(args.reps):
        t0 = time.perf_counter()
        api.unitig_links(graph, dev)
        wall = time.perf_counter() - t0
        t = api.last_unitig_graph_times()
        emit("links", {"rep": rep, "links": t["links"], "upload_ms": t["upload_ms"], "link_ms": t["link_ms"], "download_ms": t["download_ms"],
                       "peak_arena_bytes": t["peak_arena_bytes"], "wall_ms": 1e3 * wall})
    B, A, seconds = host_grouping(graph, kmers, L)
    assert (B, A) == (len(found), len(found.arm_unitig)), "the host grouping disagrees with the device"
    emit("host", {"method": "numpy.unique over the canonical keys", "bubbles": B, "arms": A, "ms": 1e3 * seconds})

    def best(kind, field):
        rows = doc[kind][1:] or doc[kind]
        return min(r[field] for r in rows)

    group_ms, allele_ms, link_ms = best("bubbles", "group_ms"), best("bubbles", "allele_ms"), best("links", "link_ms")
    doc["summary"] = {
        "group_ms": group_ms, "allele_ms": allele_ms, "carrier_ms": best("bubbles_with_masks", "carrier_ms"),
        "upload_ms": best("bubbles", "upload_ms"), "download_ms": best("bubbles", "download_ms"),
        "upload_with_masks_ms": best("bubbles_with_masks", "upload_ms"),
        "allele_min_bytes": doc["allele_min_bytes"], "allele_gb_per_s_at_the_least": round(doc["allele_min_bytes"] / (allele_ms * 1e6), 3) if allele_ms else None,
        "link_stage_ms": link_ms, "group_over_link_stage": round(group_ms / link_ms, 3),
        "host_ms": round(1e3 * seconds, 1), "host_over_group": round(1e3 * seconds / group_ms, 1),
        "peak_arena_bytes": max(r["peak_arena_bytes"] for r in doc["bubbles"]),
        "peak_arena_bytes_with_masks": max(r["peak_arena_bytes"] for r in doc["bubbles_with_masks"]),
        "bubbles": len(found), "arms": len(found.arm_unitig),
    }
    print(json.dumps({"summary": doc["summary"]}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
