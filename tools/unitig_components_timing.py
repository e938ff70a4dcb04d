"""unitig_components_timing.py -- what the connected components of the unitig graph (`--components-out`, `--min-component-kmers`;
mtg_unitig_components) cost, phase by phase, on the unitigs of G-seq (the four haplotypes of tools/compact_timing.py,
compacted by the library): the uploads, the label kernels and the statistics kernel (HIP events), the download and the peak of live
device-arena bytes; the statistics kernel with and without the per-wave aggregation of its atomics. The yardsticks run in the same
process on the same graph: the link stage (`api.unitig_links`: it reads the same edge arrays and builds the lists the component
stage does without), and a union on the host over the downloaded link lists -- scipy.sparse.csgraph.connected_components where
scipy is importable, else a numpy label propagation (min-label sweeps over the link pairs until nothing changes), named in the
output.

usage: python tools/unitig_components_timing.py [--length 100000000] [--k 31] [--reps 3] [--device 0] [--out profiles/unitig_components_gseq_1e8.json]
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


def host_components(link_off, link_to, U):
    """-> (method, labels numbered by smallest unitig, seconds) from the link lists, on the host."""
    t0 = time.perf_counter()
    src = (np.repeat(np.arange(2 * U, dtype=np.int64), np.diff(link_off).astype(np.int64)) >> 1)
    dst = (link_to >> 1).astype(np.int64)
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components

        method = "scipy.sparse.csgraph.connected_components"
        _, lab = connected_components(coo_matrix((np.ones(len(src), np.uint8), (src, dst)), shape=(U, U)), directed=False)
        root = np.full(lab.max() + 1 if U else 0, U, np.int64)
        np.minimum.at(root, lab, np.arange(U))
        label = root[lab]
    except ImportError:
        method = "numpy label propagation"
        label = np.arange(U, dtype=np.int64)
        while True:
            low = np.minimum(label[src], label[dst])
            new = label.copy()
            np.minimum.at(new, src, low)
            np.minimum.at(new, dst, low)
            new = new[new]  # one pointer jump
            if np.array_equal(new, label):
                break
            label = new
    # numbered by the smallest unitig, ascending: a unitig that is its own label starts a component
    number = np.cumsum(label == np.arange(U)) - 1
    return method, number[label], time.perf_counter() - t0


def main() -> None:
    from compact_timing import haplotype_arrays
    from matchtigs_amd import _lib, api

    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=100_000_000)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out")
    args = ap.parse_args()
    k, dev = args.k, args.device

    store, c = api.compact_unitigs(haplotype_arrays(args.length, 1), k, dev)
    U = len(store)
    graph = api.Bigraph.from_sequences(store.arrays(), k, dev)
    kmers = (np.diff(store.arrays()[1]) - np.uint64(k - 1)).astype(np.uint64)
    doc = {"tool": "unitig_components_timing", "length": args.length, "haplotypes": 4, "k": k, "unitigs": U, "nodes": graph.node_count(),
           "edges": graph.edge_count(), "components": [], "components_plain_atomics": [], "links": [], "host": []}

    def emit(kind, row):
        row = {f: (round(v, 3) if isinstance(v, float) else v) for f, v in row.items()}
        doc[kind].append(row)
        print(json.dumps({kind: row}), flush=True)

    L = _lib.load()
    comps = None
    for kind, on in (("components", 1), ("components_plain_atomics", 0)):
        L.mtg_set_unitig_components_aggregation(on)
        try:
            for rep in range(args.reps):
                t0 = time.perf_counter()
                got = api.unitig_components(graph, kmers, device_id=dev)
                wall = time.perf_counter() - t0
                emit(kind, {"rep": rep, **api.last_unitig_components_times(), "wall_ms": 1e3 * wall})
                assert comps is None or all(np.array_equal(getattr(got, f), getattr(comps, f)) for f in ("component_of", "kmers", "links", "irregular"))
                comps = got
        finally:
            L.mtg_set_unitig_components_aggregation(1)
    doc["describe"] = comps.describe()
    link_off = link_to = None
    for rep in range(args.reps):
        t0 = time.perf_counter()
        link_off, link_to = api.unitig_links(graph, dev)
        wall = time.perf_counter() - t0
        t = api.last_unitig_graph_times()
        emit("links", {"rep": rep, "links": t["links"], "upload_ms": t["upload_ms"], "link_ms": t["link_ms"], "download_ms": t["download_ms"],
                       "peak_arena_bytes": t["peak_arena_bytes"], "wall_ms": 1e3 * wall})
    method, label, seconds = host_components(link_off, link_to, U)
    assert np.array_equal(label.astype(np.uint32), comps.component_of), "the host union disagrees with the device"
    assert int(comps.links.sum()) == len(link_to)
    emit("host", {"method": method, "ms": 1e3 * seconds})

    def best(kind, field):
        rows = doc[kind][1:] or doc[kind]
        return min(r[field] for r in rows)

    label_ms, stats_ms, plain_ms, link_ms = best("components", "label_ms"), best("components", "stats_ms"), best("components_plain_atomics", "stats_ms"), best("links", "link_ms")
    doc["summary"] = {
        "label_ms": label_ms, "label_rep_ms": best("components", "rep_ms"), "label_union_ms": best("components", "union_ms"),
        "label_flatten_ms": best("components", "flatten_ms"), "stats_ms": stats_ms, "stats_plain_atomics_ms": plain_ms,
        "stats_plain_over_aggregated": round(plain_ms / stats_ms, 3),
        "upload_ms": best("components", "upload_ms"), "download_ms": best("components", "download_ms"),
        "link_stage_ms": link_ms, "component_kernels_over_link_stage": round((label_ms + stats_ms) / link_ms, 3),
        "host_method": method, "host_ms": round(1e3 * seconds, 1), "host_over_component_kernels": round(1e3 * seconds / (label_ms + stats_ms), 1),
        "peak_arena_bytes": max(r["peak_arena_bytes"] for r in doc["components"]), "components": len(comps),
    }
    print(json.dumps({"summary": doc["summary"]}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
