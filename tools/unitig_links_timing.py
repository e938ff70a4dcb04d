"""unitig_links_timing.py -- what the unitig graph output (`--unitigs-bcalm-out`, `--unitigs-gfa-out`; mtg_unitig_links,
mtg_write_unitig_graph_text) costs, phase by phase, on the unitigs of G-seq (the four haplotypes of
tools/compact_timing.py, compacted by the library): the uploads, the link kernels, the scans of the text and the text kernel (HIP
events), the download, the links, the bytes written and the peak of live device-arena bytes. The yardsticks run in the same process
on the same store: the unitig FASTA spelling (`--unitigs-fa-out`: one walk per unitig through mtg_write_walks_text_device; its
kernel's ms and output bytes) against the text kernel, and the (k-1)-mer join that built the graph (`--fa-in`; its
kernels' ms) against the link stage.

usage: python tools/unitig_links_timing.py [--length 100000000] [--k 31] [--reps 3] [--device 0] [--out profiles/unitig_links_gseq_1e8.json]
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


def main() -> None:
    from compact_timing import haplotype_arrays
    from matchtigs_amd import api

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
    doc = {"tool": "unitig_links_timing", "length": args.length, "haplotypes": 4, "k": k, "unitigs": U, "unitig_characters": c.unitig_characters,
           "join": [], "links": [], "bcalm": [], "gfa": [], "spell": []}

    def emit(kind, row):
        row = {f: (round(v, 3) if isinstance(v, float) else v) for f, v in row.items()}
        doc[kind].append(row)
        print(json.dumps({kind: row}), flush=True)

    graph = None
    for rep in range(args.reps):  # the join of DESIGN.md 14 on this store: the graph the links are read from
        graph = api.Bigraph.from_sequences(store.arrays(), k, dev)
        t = api.last_fasta_in_times()
        emit("join", {"rep": rep, "kernel_ms": t["kernel_ms"], "upload_ms": t["upload_ms"], "download_ms": t["download_ms"], "build_ms": t["build_ms"]})
    doc["nodes"], doc["edges"] = graph.node_count(), graph.edge_count()
    for rep in range(args.reps):
        t0 = time.perf_counter()
        link_off, link_to = api.unitig_links(graph, dev)
        wall = time.perf_counter() - t0
        t = api.last_unitig_graph_times()
        emit("links", {"rep": rep, "links": t["links"], "upload_ms": t["upload_ms"], "link_ms": t["link_ms"], "download_ms": t["download_ms"],
                       "peak_arena_bytes": t["peak_arena_bytes"], "wall_ms": 1e3 * wall,
                       "longest_list": int(np.diff(link_off).max()) if U else 0})
        del link_off, link_to
    kc = np.diff(store.arrays()[1]) - np.uint64(k - 1)  # (handed in, so that the abundance path runs: one per k-mer)
    for kind, gfa in (("bcalm", False), ("gfa", True)):
        for rep in range(args.reps):
            t0 = time.perf_counter()
            text = api.write_unitig_graph(graph, store, k, gfa=gfa, kc=kc, device_id=dev)
            wall = time.perf_counter() - t0
            t = api.last_unitig_graph_times()
            assert t["bytes"] == len(text)
            emit(kind, {"rep": rep, **t, "wall_ms": 1e3 * wall, "text_bytes_per_ms": t["bytes"] / t["text_ms"],
                        "text_min_bytes_gb_per_s": t["text_min_bytes"] / (t["text_ms"] * 1e6)})
            del text
    limits, edges = np.arange(1, U + 1, dtype=np.uint64), 2 * np.arange(U, dtype=np.uint32)  # one walk per unitig, forwards
    for rep in range(args.reps):
        text = api.write_walks_text_device(graph, (limits, edges), store.arrays(), k, device_id=dev)
        s = api.last_spell_kernel()
        emit("spell", {"rep": rep, "kernel_ms": s["ms"], "hbm_bytes": s["bytes"], "output_bytes": len(text),
                       "output_bytes_per_ms": len(text) / s["ms"]})
        del text

    def best(kind, field, low=True):
        rows = doc[kind][1:] or doc[kind]
        return (min if low else max)(r[field] for r in rows)

    spell_rate = best("spell", "output_bytes_per_ms", low=False)
    doc["summary"] = {
        "link_stage_ms": best("links", "link_ms"), "join_kernels_ms": best("join", "kernel_ms"),
        "link_stage_over_join": round(best("links", "link_ms") / best("join", "kernel_ms"), 3),
        "spell_output_bytes_per_ms": spell_rate,
        "bcalm_text_bytes_per_ms": best("bcalm", "text_bytes_per_ms", low=False),
        "gfa_text_bytes_per_ms": best("gfa", "text_bytes_per_ms", low=False),
        "bcalm_rate_over_spell": round(best("bcalm", "text_bytes_per_ms", low=False) / spell_rate, 3),
        "gfa_rate_over_spell": round(best("gfa", "text_bytes_per_ms", low=False) / spell_rate, 3),
        "peak_arena_bytes": max(r["peak_arena_bytes"] for kind in ("links", "bcalm", "gfa") for r in doc[kind]),
    }
    print(json.dumps({"summary": doc["summary"]}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
