"""fasta_in_timing.py -- what the plain unitig FASTA route (`--fa-in`, mtg_read_fasta) costs, phase by phase, on G-seq: the parse of
the file, the upload of the sequences, the join kernels (HIP events: pack, extract, insert, lookup, scan, edges), the download of the
edge arrays and the host graph build (mtg_graph_from_edges' checks). The join's kernel time is set against the bytes those kernels
must move at the least (fasta_in_device.hip) and the 8 TB/s HBM peak.

usage: python tools/fasta_in_timing.py [--length 100000000] [--k 31] [--reps 3] [--device 0]
One JSON line per repetition (the first one also pays the HIP runtime's start and the arena's first chunk)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main() -> None:
    from matchtigs_amd import api, synth

    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=100_000_000)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    t0 = time.perf_counter()
    ua = synth.g_seq_arrays_torch(args.length, seed=1, k=args.k, device=f"cuda:{args.device}")
    gen_s = time.perf_counter() - t0
    s, o = ua.seq.tobytes(), ua.off.astype(np.int64)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "unitigs.fa")
        with open(path, "wb") as f:
            f.write(b"".join(b">%d\n%s\n" % (u, s[o[u]:o[u + 1]]) for u in range(ua.n_unitigs)))
        file_bytes = os.path.getsize(path)
        for rep in range(args.reps):
            t0 = time.perf_counter()
            G, store = api.read_fasta(path, args.k, args.device)
            wall = time.perf_counter() - t0
            t = api.last_fasta_in_times()
            out = {"tool": "fasta_in_timing", "rep": rep, "length": args.length, "k": args.k, "unitigs": ua.n_unitigs,
                   "file_bytes": file_bytes, "nodes": G.node_count(), "edges": G.edge_count(),
                   "parse_ms": round(t["parse_ms"], 3), "upload_ms": round(t["upload_ms"], 3), "join_kernels_ms": round(t["kernel_ms"], 3),
                   "download_ms": round(t["download_ms"], 3), "graph_build_ms": round(t["build_ms"], 3), "wall_ms": round(1e3 * wall, 3),
                   "join_min_bytes": int(t["bytes"]),
                   "join_gb_per_s": round(t["bytes"] / (t["kernel_ms"] * 1e6), 1) if t["kernel_ms"] else None,
                   "join_frac_of_8tbps": round(t["bytes"] / (t["kernel_ms"] * 1e-3) / 8e12, 4) if t["kernel_ms"] else None,
                   "generator_s": round(gen_s, 1)}
            print(json.dumps(out), flush=True)
            del G, store


if __name__ == "__main__":
    main()
