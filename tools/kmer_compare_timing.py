"""kmer_compare_timing.py -- what the k-mer set comparison (`--verify`, mtg_compare_kmer_sets) costs, phase by phase, on G-seq: the
unitigs (as arrays) against their greedy matchtigs in device order (as spelled by write_walks_text_device). Per repetition the
upload, the pack, the two insert passes, the count (HIP events around the kernels) and the whole call; the table operations (one per
window of A and of B, one per slot read by the count) per second of the insert + count kernels, to set against the random-access
ceiling of 44-54 G lines/s. The baseline is the check the suite had before: synth.kmer_codes_of_sequences_torch, once
for the unitigs and once for the tigs on the same arrays, wall clock around the two calls with a synchronize after each, after one
warm-up call.

usage: python tools/kmer_compare_timing.py [--length 100000000] [--k 31] [--reps 3] [--device 0] [--out profiles/kmer_compare_gseq_1e8.json]
One JSON line per repetition (the first one also pays the arena's first chunks); --out writes all of it as one JSON document."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def fasta_sequence_arrays(fa: bytes):
    """(uint8 bases, uint64 offsets) of a FASTA with one header and one sequence line per record."""
    a = np.frombuffer(fa, np.uint8)
    nl = np.nonzero(a == 10)[0]
    starts, ends = nl[0::2] + 1, nl[1::2]
    off = np.zeros(len(starts) + 1, np.uint64)
    off[1:] = np.cumsum(ends - starts)
    d = np.zeros(len(a) + 1, np.int32)
    d[starts] += 1
    d[ends] -= 1
    return a[np.cumsum(d[:-1], dtype=np.int32) > 0], off


def main() -> None:
    import torch

    from matchtigs_amd import api, synth

    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=100_000_000)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out")
    ap.add_argument("--no-baseline", action="store_true", help="skip the torch sort baseline (profiler runs)")
    args = ap.parse_args()
    k = args.k

    t0 = time.perf_counter()
    ua = synth.g_seq_arrays_torch(args.length, seed=1, k=k, device=f"cuda:{args.device}")
    torch.cuda.empty_cache()
    G = api.Bigraph.from_unitig_links_arrays(ua.weights, ua.links)
    lim, ed = api.GreedytigAlgorithm.compute_tigs_np(G, api.GreedytigAlgorithmConfiguration(1, k, euler_mode=api.EulerMode.Device,
                                                                                            device_ids=(args.device,)))
    seq, off = fasta_sequence_arrays(api.write_walks_text_device(G, (lim, ed), (ua.seq, ua.off), k, device_id=args.device))
    del G, lim, ed
    api.release_device_memory(args.device)
    prep_s = time.perf_counter() - t0

    doc = {"tool": "kmer_compare_timing", "length": args.length, "k": k, "unitigs": ua.n_unitigs, "tigs": len(off) - 1,
           "characters_a": int(ua.off[-1]), "characters_b": int(off[-1]), "preparation_s": round(prep_s, 1), "reps": []}
    for rep in range(args.reps):
        t0 = time.perf_counter()
        c = api.compare_kmer_sets((ua.seq, ua.off), (seq, off), k, args.device)
        wall = time.perf_counter() - t0
        t = api.last_kmer_compare_times()
        slots = max(8, (2 * (c.occurrences_a + c.occurrences_b) + 7) // 8 * 8)
        ops = c.occurrences_a + c.occurrences_b + slots
        kernels_ms = t["insert_a_ms"] + t["insert_b_ms"] + t["count_ms"]
        out = {"rep": rep, **{f: round(v, 3) for f, v in t.items()}, "wall_ms": round(1e3 * wall, 3), "equal": c.equal,
               "distinct": c.distinct_a, "occurrences_a": c.occurrences_a, "occurrences_b": c.occurrences_b, "repeated_b": c.repeated_b,
               "table_slots": slots, "table_bytes": 8 * slots, "table_operations": ops,
               "insert_count_kernels_ms": round(kernels_ms, 3), "table_operations_per_s": round(ops / (kernels_ms * 1e-3)),
               "window_operations_per_s_insert_only": round((c.occurrences_a + c.occurrences_b) / ((t["insert_a_ms"] + t["insert_b_ms"]) * 1e-3))}
        doc["reps"].append(out)
        print(json.dumps(out), flush=True)
    api.release_device_memory(args.device)
    if not args.no_baseline:
        def baseline():
            t0 = time.perf_counter()
            ca, _ = synth.kmer_codes_of_sequences_torch(ua.seq, ua.off, k)
            torch.cuda.synchronize()
            cb, n_occ = synth.kmer_codes_of_sequences_torch(seq, off, k)
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0), bool(np.array_equal(ca, cb)), int(n_occ)

        baseline()  # warm-up
        doc["baseline_torch_sort"] = []
        for rep in range(2):
            ms, same, n_occ = baseline()
            doc["baseline_torch_sort"].append({"rep": rep, "total_ms": round(ms, 3), "equal": same, "occurrences_b": n_occ})
            print(json.dumps({"baseline_torch_sort": doc["baseline_torch_sort"][-1]}), flush=True)
        doc["compare_total_ms"] = min(r["total_ms"] for r in doc["reps"][1:] or doc["reps"])
        doc["baseline_total_ms"] = min(r["total_ms"] for r in doc["baseline_torch_sort"])
        doc["not_slower_than_baseline"] = max(r["total_ms"] for r in doc["reps"][1:] or doc["reps"]) <= doc["baseline_total_ms"]
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
