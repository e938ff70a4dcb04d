"""compact_timing.py -- what the unitig compaction (`--seq-in`, mtg_compact_unitigs) costs, phase by phase, on the four
haplotypes of G-seq (the splitmix64 streams of synth.random_genome, as arrays): upload, pack, insert, ids, nodes (with succ), rank
(pointer jumping), emit (HIP events around the kernel phases), download and the whole call; the pointer-jumping rounds; the bytes the
kernels must move at the least and the fraction of the 8 TB/s HBM peak they imply; the peak of live device-arena bytes. The baseline
is the only at-size compaction the tree had before: the compaction part of synth.g_seq_arrays_torch (its wall clock minus the
generation of the haplotypes, which is timed on its own with the same torch operations; what remains also lists the links between
the unitigs and downloads the arrays, which g_seq_arrays_torch does not separate), in the same process, after the device runs.

usage: python tools/compact_timing.py [--length 100000000] [--k 31] [--reps 3] [--device 0] [--out profiles/compact_gseq_1e8.json]
One JSON line per repetition (the first one also pays the arena's first chunks and is left out of the summary); --out writes all of
it as one JSON document."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def haplotype_arrays(length: int, seed: int, haplotypes: int = 4, sub_rate: float = 0.02):
    """synth.random_genome as one uint8 array plus offsets."""
    from matchtigs_amd import synth

    abc = np.frombuffer(b"ACGT", np.uint8)
    g = (synth.splitmix64(seed, length, 10) % np.uint64(4)).astype(np.int64)
    data = np.empty(haplotypes * length, np.uint8)
    data[:length] = abc[g]
    for h in range(1, haplotypes):
        mut = synth._uniform01(synth.splitmix64(seed, length, 20 + h)) < sub_rate
        shift = (synth.splitmix64(seed, length, 40 + h) % np.uint64(3)).astype(np.int64) + 1
        data[h * length:(h + 1) * length] = abc[np.where(mut, (g + shift) % 4, g)]
    return data, np.arange(haplotypes + 1, dtype=np.uint64) * np.uint64(length)


def main() -> None:
    from matchtigs_amd import api, synth

    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=100_000_000)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out")
    ap.add_argument("--no-baseline", action="store_true", help="skip the torch compaction (profiler runs, k > 31 or even k)")
    args = ap.parse_args()
    k = args.k

    data, off = haplotype_arrays(args.length, 1)
    doc = {"tool": "compact_timing", "length": args.length, "haplotypes": 4, "k": k, "reps": []}
    phases = ("pack_ms", "insert_ms", "ids_ms", "nodes_ms", "rank_ms", "emit_ms")
    for rep in range(args.reps):
        t0 = time.perf_counter()
        store, c = api.compact_unitigs((data, off), k, args.device)
        wall = time.perf_counter() - t0
        t = api.last_compact_times()
        kernels_ms = sum(t[p] for p in phases)
        out = {"rep": rep, **{f: (round(v, 3) if isinstance(v, float) else v) for f, v in t.items()}, "wall_ms": round(1e3 * wall, 3),
               "kernel_phases_ms": round(kernels_ms, 3), "slowest_phase": max(phases, key=lambda p: t[p]),
               "min_bytes_gb_per_s": round(t["bytes"] / (kernels_ms * 1e6), 1),
               "min_bytes_frac_of_8tbps": round(t["bytes"] / (kernels_ms * 1e-3) / 8e12, 4),
               "unitigs": c.unitigs, "unitig_characters": c.unitig_characters, "distinct_kmers": c.distinct_kmers,
               "closed_walks": c.closed_walks, "longest_unitig_kmers": c.longest_unitig_kmers}
        doc["reps"].append(out)
        print(json.dumps(out), flush=True)
        del store
    api.release_device_memory(args.device)
    kept = doc["reps"][1:] or doc["reps"]
    doc["compact_total_ms"] = min(r["total_ms"] for r in kept)
    doc["compact_kernel_phases_ms"] = min(r["kernel_phases_ms"] for r in kept)
    if not args.no_baseline and k <= 31 and k % 2 == 1:
        import torch

        dev = f"cuda:{args.device}"

        def generation_ms():  # the part of g_seq_arrays_torch that is not compaction: the haplotypes' bases (same operations)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            z = torch.arange(1, args.length + 1, dtype=torch.int64, device=dev)
            for _ in range(1 + 2 * 3):  # splitmix streams: the genome, and two per further haplotype
                y = z * 0x1E3779B97F4A7C15 + 1
                y = (y ^ (y >> 30)) * 0x3F58476D1CE4E5B9
                y = (y ^ (y >> 27)) * 0x14D049BB133111EB
                y = y ^ (y >> 31)
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0)

        def baseline():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ua = synth.g_seq_arrays_torch(args.length, seed=1, k=k, device=dev)
            torch.cuda.synchronize()
            ms = 1e3 * (time.perf_counter() - t0)
            return ms, ua.n_unitigs, int(ua.off[-1])

        baseline()  # warm-up
        gen = min(generation_ms() for _ in range(3))  # (the smallest of three: the caching allocator's refills are not generation)
        doc["baseline_torch"] = []
        for rep in range(2):
            ms, n_u, n_c = baseline()
            doc["baseline_torch"].append({"rep": rep, "g_seq_arrays_torch_ms": round(ms, 3), "generation_ms": round(gen, 3),
                                          "compaction_ms": round(ms - gen, 3), "unitigs": n_u, "unitig_characters": n_c})
            print(json.dumps({"baseline_torch": doc["baseline_torch"][-1]}), flush=True)
            torch.cuda.empty_cache()
        doc["baseline_compaction_ms"] = min(r["compaction_ms"] for r in doc["baseline_torch"])
        doc["same_counts_as_baseline"] = all((r["unitigs"], r["unitig_characters"]) == (kept[0]["unitigs"], kept[0]["unitig_characters"])
                                             for r in doc["baseline_torch"])
        doc["faster_than_baseline"] = max(r["total_ms"] for r in kept) < doc["baseline_compaction_ms"]
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
