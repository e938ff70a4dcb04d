"""tig_index_timing.py -- the sparse minimizer index (api.TigIndex, mtg_tig_index_*) beside the table index
(api.KmerIndex) on the workload of tools/kmer_query_timing.py: G-seq, the query = the unitigs plus an equal volume of the
same unitigs with 3 % substitutions and an `N` every ~10^3 bases. In one process, for each index kind (table, minimizer with m = 19 at
k = 31) over each indexed set (the unitigs, the greedy tigs in device order): device_bytes, bytes per distinct k-mer, the build phases
and the windows per second of the probe kernel (HIP events around the kernels), `--reps` repetitions each; `best` takes the fastest
repetition after the first, which also pays the arena's first chunks. The two kinds must give the same counts, which the tool checks.
No speed is promised either way: the ratios minimizer / table are what the JSON is for.

usage: python tools/tig_index_timing.py [--length 100000000] [--k 31] [--m 19] [--reps 3] [--device 0] [--out profiles/tig_index_gseq_1e8.json]
One JSON line per repetition; --out writes all of it as one JSON document."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from kmer_compare_timing import fasta_sequence_arrays  # noqa: E402


def main() -> None:
    import torch

    from matchtigs_amd import api, synth

    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=100_000_000)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--m", type=int, default=None, help="minimizer length (default: the library's, 19 at k = 31)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out")
    args = ap.parse_args()
    k = args.k

    t0 = time.perf_counter()
    ua = synth.g_seq_arrays_torch(args.length, seed=1, k=k, device=f"cuda:{args.device}")
    torch.cuda.empty_cache()
    G = api.Bigraph.from_unitig_links_arrays(ua.weights, ua.links)
    lim, ed = api.GreedytigAlgorithm.compute_tigs_np(G, api.GreedytigAlgorithmConfiguration(1, k, euler_mode=api.EulerMode.Device,
                                                                                            device_ids=(args.device,)))
    tig_seq, tig_off = fasta_sequence_arrays(api.write_walks_text_device(G, (lim, ed), (ua.seq, ua.off), k, device_id=args.device))
    del G, lim, ed
    api.release_device_memory(args.device)
    rng = np.random.default_rng(1)
    n = len(ua.seq)
    noisy = ua.seq.copy()
    sub = rng.random(n) < 0.03
    noisy[sub] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(sub.sum()))]
    noisy[rng.random(n) < 1e-3] = ord("N")
    q_seq = np.concatenate([ua.seq, noisy])
    q_off = np.concatenate([ua.off, ua.off[1:] + ua.off[-1]]).astype(np.uint64)
    del noisy, sub
    distinct = len(ua.kmers)
    doc = {"tool": "tig_index_timing", "length": args.length, "k": k, "distinct_kmers": distinct, "query_records": len(q_off) - 1,
           "query_characters": int(q_off[-1]), "preparation_s": round(time.perf_counter() - t0, 1), "runs": {}}

    sets = {"unitigs": (ua.seq, ua.off.astype(np.uint64)), "greedytigs": (tig_seq, tig_off)}
    counts = {}
    for over, indexed in sets.items():
        for kind in ("table", "minimizer"):
            reps = []
            for rep in range(args.reps):
                t0 = time.perf_counter()
                ix = api.KmerIndex(indexed, k, args.device) if kind == "table" else api.TigIndex(indexed, k, args.m, args.device)
                build_wall = time.perf_counter() - t0
                t0 = time.perf_counter()
                r = ix.query((q_seq, q_off), bits=True)
                query_wall = time.perf_counter() - t0
                t = api.last_kmer_query_times() if kind == "table" else api.last_tig_index_times()
                info = ix.info
                ix.close()
                windows = int(r.kmers.sum())
                counts[over, kind] = (windows, int(r.valid.sum()), int(r.found.sum()))
                out = {"over": over, "index": kind, "rep": rep, **{f: round(v, 3) for f, v in t.items()}, "build_wall_ms": round(1e3 * build_wall, 3),
                       "query_wall_ms": round(1e3 * query_wall, 3), "windows": windows, "valid": counts[over, kind][1], "found": counts[over, kind][2],
                       "probe_windows_per_s": round(windows / (t["query_probe_ms"] * 1e-3))}
                reps.append(out)
                print(json.dumps(out), flush=True)
                del r
            later = reps[1:] or reps
            fields = {f.name: getattr(info, f.name) for f in info.__dataclass_fields__.values()}
            doc["runs"][f"{kind}/{over}"] = {
                "info": fields, "device_bytes": info.device_bytes, "bytes_per_distinct_kmer": round(info.device_bytes / distinct, 4),
                "bytes_per_window": round(info.device_bytes / info.occurrences, 4),
                "best": {"probe_windows_per_s": max(x["probe_windows_per_s"] for x in later),
                         "build_kernels_ms": round(min(sum(v for f, v in x.items() if f.startswith("build_") and f.endswith("_ms")
                                                           and f not in ("build_upload_ms", "build_wall_ms")) for x in later), 3)},
                "reps": reps}
            api.release_device_memory(args.device)
    if len(set(counts.values())) != 1:
        raise SystemExit(f"the indexes disagree: {counts}")
    doc["minimizer_over_table"] = {}
    for over in sets:
        a, b = doc["runs"][f"minimizer/{over}"], doc["runs"][f"table/{over}"]
        doc["minimizer_over_table"][over] = {"device_bytes": round(a["device_bytes"] / b["device_bytes"], 4),
                                             "probe_windows_per_s": round(a["best"]["probe_windows_per_s"] / b["best"]["probe_windows_per_s"], 4),
                                             "build_kernels_ms": round(a["best"]["build_kernels_ms"] / b["best"]["build_kernels_ms"], 4)}
    a, b = doc["runs"]["minimizer/greedytigs"], doc["runs"]["minimizer/unitigs"]
    doc["minimizer_greedytigs_over_unitigs_device_bytes"] = round(a["device_bytes"] / b["device_bytes"], 4)
    print(json.dumps({"minimizer_over_table": doc["minimizer_over_table"]}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
