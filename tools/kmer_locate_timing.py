"""kmer_locate_timing.py -- what locating k-mers (`--query-locate-out`, mtg_kmer_index_locate) costs beside the
membership query, on the inputs of kmer_query_timing.py: G-seq; the index is built from the greedy matchtigs in
device order; the query is the unitigs plus an equal volume of the same unitigs with 3 % substitutions and an `N` every ~10^3 bases.

In one process and per k (31 and one k >= 32 by default; the tigs and the unitigs are those of k = 31 either way, the index and
the query windows are of the k asked for) a plain and a locating index are built, and `query` (without bit arrays) and `locate` run
on the same query. Per repetition: build ms and device bytes of both index kinds, probe ms and ns per window of `query` and of
`locate`, the runs phase, the bytes `locate` downloads (5 x 8 + 1 per run, 2 x 8 per record, 8 for the count) beside the 8 B per
query base a per-window answer would take, and the number of runs. The membership probe (query_probe_ms) is the parent's kernel and
the yardstick; the JSON gives locate's probe and probe + runs as multiples of it (the first repetition, which pays the arena's first
chunks, left out where there are more).

usage: python tools/kmer_locate_timing.py [--length 100000000] [--k 31 41] [--reps 3] [--device 0] [--out profiles/kmer_locate_gseq_1e8.json]
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
    ap.add_argument("--k", type=int, nargs="+", default=[31, 41])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out")
    args = ap.parse_args()
    k_graph = 31

    t0 = time.perf_counter()
    ua = synth.g_seq_arrays_torch(args.length, seed=1, k=k_graph, device=f"cuda:{args.device}")
    torch.cuda.empty_cache()
    G = api.Bigraph.from_unitig_links_arrays(ua.weights, ua.links)
    lim, ed = api.GreedytigAlgorithm.compute_tigs_np(G, api.GreedytigAlgorithmConfiguration(1, k_graph, euler_mode=api.EulerMode.Device,
                                                                                            device_ids=(args.device,)))
    tig_seq, tig_off = fasta_sequence_arrays(api.write_walks_text_device(G, (lim, ed), (ua.seq, ua.off), k_graph, device_id=args.device))
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
    prep_s = time.perf_counter() - t0

    doc = {"tool": "kmer_locate_timing", "length": args.length, "k_of_the_tigs": k_graph, "tigs": len(tig_off) - 1,
           "index_characters": int(tig_off[-1]), "query_records": len(q_off) - 1, "query_characters": int(q_off[-1]),
           "preparation_s": round(prep_s, 1), "per_k": []}
    for k in args.k:
        reps = []
        for rep in range(args.reps):
            out = {"k": k, "rep": rep}
            for kind, locating in (("plain", False), ("locating", True)):
                t0 = time.perf_counter()
                ix = api.KmerIndex((tig_seq, tig_off), k, args.device, locate=locating)
                out[f"{kind}_build_wall_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
                tb = api.last_kmer_query_times()
                out[f"{kind}_build_ms"] = round(tb["build_upload_ms"] + tb["build_pack_ms"] + tb["build_insert_ms"], 3)
                out[f"{kind}_build_insert_ms"] = round(tb["build_insert_ms"], 3)
                out[f"{kind}_device_bytes"] = ix.info.device_bytes
                t0 = time.perf_counter()
                r = ix.query((q_seq, q_off))
                out[f"{kind}_query_wall_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
                out[f"{kind}_query_probe_ms"] = round(api.last_kmer_query_times()["query_probe_ms"], 3)
                windows, found = int(r.kmers.sum()), int(r.found.sum())
                if locating:
                    t0 = time.perf_counter()
                    loc = ix.locate((q_seq, q_off))
                    out["locate_wall_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
                    tl = api.last_kmer_locate_times()
                    out.update({f"locate_{f}": round(v, 3) for f, v in tl.items()})
                    out["runs"] = len(loc.runs)
                    out["counts_equal_query"] = bool(np.array_equal(loc.found, r.found) and np.array_equal(loc.valid, r.valid))
                    out["runs_cover_found"] = int(loc.runs["kmers"].sum()) == found
                    out["locate_downloaded_bytes"] = 41 * len(loc.runs) + 16 * len(loc.kmers) + 8
                    out["per_window_answer_bytes"] = 8 * int(q_off[-1])
                    del loc
                ix.close()
                del r
            out.update({"windows": windows, "found": found,
                        "query_probe_ns_per_window": round(1e6 * out["plain_query_probe_ms"] / windows, 4),
                        "locate_probe_ns_per_window": round(1e6 * out["locate_probe_ms"] / windows, 4),
                        "locate_runs_ns_per_window": round(1e6 * out["locate_runs_ms"] / windows, 4),
                        "locate_probe_over_query_probe": round(out["locate_probe_ms"] / out["plain_query_probe_ms"], 3),
                        "locate_probe_and_runs_over_query_probe": round((out["locate_probe_ms"] + out["locate_runs_ms"]) / out["plain_query_probe_ms"], 3)})
            reps.append(out)
            print(json.dumps(out), flush=True)
        api.release_device_memory(args.device)
        steady = reps[1:] or reps
        doc["per_k"].append({"k": k, "reps": reps,
                             "locate_probe_over_query_probe_min_max": [min(r["locate_probe_over_query_probe"] for r in steady),
                                                                       max(r["locate_probe_over_query_probe"] for r in steady)],
                             "locate_probe_and_runs_over_query_probe_min_max": [min(r["locate_probe_and_runs_over_query_probe"] for r in steady),
                                                                                max(r["locate_probe_and_runs_over_query_probe"] for r in steady)]})
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
