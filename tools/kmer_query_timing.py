"""kmer_query_timing.py -- what the k-mer index (`--query-fa`, mtg_kmer_index_*) costs, phase by phase, on G-seq: the
index is built from the greedy matchtigs in device order (as spelled by write_walks_text_device); the query is the unitigs plus an
equal volume of the same unitigs with 3 % substitutions and an `N` every ~10^3 bases. Per repetition the build phases (upload, pack,
insert) and the query phases (upload, pack, probe; HIP events around the kernels) and the windows per second of the probe kernel.

For context, in the same process: (a) api.compare_kmer_sets on the two sets the index and the clean half of the query are -- the
tigs as A, the unitigs as B (the comparison aborts on `N`, so the noisy half stays out). Its insert_b_ms per window of B is the
nearest kernel the library had before: B's windows looked up in, and marked in, a table that holds A's.
(b) a torch baseline on the same arrays: synth.kmer_codes_of_sequences_torch of the tigs and of the unitigs plus torch.searchsorted
of the unitigs' codes in the tigs' (the clean half only: the baseline has no notion of `N`), wall clock with a synchronize. It is
context, not like for like: it looks up the distinct codes of the query, not every window, answers nothing per record, and its time
includes a device -> host -> device trip of the codes. The JSON says so, and gives the probe-against-insert verdict in both readings
(best probe against worst insert repetition, and best against best).

usage: python tools/kmer_query_timing.py [--length 100000000] [--k 31] [--reps 3] [--device 0] [--out profiles/kmer_query_gseq_1e8.json]
One JSON line per repetition (the first one also pays the arena's first chunks); --out writes all of it as one JSON document."""
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out")
    ap.add_argument("--no-baseline", action="store_true", help="skip the torch baseline (profiler runs)")
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
    # the query: the unitigs, then the unitigs again with 3 % substitutions and a sprinkling of N
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

    doc = {"tool": "kmer_query_timing", "length": args.length, "k": k, "tigs": len(tig_off) - 1, "index_characters": int(tig_off[-1]),
           "query_records": len(q_off) - 1, "query_characters": int(q_off[-1]), "preparation_s": round(prep_s, 1), "reps": []}
    for rep in range(args.reps):
        t0 = time.perf_counter()
        ix = api.KmerIndex((tig_seq, tig_off), k, args.device)
        build_wall = time.perf_counter() - t0
        t0 = time.perf_counter()
        r = ix.query((q_seq, q_off), bits=True)
        query_wall = time.perf_counter() - t0
        t = api.last_kmer_query_times()
        info = ix.info
        ix.close()
        windows, valid, found = int(r.kmers.sum()), int(r.valid.sum()), int(r.found.sum())
        clean = int(r.found[:ua.n_unitigs].sum())
        out = {"rep": rep, **{f: round(v, 3) for f, v in t.items()}, "build_wall_ms": round(1e3 * build_wall, 3),
               "query_wall_ms": round(1e3 * query_wall, 3), "distinct": info.distinct, "index_occurrences": info.occurrences,
               "table_slots": info.slots, "index_device_bytes": info.device_bytes, "windows": windows, "valid": valid, "found": found,
               "clean_half_all_found": clean == int(r.kmers[:ua.n_unitigs].sum()),
               "probe_windows_per_s": round(windows / (t["query_probe_ms"] * 1e-3)),
               "probe_ns_per_window": round(1e6 * t["query_probe_ms"] / windows, 4),
               "build_insert_ns_per_window": round(1e6 * t["build_insert_ms"] / max(1, info.occurrences), 4)}
        doc["reps"].append(out)
        print(json.dumps(out), flush=True)
        del r
    api.release_device_memory(args.device)

    # (a) the nearest kernel of the parent: the comparison's insert of B (the unitigs) into the table that holds A (the tigs)
    doc["compare_insert_b"] = []
    for rep in range(args.reps):
        c = api.compare_kmer_sets((tig_seq, tig_off), (ua.seq, ua.off), k, args.device)
        t = api.last_kmer_compare_times()
        out = {"rep": rep, "insert_a_ms": round(t["insert_a_ms"], 3), "insert_b_ms": round(t["insert_b_ms"], 3), "windows_b": c.occurrences_b,
               "insert_b_ns_per_window": round(1e6 * t["insert_b_ms"] / c.occurrences_b, 4), "equal": c.equal}
        doc["compare_insert_b"].append(out)
        print(json.dumps({"compare_insert_b": out}), flush=True)
    api.release_device_memory(args.device)
    probe = [r["probe_ns_per_window"] for r in doc["reps"][1:] or doc["reps"]]
    ins = [r["insert_b_ns_per_window"] for r in doc["compare_insert_b"][1:] or doc["compare_insert_b"]]
    doc["probe_ns_per_window_min_max"] = [min(probe), max(probe)]
    doc["compare_insert_b_ns_per_window_min_max"] = [min(ins), max(ins)]
    # two readings of "not slower beyond the run-to-run spread": the lenient one sets the probe's best against the insert's worst
    # repetition, the strict one best against best (the first repetition of each, which pays the arena's first chunks, left out)
    doc["probe_not_slower_per_window_than_insert_b"] = {"best_probe_vs_worst_insert": min(probe) <= max(ins),
                                                         "best_probe_vs_best_insert": min(probe) <= min(ins)}

    if not args.no_baseline:  # (b) torch: codes of both sides + searchsorted, the clean half of the query only
        def baseline():
            t0 = time.perf_counter()
            ci, _ = synth.kmer_codes_of_sequences_torch(tig_seq, tig_off, k)
            cq, n_occ = synth.kmer_codes_of_sequences_torch(ua.seq, ua.off, k)
            dev = f"cuda:{args.device}"
            a = torch.from_numpy(ci.view(np.int64) ^ np.int64(-2 ** 63)).to(dev)  # (order-preserving map of uint64 to int64)
            b = torch.from_numpy(cq.view(np.int64) ^ np.int64(-2 ** 63)).to(dev)
            at = torch.searchsorted(a, b).clamp_(max=len(a) - 1)
            hits = int((a[at] == b).sum())
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0), hits, int(n_occ)

        baseline()  # warm-up
        doc["baseline_torch_note"] = ("not like for like: kmer_codes_of_sequences_torch returns each side's distinct sorted codes, so the "
                                      "searchsorted looks up distinct k-mers, not every window, and answers nothing per record; the codes "
                                      "go device -> host -> device on the way, which total_ms includes")
        doc["baseline_torch"] = []
        for rep in range(2):
            ms, hits, n_occ = baseline()
            doc["baseline_torch"].append({"rep": rep, "total_ms": round(ms, 3), "distinct_found": hits, "windows": n_occ})
            print(json.dumps({"baseline_torch": doc["baseline_torch"][-1]}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
