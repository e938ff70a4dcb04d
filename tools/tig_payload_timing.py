"""tig_payload_timing.py -- what abundances and colours from the sparse minimizer index cost (api.TigIndex.annotated)
beside the weighted / coloured table, on the workload of tools/tig_index_timing.py: G-seq, the query = the unitigs plus an equal volume
of the same unitigs with 3 % substitutions and an `N` every ~10^3 bases.

The parent process starts no GPU work. Every GPU step is a child process under its own `timeout`; the first that fails ends the run:
  prepare          the unitigs, the greedy tigs (device order), the query and the payloads, written as .npy files into --work.
                   PAYLOAD MODEL (synthetic, stated in the JSON): weights = a walk along the unitigs' windows that starts at 30 and
                   moves by +-1 with probability --change (0.4: about what 30 x coverage by 150-base reads does to a depth profile),
                   never below 1; masks = one random non-empty subset of 4 colours per unitig. The greedy tigs' payloads are read off a
                   transient annotated table over the unitigs, as the command line does it.
  sparse           over the unitigs and over the greedy tigs, dense and runs: the annotated TigIndex -- device bytes, bytes per distinct
                   k-mer, per payload layout / width / runs per window / bytes, the payload build's phases -- and TigIndex.locate's,
                   .abundance's and .color_hits' phases
  table            the annotated KmerIndex over the unitigs: device bytes, KmerIndex.abundance's and .color_hits' probes
The answers of all steps must agree (the sum of the sums, the per-colour totals, found), which the parent checks. `best` is the fastest
repetition after the first. No speed or size is promised. The membership and locate probes against the parent commit's library are
tools/tig_locate_timing.py's guard (--parent-library), whose kernels this feature does not touch; it is not repeated here.

usage: python tools/tig_payload_timing.py [--length 100000000] [--k 31] [--m 19] [--reps 3] [--device 0] [--change 0.4] [--work DIR]
                                          [--step-timeout 900] [--out profiles/tig_payload_gseq_1e8.json]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

N_COLORS = 4


def save(work, **arrays):
    for name, a in arrays.items():
        np.save(os.path.join(work, name + ".npy"), np.asarray(a))


def load(work, *names):
    return [np.ascontiguousarray(np.load(os.path.join(work, n + ".npy"))) for n in names]


def windows_of(off, k):
    return np.maximum(np.diff(off.astype(np.int64)) - (k - 1), 0)


def prepare_step(args) -> None:
    import torch

    from kmer_compare_timing import fasta_sequence_arrays
    from matchtigs_amd import api, synth

    k, t0 = args.k, time.perf_counter()
    ua = synth.g_seq_arrays_torch(args.length, seed=1, k=k, device=f"cuda:{args.device}")
    torch.cuda.empty_cache()
    G = api.Bigraph.from_unitig_links_arrays(ua.weights, ua.links)
    lim, ed = api.GreedytigAlgorithm.compute_tigs_np(G, api.GreedytigAlgorithmConfiguration(1, k, euler_mode=api.EulerMode.Device,
                                                                                            device_ids=(args.device,)))
    tig_seq, tig_off = fasta_sequence_arrays(api.write_walks_text_device(G, (lim, ed), (ua.seq, ua.off), k, device_id=args.device))
    del G, lim, ed
    api.release_device_memory(args.device)
    rng = np.random.default_rng(1)
    u_off = ua.off.astype(np.uint64)
    n_win = windows_of(u_off, k)
    W = int(n_win.sum())
    steps = np.where(rng.random(W) < args.change, rng.integers(0, 2, W) * 2 - 1, 0).astype(np.int64)
    first = np.cumsum(n_win) - n_win  # every unitig starts again at 30
    steps[first[n_win > 0]] = 0
    walk = np.cumsum(steps)
    walk -= np.repeat(walk[first[n_win > 0]], n_win[n_win > 0])
    weights = np.maximum(30 + walk, 1).astype(np.uint32)
    masks = np.repeat(rng.integers(1, 1 << N_COLORS, len(n_win), dtype=np.uint64), n_win)
    with api.KmerIndex((ua.seq, u_off), k, args.device, weights=weights, colors=masks, n_colors=N_COLORS) as table:  # the tigs' payloads
        tw, tc, at = [], [], 0
        t_off = tig_off.astype(np.int64)
        while at < len(t_off) - 1:
            end = max(at + 1, int(np.searchsorted(t_off, int(t_off[at]) + (1 << 27), side="right")) - 1)
            piece = (np.ascontiguousarray(tig_seq[t_off[at]:t_off[end]]), (t_off[at:end + 1] - t_off[at]).astype(np.uint64))
            a, c = table.abundance(piece, per_window=True), table.color_hits(piece, per_window=True)
            if not np.array_equal(a.found, a.kmers):
                raise SystemExit("a window of a greedy tig is not a k-mer of the unitigs")
            n = a.kmers.astype(np.int64)
            rec = np.repeat(np.arange(at, end), n)
            pos = (t_off[rec] - t_off[at]) + (np.arange(len(rec)) - np.repeat(np.cumsum(n) - n, n))
            tw.append(a.per_window[pos])
            tc.append(c.per_window[pos])
            at = end
    n = len(ua.seq)
    noisy = ua.seq.copy()
    sub = rng.random(n) < 0.03
    noisy[sub] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(sub.sum()))]
    noisy[rng.random(n) < 1e-3] = ord("N")
    save(args.work, unitigs_seq=ua.seq, unitigs_off=u_off, unitigs_weights=weights, unitigs_masks=masks, greedytigs_seq=tig_seq,
         greedytigs_off=tig_off.astype(np.uint64), greedytigs_weights=np.concatenate(tw), greedytigs_masks=np.concatenate(tc),
         query_seq=np.concatenate([ua.seq, noisy]), query_off=np.concatenate([u_off, u_off[1:] + u_off[-1]]).astype(np.uint64))
    print(json.dumps({"step": "prepare", "distinct_kmers": len(ua.kmers), "unitigs": len(u_off) - 1, "unitig_windows": W,
                      "greedytigs": len(tig_off) - 1, "greedytig_windows": int(windows_of(tig_off, k).sum()), "query_records": 2 * (len(u_off) - 1),
                      "query_characters": 2 * n, "seconds": round(time.perf_counter() - t0, 1)}), flush=True)


def answers(ab, ch):
    return {"found": int(ab.found.sum()), "valid": int(ab.valid.sum()), "sum_of_sums": int(ab.sum.sum()), "max_of_max": int(ab.max.max()),
            "min_sum": int(ab.min.astype(np.uint64).sum()), "per_color_totals": ch.per_color.astype(np.uint64).sum(axis=0).tolist()}


def measure_step(args) -> None:
    from matchtigs_amd import api

    k = args.k
    seq, off, weights, masks = load(args.work, args.over + "_seq", args.over + "_off", args.over + "_weights", args.over + "_masks")
    query = tuple(load(args.work, "query_seq", "query_off"))
    for rep in range(args.reps):
        t0 = time.perf_counter()
        if args.step == "table":
            ix = api.KmerIndex((seq, off), k, args.device, weights=weights, colors=masks, n_colors=N_COLORS)
            out = {"build_kernels_ms": round(sum(v for f, v in api.last_kmer_query_times().items() if f in ("build_pack_ms", "build_insert_ms")), 3)}
        else:
            ix = api.TigIndex.annotated((seq, off), k, args.m, args.device, weights=weights, colors=masks, n_colors=N_COLORS, payload_layout=args.layout)
            tb, tp = api.last_tig_index_times(), api.last_tig_payload_times()
            out = {"build_kernels_ms": round(sum(v for f, v in tb.items() if f.startswith("build_") and f != "build_upload_ms"), 3),
                   "payload_build_ms": {p: {f: round(v, 3) for f, v in tp[p].items()} for p in ("weights", "colors")},
                   "payloads": {p: dict(v, runs_per_window=round(v["runs"] / max(v["windows"], 1), 5)) for p, v in ix.payload_info.items()}}
        out.update(step=args.step, over=args.over, layout=args.layout, rep=rep, build_wall_ms=round(1e3 * (time.perf_counter() - t0), 3),
                   device_bytes=ix.info.device_bytes, occurrences=ix.info.occurrences)
        if args.step == "sparse":
            loc = ix.locate(query)
            tl = api.last_tig_locate_times()
            out.update(locate_probe_ms=round(tl["probe_ms"], 3), locate_runs_ms=round(tl["runs_ms"], 3), locate_found=int(loc.found.sum()))
            del loc
        ab = ix.abundance(query)
        ta = api.last_tig_payload_times() if args.step == "sparse" else api.last_kmer_abundance_times()
        ch = ix.color_hits(query)
        tc = api.last_tig_payload_times() if args.step == "sparse" else api.last_kmer_color_times()
        out.update(abundance_probe_ms=round(ta["probe_ms"], 3), colors_probe_ms=round(tc["probe_ms"], 3), answers=answers(ab, ch))
        if args.step == "sparse":
            out.update(abundance_gather_ms=round(ta["gather_ms"], 3), colors_gather_ms=round(tc["gather_ms"], 3))
        del ab, ch
        ix.close()
        print(json.dumps(out), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=100_000_000)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--m", type=int, default=None, help="minimizer length (default: the library's, 19 at k = 31)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--change", type=float, default=0.4, help="probability that the weight moves by +-1 from one window to the next")
    ap.add_argument("--work", help="directory for the steps' inputs (default: a temporary one)")
    ap.add_argument("--step-timeout", type=int, default=900, help="seconds a child may take")
    ap.add_argument("--out")
    ap.add_argument("--step", choices=("prepare", "sparse", "table"), help=argparse.SUPPRESS)
    ap.add_argument("--over", default="unitigs", help=argparse.SUPPRESS)
    ap.add_argument("--layout", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step == "prepare":
        return prepare_step(args)
    if args.step:
        return measure_step(args)

    with tempfile.TemporaryDirectory() as tmp:
        work = args.work or tmp
        os.makedirs(work, exist_ok=True)

        def child(step, *extra):
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, "--k", str(args.k),
                   "--device", str(args.device), "--work", work, "--reps", str(args.reps), "--length", str(args.length), "--change", str(args.change)]
            cmd += (["--m", str(args.m)] if args.m else []) + list(extra)
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:  # nothing more is started on the GPU
                sys.stderr.write(r.stderr[-4000:])
                raise SystemExit(f"step {step} {' '.join(extra)} ended with status {r.returncode}")
            rows = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
            for row in rows:
                print(json.dumps(row), flush=True)
            return rows

        prep = child("prepare")[-1]
        distinct = prep["distinct_kmers"]
        doc = {"tool": "tig_payload_timing", "length": args.length, "k": args.k, "n_colors": N_COLORS,
               "payload_model": {"weights": f"walk from 30 per unitig, +-1 with probability {args.change} per window, at least 1",
                                 "masks": f"one random non-empty subset of {N_COLORS} colours per unitig",
                                 "greedytigs": "read off a transient annotated table over the unitigs"}, "workload": prep, "runs": {}}
        steps = [("table", "unitigs", None)] + [("sparse", over, layout) for over in ("unitigs", "greedytigs") for layout in ("dense", "runs")]
        for step, over, layout in steps:
            reps = child(step, "--over", over, *(["--layout", layout] if layout else []))
            later = reps[1:] or reps
            best = {f: min(x[f] for x in later) for f in ("build_kernels_ms", "locate_probe_ms", "abundance_probe_ms", "abundance_gather_ms",
                                                          "colors_probe_ms", "colors_gather_ms") if f in reps[0]}
            doc["runs"][f"{step}/{over}" + (f"/{layout}" if layout else "")] = {
                "device_bytes": reps[0]["device_bytes"], "bytes_per_distinct_kmer": round(reps[0]["device_bytes"] / distinct, 4),
                "payloads": reps[0].get("payloads"), "answers": reps[0]["answers"], "best": best, "reps": reps}
    first = doc["runs"]["table/unitigs"]["answers"]
    doc["answers_equal"] = all(r["answers"] == first for r in doc["runs"].values())
    tab = doc["runs"]["table/unitigs"]
    doc["ratios"] = {}
    for name, r in doc["runs"].items():
        if name.startswith("sparse"):
            b = r["best"]
            doc["ratios"][name] = {"device_bytes_over_table": round(r["device_bytes"] / tab["device_bytes"], 4),
                                   "abundance_over_locate_probe": round((b["abundance_probe_ms"] + b["abundance_gather_ms"]) / b["locate_probe_ms"], 4),
                                   "colors_over_locate_probe": round((b["colors_probe_ms"] + b["colors_gather_ms"]) / b["locate_probe_ms"], 4),
                                   "abundance_over_table": round((b["abundance_probe_ms"] + b["abundance_gather_ms"]) / tab["best"]["abundance_probe_ms"], 4),
                                   "colors_over_table": round((b["colors_probe_ms"] + b["colors_gather_ms"]) / tab["best"]["colors_probe_ms"], 4)}
    print(json.dumps({"answers_equal": doc["answers_equal"], "ratios": doc["ratios"]}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    if not doc["answers_equal"]:
        raise SystemExit("the steps disagree on the answers")


if __name__ == "__main__":
    main()
