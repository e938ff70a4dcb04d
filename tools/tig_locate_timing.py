"""tig_locate_timing.py -- what `locate` on the sparse minimizer index costs (api.TigIndex.locate, mtg_tig_index_locate)
beside its two yardsticks, on the workload of tools/tig_index_timing.py: G-seq, the query = the unitigs plus an equal volume of the same
unitigs with 3 % substitutions and an `N` every ~10^3 bases. In one process:
  over the unitigs and over the greedy tigs (device order): a plain and a locating TigIndex -- build kernels ms, device bytes --,
                    TigIndex.query's probe on each, TigIndex.locate's probe and runs phases, the number of runs
  over the unitigs: a locating KmerIndex -- build, device bytes, KmerIndex.locate's probe and runs phases; the two locates must return
                    equal arrays, which the tool checks
`--reps` repetitions each (HIP events around the kernels); `best` takes the fastest repetition after the first, which also pays the
arena's first chunks. No speed is promised: the ratios locate / query and sparse / table are what the JSON is for.

The guard on the membership query, whose code is not meant to change: with --parent-library (libmatchtigs.so of the parent commit, built
aside) the unitigs and the query are written once as .npy files into --work, and child processes -- each under its own `timeout`, the
first that fails ends the run -- load the parent's library and this one IN TURN through plain ctypes (the parent lacks the new entry
points, which matchtigs_amd._lib insists on), build the plain index over the unitigs, query twice and report the second probe. This
library's best probe must lie within the parent's own min .. max: the tool says so in the JSON, and ends with a non-zero status if it lies
above the parent's max or the answers differ.

usage: python tools/tig_locate_timing.py [--length 100000000] [--k 31] [--m 19] [--reps 3] [--device 0] [--parent-library PATH]
                                         [--guard-reps 5] [--work DIR] [--step-timeout 600] [--out profiles/tig_locate_gseq_1e8.json]
One JSON line per repetition; --out writes all of it as one JSON document."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

FILES = ("index_seq", "index_off", "query_seq", "query_off")


def guard_step(args) -> None:
    """One child of the guard: the library named by --library, plain ctypes, the plain index over the unitigs, two queries."""
    from matchtigs_amd import _lib  # (the structure's layout only; the library it would load is never asked for)

    L = C.CDLL(args.library)
    vp, u64 = C.c_void_p, C.c_uint64
    L.mtg_tig_index_build.restype = vp
    L.mtg_tig_index_build.argtypes = [vp, vp, u64, u64, u64, u64, C.c_int]
    L.mtg_tig_index_get_info.argtypes = [vp, C.POINTER(_lib.MtgTigIndexInfo)]
    L.mtg_tig_index_query.argtypes = [vp, vp, vp, u64, vp, vp, vp, vp, vp]
    L.mtg_tig_index_free.argtypes = [vp]
    L.mtg_last_tig_index_times.argtypes = [C.POINTER(C.c_double)]
    d = {f: np.ascontiguousarray(np.load(os.path.join(args.work, f + ".npy"))) for f in FILES}
    n_ix, n_q = len(d["index_off"]) - 1, len(d["query_off"]) - 1
    ix = L.mtg_tig_index_build(d["index_seq"].ctypes.data, d["index_off"].ctypes.data, n_ix, args.k, args.m or 0, 0, args.device)
    info = _lib.MtgTigIndexInfo()
    L.mtg_tig_index_get_info(ix, C.byref(info))
    kmers, valid, found = (np.zeros(n_q, np.uint64) for _ in range(3))
    words = (int(d["query_off"][-1]) + 63) // 64
    vb, pb = np.zeros(words, np.uint64), np.zeros(words, np.uint64)
    t = (C.c_double * 8)()
    for _ in range(2):  # the second call finds the arena's chunks in place
        L.mtg_tig_index_query(ix, d["query_seq"].ctypes.data, d["query_off"].ctypes.data, n_q, kmers.ctypes.data, valid.ctypes.data,
                              found.ctypes.data, pb.ctypes.data, vb.ctypes.data)
        L.mtg_last_tig_index_times(t)
    L.mtg_tig_index_free(ix)
    print(json.dumps({"step": "guard", "library": args.which, "rep": args.rep, "query_probe_ms": round(t[7], 3), "device_bytes": int(info.device_bytes),
                      "windows": int(kmers.sum()), "valid": int(valid.sum()), "found": int(found.sum()),
                      "present_bits_popcount": int(sum(bin(int(x)).count("1") for x in pb[:4096]))}), flush=True)


def best_of(reps, f):
    later = reps[1:] or reps
    return min(x[f] for x in later)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=100_000_000)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--m", type=int, default=None, help="minimizer length (default: the library's, 19 at k = 31)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--parent-library", help="libmatchtigs.so of the parent commit, built aside: the guard on the membership probe")
    ap.add_argument("--guard-reps", type=int, default=5, help="repetitions of each library in the guard (at least five: the spread)")
    ap.add_argument("--work", help="directory for the guard's inputs (default: a temporary one)")
    ap.add_argument("--step-timeout", type=int, default=600, help="seconds a child of the guard may take")
    ap.add_argument("--out")
    ap.add_argument("--step", choices=("guard",), help=argparse.SUPPRESS)
    ap.add_argument("--library", help=argparse.SUPPRESS)
    ap.add_argument("--which", help=argparse.SUPPRESS)
    ap.add_argument("--rep", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step == "guard":
        return guard_step(args)
    if args.parent_library and args.guard_reps < 5:
        ap.error("the spread needs at least five repetitions")

    import torch

    from kmer_compare_timing import fasta_sequence_arrays
    from matchtigs_amd import _lib, api, synth

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
    query = (q_seq, q_off)
    distinct = len(ua.kmers)
    doc = {"tool": "tig_locate_timing", "length": args.length, "k": k, "distinct_kmers": distinct, "query_records": len(q_off) - 1,
           "query_characters": int(q_off[-1]), "preparation_s": round(time.perf_counter() - t0, 1), "runs": {}}
    sets = {"unitigs": (ua.seq, ua.off.astype(np.uint64)), "greedytigs": (tig_seq, tig_off)}

    def build_kernels_ms(t):
        return sum(v for f, v in t.items() if f.startswith("build_") and f != "build_upload_ms")

    located = {}  # over the unitigs: the arrays of the two locates
    for over, indexed in sets.items():
        for kind in ("minimizer", "minimizer-locating") + (("table-locating",) if over == "unitigs" else ()):
            reps = []
            for rep in range(args.reps):
                t0 = time.perf_counter()
                if kind == "table-locating":
                    ix = api.KmerIndex(indexed, k, args.device, locate=True)
                    tb = api.last_kmer_query_times()
                else:
                    ix = api.TigIndex(indexed, k, args.m, args.device, locate=kind == "minimizer-locating")
                    tb = api.last_tig_index_times()
                out = {"over": over, "index": kind, "rep": rep, "build_wall_ms": round(1e3 * (time.perf_counter() - t0), 3),
                       "build_kernels_ms": round(build_kernels_ms(tb), 3), "device_bytes": ix.info.device_bytes}
                r = ix.query(query, bits=True)
                tq = api.last_kmer_query_times() if kind == "table-locating" else api.last_tig_index_times()
                windows = int(r.kmers.sum())
                out.update(query_probe_ms=round(tq["query_probe_ms"], 3), windows=windows, valid=int(r.valid.sum()), found=int(r.found.sum()))
                del r
                if kind != "minimizer":
                    t0 = time.perf_counter()
                    loc = ix.locate(query)
                    wall = time.perf_counter() - t0
                    tl = api.last_kmer_locate_times() if kind == "table-locating" else api.last_tig_locate_times()
                    out.update(locate_wall_ms=round(1e3 * wall, 3), locate_probe_ms=round(tl["probe_ms"], 3), locate_runs_ms=round(tl["runs_ms"], 3),
                               runs=len(loc.runs), locate_found=int(loc.found.sum()),
                               locate_probe_windows_per_s=round(windows / (tl["probe_ms"] * 1e-3)))
                    if over == "unitigs" and rep == 0:
                        located[kind] = loc
                    del loc
                info = ix.info
                ix.close()
                reps.append(out)
                print(json.dumps(out), flush=True)
            best = {f: best_of(reps, f) for f in ("build_kernels_ms", "query_probe_ms", "locate_probe_ms", "locate_runs_ms") if f in reps[0]}
            doc["runs"][f"{kind}/{over}"] = {"info": {f.name: getattr(info, f.name) for f in info.__dataclass_fields__.values()},
                                             "device_bytes": info.device_bytes, "bytes_per_distinct_kmer": round(info.device_bytes / distinct, 4),
                                             "best": best, "reps": reps}
            api.release_device_memory(args.device)
    a, b = located["minimizer-locating"], located["table-locating"]
    equal = all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("offsets", "kmers", "valid", "found", "runs"))
    doc["locates_over_the_unitigs_equal"] = bool(equal)
    if not equal:
        raise SystemExit("TigIndex.locate and KmerIndex.locate over the unitigs disagree")
    del located, a, b

    ratios = {}
    for over in sets:
        plain, loc = doc["runs"][f"minimizer/{over}"], doc["runs"][f"minimizer-locating/{over}"]
        ratios[over] = {"locating_over_plain_device_bytes": round(loc["device_bytes"] / plain["device_bytes"], 4),
                        "locating_over_plain_build_kernels_ms": round(loc["best"]["build_kernels_ms"] / plain["best"]["build_kernels_ms"], 4),
                        "locate_probe_over_query_probe": round(loc["best"]["locate_probe_ms"] / plain["best"]["query_probe_ms"], 4),
                        "locate_probe_plus_runs_over_query_probe": round((loc["best"]["locate_probe_ms"] + loc["best"]["locate_runs_ms"]) /
                                                                         plain["best"]["query_probe_ms"], 4),
                        "query_probe_on_locating_over_on_plain": round(loc["best"]["query_probe_ms"] / plain["best"]["query_probe_ms"], 4)}
    loc, tab = doc["runs"]["minimizer-locating/unitigs"], doc["runs"]["table-locating/unitigs"]
    ratios["sparse_over_table_unitigs"] = {"device_bytes": round(loc["device_bytes"] / tab["device_bytes"], 4),
                                           "build_kernels_ms": round(loc["best"]["build_kernels_ms"] / tab["best"]["build_kernels_ms"], 4),
                                           "locate_probe_ms": round(loc["best"]["locate_probe_ms"] / tab["best"]["locate_probe_ms"], 4),
                                           "locate_runs_ms": round(loc["best"]["locate_runs_ms"] / tab["best"]["locate_runs_ms"], 4)}
    doc["ratios"] = ratios
    print(json.dumps({"ratios": ratios}), flush=True)

    guard_ok = True
    if args.parent_library:
        with tempfile.TemporaryDirectory() as tmp:
            work = args.work or tmp
            os.makedirs(work, exist_ok=True)
            for f, v in zip(FILES, (*sets["unitigs"], q_seq, q_off)):
                np.save(os.path.join(work, f + ".npy"), np.asarray(v))
            libs = {"parent": os.path.abspath(args.parent_library), "new": str(_lib.LIB_PATH)}
            rows = {"parent": [], "new": []}
            for rep in range(args.guard_reps):
                for which in ("parent", "new"):  # in turn: what drifts on the machine meets both alike
                    cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", "guard", "--rep", str(rep),
                           "--k", str(k), "--device", str(args.device), "--work", work, "--library", libs[which], "--which", which]
                    if args.m:
                        cmd += ["--m", str(args.m)]
                    r = subprocess.run(cmd, capture_output=True, text=True)
                    if r.returncode != 0:  # nothing more is started on the GPU
                        sys.stderr.write(r.stderr[-4000:])
                        raise SystemExit(f"guard step {which} (repetition {rep}) ended with status {r.returncode}")
                    line = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")][-1]
                    print(json.dumps(line), flush=True)
                    rows[which].append(line)
        p, q = [x["query_probe_ms"] for x in rows["parent"]], [x["query_probe_ms"] for x in rows["new"]]
        same = all(rows["new"][0][f] == rows["parent"][0][f] for f in ("windows", "valid", "found", "device_bytes", "present_bits_popcount"))
        guard_ok = min(q) <= max(p) and same  # (a best below the parent's is noise in the welcome direction: reported, not refused)
        doc["membership_guard"] = {"parent_query_probe_ms": {"min": min(p), "max": max(p), "max_over_min": round(max(p) / min(p), 4)},
                                   "new_query_probe_ms": {"min": min(q), "max": max(q), "max_over_min": round(max(q) / min(q), 4)},
                                   "new_best_over_parent_best": round(min(q) / min(p), 4), "same_answers": bool(same),
                                   "new_best_within_parent_spread": bool(min(p) <= min(q) <= max(p)), "rows": rows}
        print(json.dumps({"membership_guard": {f: v for f, v in doc["membership_guard"].items() if f != "rows"}}), flush=True)
    else:
        doc["membership_guard"] = "not measured (no --parent-library given)"
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    if not guard_ok:
        raise SystemExit("the membership probe of this library lies outside the parent's own spread, or answers differently")


if __name__ == "__main__":
    main()
