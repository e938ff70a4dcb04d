"""abundance_timing.py -- what counting costs the unitig compaction (`--min-abundance`, mtg_compact_unitigs_counted) on
the input of DESIGN.md 16: the four haplotypes of G-seq (tools/compact_timing.py's arrays), k = 31. The counted call runs at m = 1
and m = 2; per repetition the twelve figures of mtg_last_compact_times (the spectrum sweep is booked under ids, the per-unitig sums
under emit) and the counts. The yardstick is the library of the PARENT commit, built aside and named by --parent-library: a child
process (a fresh one: the two libraries never share a process) loads it through MATCHTIGS_LIBRARY with plain ctypes -- it lacks
the new entry points, which matchtigs_amd._lib insists on -- and runs mtg_compact_unitigs on the same input. Recorded: counted insert /
parent insert and counted whole call / parent whole call, at m = 1 and m = 2, each from the fastest repetition after the first.

usage: python tools/abundance_timing.py --parent-library PATH [--length 100000000] [--k 31] [--reps 3] [--device 0]
                                        [--out profiles/abundance_gseq_1e8.json]
Without --parent-library the ratios are left out."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

TIMES = ("upload_ms", "pack_ms", "insert_ms", "ids_ms", "nodes_ms", "rank_ms", "emit_ms", "download_ms", "total_ms", "rounds", "bytes",
         "peak_arena_bytes")


def _rounded(t: dict) -> dict:
    return {f: (round(v, 3) if isinstance(v, float) else v) for f, v in t.items()}


def parent_child(args) -> None:
    """In the child: the plain compaction of the library MATCHTIGS_LIBRARY names, by ctypes alone. One JSON line per repetition."""
    from compact_timing import haplotype_arrays
    from matchtigs_amd import _lib

    L = C.CDLL(os.environ["MATCHTIGS_LIBRARY"])
    L.mtg_compact_unitigs.restype = None
    L.mtg_compact_unitigs.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_void_p), C.POINTER(_lib.MtgCompaction)]
    L.mtg_unitigs_free.argtypes = [C.c_void_p]
    L.mtg_last_compact_times.argtypes = [C.POINTER(C.c_double)]
    data, off = haplotype_arrays(args.length, 1)
    for rep in range(args.reps):
        out, stats, times = C.c_void_p(), _lib.MtgCompaction(), (C.c_double * 12)()
        t0 = time.perf_counter()
        L.mtg_compact_unitigs(data.ctypes.data, off.ctypes.data, len(off) - 1, args.k, args.device, C.byref(out), C.byref(stats))
        wall = time.perf_counter() - t0
        L.mtg_last_compact_times(times)
        L.mtg_unitigs_free(out)
        t = dict(zip(TIMES, list(times)))
        for f in TIMES[9:]:
            t[f] = int(t[f])
        print(json.dumps({"rep": rep, **_rounded(t), "wall_ms": round(1e3 * wall, 3), **stats.as_dict()}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=100_000_000)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--parent-library", help="libmatchtigs.so of the parent commit, built aside")
    ap.add_argument("--parent-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.parent_child:
        return parent_child(args)

    from compact_timing import haplotype_arrays
    from matchtigs_amd import api

    doc = {"tool": "abundance_timing", "length": args.length, "haplotypes": 4, "k": args.k, "counted": {}}
    if args.parent_library:  # first, in a process of its own
        env = dict(os.environ, MATCHTIGS_LIBRARY=os.path.abspath(args.parent_library))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--parent-child", "--length", str(args.length), "--k", str(args.k),
                            "--reps", str(args.reps), "--device", str(args.device)], env=env, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            raise SystemExit(f"the parent library's run failed with status {r.returncode}")
        doc["parent"] = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
        for rep in doc["parent"]:
            print(json.dumps({"parent": rep}), flush=True)
    data, off = haplotype_arrays(args.length, 1)
    for m in (1, 2):
        reps = []
        for rep in range(args.reps):
            t0 = time.perf_counter()
            store, c, a = api.compact_unitigs_counted((data, off), args.k, m, args.device)
            wall = time.perf_counter() - t0
            t = api.last_compact_times()
            reps.append({"rep": rep, "min_abundance": m, **_rounded(t), "wall_ms": round(1e3 * wall, 3), "windows": c.windows,
                         "distinct_kmers": c.distinct_kmers, "unitigs": c.unitigs, "unitig_characters": c.unitig_characters,
                         "closed_walks": c.closed_walks, "distinct_all": a.distinct_all, "dropped": a.dropped,
                         "max_abundance": a.max_abundance, "kept_occurrences": a.kept_occurrences,
                         "spectrum_head": a.spectrum[:9].tolist(), "unitig_sums_total": int(a.unitig_sums.sum())})
            print(json.dumps(reps[-1]), flush=True)
            del store
        doc["counted"][f"m{m}"] = reps
    api.release_device_memory(args.device)

    def best(reps, field):  # the first repetition also pays the arena's first chunks
        return min(r[field] for r in (reps[1:] or reps))

    doc["summary"] = {f"m{m}": {f: best(doc["counted"][f"m{m}"], f) for f in ("insert_ms", "ids_ms", "emit_ms", "total_ms", "peak_arena_bytes")}
                      for m in (1, 2)}
    if args.parent_library:
        p_insert, p_total = best(doc["parent"], "insert_ms"), best(doc["parent"], "total_ms")
        doc["summary"]["parent"] = {"insert_ms": p_insert, "total_ms": p_total, "peak_arena_bytes": best(doc["parent"], "peak_arena_bytes")}
        for m in (1, 2):
            s = doc["summary"][f"m{m}"]
            s["insert_over_parent_insert"] = round(s["insert_ms"] / p_insert, 3)
            s["total_over_parent_total"] = round(s["total_ms"] / p_total, 3)
        same = doc["counted"]["m1"][0]
        doc["summary"]["m1_counts_equal_parent"] = all(same[f] == doc["parent"][0][f] for f in ("windows", "distinct_kmers", "unitigs",
                                                                                                 "unitig_characters", "closed_walks"))
    print(json.dumps({"summary": doc["summary"]}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
