"""clip_tips_timing.py -- what tip clipping costs the unitig compaction (`--clip-tips`, mtg_compact_unitigs_cleaned) on the
input of DESIGN.md 16: the four haplotypes of G-seq (tools/compact_timing.py's arrays), k = 31, m = 2, plus about 1 % of planted tips
-- one record per tip, k - 1 bases of haplotype 0, a base that differs from the next one, and 0 .. k - 2 random bases, every record
given twice (once per strand) so that it passes the threshold. Per repetition the twelve figures of mtg_last_compact_times, the two of
mtg_last_clean_times, the counts and the arena's peak, for
  off    the cleaned call with both lengths 0 -- the kernels of the counted call, nothing else;
  clip   one round at L = k;
  parent the library of the PARENT commit, built aside and named by --parent-library, running mtg_compact_unitigs_counted on the same
         input in a child process of its own (the two libraries never share a process), by ctypes alone.
Recorded: (a) off / parent and (b) clip / parent over the whole call and per phase, each from the fastest repetition after the first,
and beside them the spread of the parent's own repetitions (slowest / fastest after the first): a ratio inside that spread says nothing.

usage: python tools/clip_tips_timing.py --parent-library PATH [--length 100000000] [--k 31] [--tips-per-cent 1.0] [--reps 5]
                                        [--device 0] [--child-timeout 1200] [--out profiles/clip_tips_gseq_1e8.json]
Without --parent-library the ratios are left out."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

TIMES = ("upload_ms", "pack_ms", "insert_ms", "ids_ms", "nodes_ms", "rank_ms", "emit_ms", "download_ms", "total_ms", "rounds", "bytes",
         "peak_arena_bytes")
M = 2


def _rounded(t: dict) -> dict:
    return {f: (round(v, 3) if isinstance(v, float) else v) for f, v in t.items()}


def tipped_arrays(length: int, k: int, per_cent: float):
    """compact_timing.haplotype_arrays plus the tip records -> (data, offsets, tips, planted k-mers). The sites are evenly spaced over
    haplotype 0, at least 2 k apart; tip i has 1 + i mod (k - 1) k-mers."""
    from compact_timing import haplotype_arrays
    from matchtigs_amd import synth

    data, off = haplotype_arrays(length, 1)
    n = max(1, min(int(length * per_cent / 100.0 / ((k - 1) / 2.0 + 1)), (length - 4 * k) // (2 * k)))  # about per_cent % of the k-mers of a haplotype
    sites = (2 * k + np.arange(n, dtype=np.int64) * ((length - 4 * k) // n))
    kmers = 1 + np.arange(n, dtype=np.int64) % (k - 1)
    lens = k - 1 + kmers
    starts = np.concatenate([[0], np.cumsum(lens)])
    rec = np.repeat(np.arange(n), lens)
    within = np.arange(int(starts[-1])) - starts[rec]
    code = {ord(c): i for i, c in enumerate("ACGT")}
    lut = np.zeros(256, np.int64)
    for c, i in code.items():
        lut[c] = i
    abc = np.frombuffer(b"ACGT", np.uint8)
    noise = (synth.splitmix64(7, int(starts[-1]), 90) % np.uint64(4)).astype(np.int64)
    genome_at = np.minimum(sites[rec] + within, length - 1)
    bases = np.where(within < k - 1, lut[data[genome_at]], noise)
    fork = within == k - 1  # differs from the genome's next base
    bases[fork] = (lut[data[genome_at[fork]]] + 1 + noise[fork] % 3) % 4
    fwd = abc[bases]
    # the reverse complement of every record, record by record
    back = (starts[rec + 1] - 1 - within)
    rc = abc[3 - bases[back]]
    tips = np.concatenate([fwd, rc])
    tip_off = np.concatenate([starts[:-1], starts[-1] + starts]).astype(np.uint64) + np.uint64(len(data))
    return np.concatenate([data, tips]), np.concatenate([off[:-1], tip_off]), n, int(kmers.sum())


def parent_child(args) -> None:
    """In the child: the counted compaction of the library MATCHTIGS_LIBRARY names, by ctypes alone. One JSON line per repetition."""
    from matchtigs_amd import _lib

    L = C.CDLL(os.environ["MATCHTIGS_LIBRARY"])
    L.mtg_compact_unitigs_counted.restype = None
    L.mtg_compact_unitigs_counted.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_void_p),
                                              C.POINTER(_lib.MtgCompaction), C.POINTER(_lib.MtgAbundance), C.POINTER(C.c_void_p)]
    L.mtg_unitigs_free.argtypes = [C.c_void_p]
    L.mtg_abundance_sums_free.argtypes = [C.c_void_p]
    L.mtg_last_compact_times.argtypes = [C.POINTER(C.c_double)]
    data, off, _, _ = tipped_arrays(args.length, args.k, args.tips_per_cent)
    for rep in range(args.reps):
        out, sums, stats, ab, times = C.c_void_p(), C.c_void_p(), _lib.MtgCompaction(), _lib.MtgAbundance(), (C.c_double * 12)()
        t0 = time.perf_counter()
        L.mtg_compact_unitigs_counted(data.ctypes.data, off.ctypes.data, len(off) - 1, args.k, M, args.device, C.byref(out), C.byref(stats),
                                      C.byref(ab), C.byref(sums))
        wall = time.perf_counter() - t0
        L.mtg_last_compact_times(times)
        L.mtg_unitigs_free(out)
        L.mtg_abundance_sums_free(sums)
        t = dict(zip(TIMES, list(times)))
        for f in TIMES[9:]:
            t[f] = int(t[f])
        print(json.dumps({"rep": rep, **_rounded(t), "wall_ms": round(1e3 * wall, 3), **stats.as_dict()}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=100_000_000)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--tips-per-cent", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--parent-library", help="libmatchtigs.so of the parent commit, built aside")
    ap.add_argument("--child-timeout", type=float, default=1200.0, help="seconds the parent library's child process may take")
    ap.add_argument("--parent-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.parent_child:
        return parent_child(args)

    from matchtigs_amd import api

    doc = {"tool": "clip_tips_timing", "length": args.length, "haplotypes": 4, "k": args.k, "min_abundance": M, "runs": {}}
    if args.parent_library:  # first, in a process of its own
        env = dict(os.environ, MATCHTIGS_LIBRARY=os.path.abspath(args.parent_library))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--parent-child", "--length", str(args.length), "--k", str(args.k),
                            "--tips-per-cent", str(args.tips_per_cent), "--reps", str(args.reps), "--device", str(args.device)],
                           env=env, capture_output=True, text=True, timeout=args.child_timeout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            raise SystemExit(f"the parent library's run failed with status {r.returncode}")
        doc["parent"] = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
        for rep in doc["parent"]:
            print(json.dumps({"parent": rep}), flush=True)
    data, off, n_tips, planted = tipped_arrays(args.length, args.k, args.tips_per_cent)
    doc["tips"], doc["tip_kmers"] = n_tips, planted
    for name, clip in (("off", 0), ("clip", args.k)):
        reps = []
        for rep in range(args.reps):
            t0 = time.perf_counter()
            store, c, a, _, _, cl = api.compact_unitigs_cleaned((data, off), args.k, clip_tips=clip, min_abundance=M, device_id=args.device)
            wall = time.perf_counter() - t0
            reps.append({"rep": rep, "clip_tips": clip, **_rounded(api.last_compact_times()), **_rounded(api.last_clean_times()),
                         "wall_ms": round(1e3 * wall, 3), "distinct_kept": a.distinct_kept, "distinct_kmers": c.distinct_kmers,
                         "unitigs": c.unitigs, "closed_walks": c.closed_walks, "tips": cl.tips, "tip_kmers": cl.tip_kmers,
                         "removed_occurrences": cl.removed_occurrences})
            print(json.dumps(reps[-1]), flush=True)
            del store
        doc["runs"][name] = reps
    api.release_device_memory(args.device)

    def best(reps, field):  # the first repetition also pays the arena's first chunks
        return min(r[field] for r in (reps[1:] or reps))

    phases = ("insert_ms", "ids_ms", "nodes_ms", "rank_ms", "emit_ms", "total_ms")
    doc["summary"] = {name: {**{f: best(doc["runs"][name], f) for f in phases + ("peak_arena_bytes",)},
                             "clean_ms": best(doc["runs"][name], "clean_ms"), "rounds_run": doc["runs"][name][-1]["rounds_run"]}
                      for name in ("off", "clip")}
    if args.parent_library:
        later = doc["parent"][1:] or doc["parent"]
        doc["summary"]["parent"] = {**{f: best(doc["parent"], f) for f in phases + ("peak_arena_bytes",)},
                                    "spread": {f: round(max(r[f] for r in later) / min(r[f] for r in later), 3) for f in phases}}
        for name, label in (("off", "a_off_over_parent"), ("clip", "b_clip_over_parent")):
            doc["summary"][label] = {f: round(doc["summary"][name][f] / doc["summary"]["parent"][f], 3) for f in phases}
        doc["summary"]["off_counts_equal_parent"] = all(doc["runs"]["off"][0][f] == doc["parent"][0][f] for f in ("distinct_kmers", "unitigs", "closed_walks"))
    print(json.dumps({"summary": doc["summary"]}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
