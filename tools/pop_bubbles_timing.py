"""pop_bubbles_timing.py -- what bubble popping costs the cleaned unitig compaction (`--pop-bubbles`, mtg_compact_unitigs_simplified,
DESIGN.md 25) on the input of DESIGN.md 24 (tools/clip_tips_timing.py: the four haplotypes of G-seq plus about 1 % of planted tips, k = 31,
m = 2) plus about 1 % of planted SNP bubbles -- one record of 2 k - 1 bases of haplotype 0 per site with its middle base changed, every
record given twice (once per strand) so that it passes the threshold. Every call clips tips in one round at L = k. Per repetition the
twelve figures of mtg_last_compact_times, mtg_last_clean_times, mtg_last_bubble_times, the counts and the arena's peak, for
  off    the simplified call with max_arm_kmers 0 -- the kernels of the cleaned call, nothing else;
  pop    the simplified call with one round at L = 2 k, R = 1;
  parent the library of the PARENT commit, built aside and named by --parent-library, running mtg_compact_unitigs_cleaned on the same
         input in a child process of its own (the two libraries never share a process), by ctypes alone.
Recorded: (a) off / parent and (b) pop / parent over the whole call and per phase, each from the fastest repetition after the first,
and beside them the spread of the parent's own repetitions (slowest / fastest after the first): a ratio inside that spread says nothing.

usage: python tools/pop_bubbles_timing.py --parent-library PATH [--length 100000000] [--k 31] [--tips-per-cent 1.0] [--snps-per-cent 1.0]
                                          [--reps 5] [--device 0] [--child-timeout 1200] [--out profiles/pop_bubbles_gseq_1e8.json]
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

from clip_tips_timing import M, TIMES, _rounded, tipped_arrays  # noqa: E402


def bubbled_arrays(length: int, k: int, tips_per_cent: float, snps_per_cent: float):
    """clip_tips_timing.tipped_arrays plus the SNP records -> (data, offsets, tips, SNP sites). The sites are evenly spaced over
    haplotype 0, at least 4 k apart and half a stride from the tips' sites; every arm has k k-mers."""
    data, off, n_tips, _ = tipped_arrays(length, k, tips_per_cent)
    n = max(1, min(int(length * snps_per_cent / 100.0 / k), (length - 8 * k) // (4 * k)))  # about per_cent % of the k-mers of a haplotype
    stride = (length - 8 * k) // n
    sites = 4 * k + stride // 2 + np.arange(n, dtype=np.int64) * stride
    rows = data[sites[:, None] + np.arange(-(k - 1), k, dtype=np.int64)[None, :]].copy()  # [n, 2 k - 1], the site in the middle
    lut = np.zeros(256, np.int64)
    for i, c in enumerate(b"ACGT"):
        lut[c] = i
    abc = np.frombuffer(b"ACGT", np.uint8)
    rows[:, k - 1] = abc[(lut[rows[:, k - 1]] + 1 + np.arange(n) % 3) % 4]
    back = abc[3 - lut[rows[:, ::-1]]]
    snps = np.concatenate([rows.ravel(), back.ravel()])
    starts = np.arange(2 * n + 1, dtype=np.uint64) * np.uint64(2 * k - 1) + np.uint64(len(data))
    return np.concatenate([data, snps]), np.concatenate([off[:-1], starts]), n_tips, n


def parent_child(args) -> None:
    """In the child: the cleaned compaction of the library MATCHTIGS_LIBRARY names, by ctypes alone. One JSON line per repetition."""
    from matchtigs_amd import _lib

    L = C.CDLL(os.environ["MATCHTIGS_LIBRARY"])
    vp, u64, P = C.c_void_p, C.c_uint64, C.POINTER
    L.mtg_compact_unitigs_cleaned.restype = None
    L.mtg_compact_unitigs_cleaned.argtypes = [vp, vp, u64, u64, u64, vp, u64, C.c_int, P(_lib.MtgCleaningParams), C.c_int, P(vp), P(_lib.MtgCompaction),
                                              P(_lib.MtgAbundance), P(vp), P(vp), P(vp), P(_lib.MtgColorStats), P(vp), P(_lib.MtgCleaning)]
    L.mtg_unitigs_free.argtypes = [vp]
    L.mtg_abundance_sums_free.argtypes = [vp]
    L.mtg_last_compact_times.argtypes = [P(C.c_double)]
    L.mtg_last_clean_times.argtypes = [P(C.c_double)]
    data, off, _, _ = bubbled_arrays(args.length, args.k, args.tips_per_cent, args.snps_per_cent)
    for rep in range(args.reps):
        out, sums, stats, ab, cl = vp(), vp(), _lib.MtgCompaction(), _lib.MtgAbundance(), _lib.MtgCleaning()
        params, times, clean = _lib.MtgCleaningParams(args.k, 0, 1), (C.c_double * 12)(), (C.c_double * 2)()
        t0 = time.perf_counter()
        L.mtg_compact_unitigs_cleaned(data.ctypes.data, off.ctypes.data, len(off) - 1, args.k, M, None, 0, 0, C.byref(params), args.device, C.byref(out),
                                      C.byref(stats), C.byref(ab), C.byref(sums), None, None, None, None, C.byref(cl))
        wall = time.perf_counter() - t0
        L.mtg_last_compact_times(times)
        L.mtg_last_clean_times(clean)
        L.mtg_unitigs_free(out)
        L.mtg_abundance_sums_free(sums)
        t = dict(zip(TIMES, list(times)))
        for f in TIMES[9:]:
            t[f] = int(t[f])
        print(json.dumps({"rep": rep, **_rounded(t), "clean_ms": round(clean[0], 3), "wall_ms": round(1e3 * wall, 3), **stats.as_dict(),
                          "tips": int(cl.tips)}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=100_000_000)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--tips-per-cent", type=float, default=1.0)
    ap.add_argument("--snps-per-cent", type=float, default=1.0)
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

    doc = {"tool": "pop_bubbles_timing", "length": args.length, "haplotypes": 4, "k": args.k, "min_abundance": M, "clip_tips": args.k, "runs": {}}
    if args.parent_library:  # first, in a process of its own
        env = dict(os.environ, MATCHTIGS_LIBRARY=os.path.abspath(args.parent_library))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--parent-child", "--length", str(args.length), "--k", str(args.k),
                            "--tips-per-cent", str(args.tips_per_cent), "--snps-per-cent", str(args.snps_per_cent), "--reps", str(args.reps),
                            "--device", str(args.device)], env=env, capture_output=True, text=True, timeout=args.child_timeout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            raise SystemExit(f"the parent library's run failed with status {r.returncode}")
        doc["parent"] = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
        for rep in doc["parent"]:
            print(json.dumps({"parent": rep}), flush=True)
    data, off, n_tips, n_snps = bubbled_arrays(args.length, args.k, args.tips_per_cent, args.snps_per_cent)
    doc["tips"], doc["snps"] = n_tips, n_snps
    for name, pop in (("off", 0), ("pop", 2 * args.k)):
        reps = []
        for rep in range(args.reps):
            t0 = time.perf_counter()
            store, c, a, _, _, cl, bu = api.compact_unitigs_simplified((data, off), args.k, pop_bubbles=pop, clip_tips=args.k, min_abundance=M,
                                                                       device_id=args.device)
            wall = time.perf_counter() - t0
            reps.append({"rep": rep, "pop_bubbles": pop, **_rounded(api.last_compact_times()), **_rounded(api.last_clean_times()),
                         **_rounded(api.last_bubble_times()), "wall_ms": round(1e3 * wall, 3), "distinct_kept": a.distinct_kept,
                         "distinct_kmers": c.distinct_kmers, "unitigs": c.unitigs, "closed_walks": c.closed_walks, "tips": cl.tips, "arms": bu.arms,
                         "arm_kmers": bu.arm_kmers, "removed_occurrences": bu.removed_occurrences})
            print(json.dumps(reps[-1]), flush=True)
            del store
        doc["runs"][name] = reps
    api.release_device_memory(args.device)

    def best(reps, field):  # the first repetition also pays the arena's first chunks
        return min(r[field] for r in (reps[1:] or reps))

    phases = ("insert_ms", "ids_ms", "nodes_ms", "rank_ms", "emit_ms", "clean_ms", "total_ms")
    doc["summary"] = {name: {**{f: best(doc["runs"][name], f) for f in phases + ("peak_arena_bytes", "bubble_ms")},
                             "rounds_run": doc["runs"][name][-1]["rounds_run"], "arms": doc["runs"][name][-1]["arms"]} for name in ("off", "pop")}
    if args.parent_library:
        later = doc["parent"][1:] or doc["parent"]
        doc["summary"]["parent"] = {**{f: best(doc["parent"], f) for f in phases + ("peak_arena_bytes",)},
                                    "spread": {f: round(max(r[f] for r in later) / min(r[f] for r in later), 3) for f in phases}}
        for name, label in (("off", "a_off_over_parent"), ("pop", "b_pop_over_parent")):
            doc["summary"][label] = {f: round(doc["summary"][name][f] / doc["summary"]["parent"][f], 3) for f in phases}
        doc["summary"]["off_counts_equal_parent"] = all(doc["runs"]["off"][0][f] == doc["parent"][0][f]
                                                        for f in ("distinct_kmers", "unitigs", "closed_walks", "tips"))
    print(json.dumps({"summary": doc["summary"]}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
