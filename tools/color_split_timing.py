"""color_split_timing.py -- what monochromatic unitigs and the colour classes cost (mtg_compact_unitigs_colored_classes)
on the input of DESIGN.md 22: the four haplotypes of G-seq (tools/kmer_color_timing.py's records), k = 31, one colour per haplotype
(C = 4) and 64 colours dealt round-robin over the records (C = 64).

Every GPU step is a child process of its own, under its own `timeout`, and the first one that fails ends the run:
  prepare         the records, written once as .npy files into --work (kmer_color_timing.py's; every later child reads the same bytes)
  parent <rep>    the PARENT commit's library, built aside and named by --parent-library, loaded through MATCHTIGS_LIBRARY with plain
                  ctypes: mtg_compact_unitigs_colored at C = 4 and C = 64 -- the yardstick
  new <rep>       this library: the coloured call (unchanged machine code but for succ_kernel's trailing argument: it must stay within
                  the parent's spread), and the classes call with split = 0 and split = 1, at C = 4 and C = 64: the twelve figures of
                  mtg_last_compact_times, the dictionary's phases, unitigs, classes, runs
  counts <rep>    the dictionary alone (mtg_color_classes_build) on two synthetic mask arrays of --counts-n windows: every window a run
                  of ONE class (one mask, every window a unitig of its own) and every window a run of its OWN class (distinct masks)
In every child a call is made twice and the second is reported: the first also pays the arena's chunks. At least five repetitions; the
parent's own spread (min, max, max / min) is written beside each ratio: whole call / parent's whole call, nodes + succ with SPLIT /
parent's nodes + succ, and the counts kernel on the one-class array / on the own-class array.

usage: python tools/color_split_timing.py [--parent-library PATH] [--length 100000000] [--pieces 64] [--k 31] [--reps 5] [--counts-n 100000000]
                                          [--device 0] [--work DIR] [--step-timeout 900] [--out profiles/color_split_gseq_1e8.json]
Without --parent-library the parent's figures and the ratios against it are left out. One JSON line per child; --out writes all of it."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from kmer_color_timing import TIMES, _load, _rounded, prepare  # noqa: E402

COLORINGS = ("4", "64")


def _colors(which, haplotype):
    return haplotype if which == "4" else (np.arange(len(haplotype)) % 64).astype(np.uint8)


def parent_step(args) -> None:
    from matchtigs_amd import _lib  # (the structures' layout only; the library it would load is never asked for)

    L = C.CDLL(os.environ["MATCHTIGS_LIBRARY"])
    vp, u64, P = C.c_void_p, C.c_uint64, C.POINTER
    L.mtg_compact_unitigs_colored.argtypes = [vp, vp, u64, u64, u64, vp, u64, C.c_int, P(vp), P(_lib.MtgCompaction), P(_lib.MtgAbundance), P(vp), P(vp),
                                              P(vp), P(_lib.MtgColorStats)]
    L.mtg_last_compact_times.argtypes = [P(C.c_double)]
    for f in ("mtg_unitigs_free", "mtg_abundance_sums_free", "mtg_kmer_counts_free", "mtg_kmer_colors_free"):
        getattr(L, f).restype, getattr(L, f).argtypes = None, [vp]
    seq, off, haplotype = _load(args.work)
    line = {"step": "parent", "rep": args.rep}
    for which in COLORINGS:
        rc = np.ascontiguousarray(_colors(which, haplotype))
        for _ in range(2):
            out, sums, counts, masks = vp(), vp(), vp(), vp()
            stats, ab, cs, times = _lib.MtgCompaction(), _lib.MtgAbundance(), _lib.MtgColorStats(), (C.c_double * 12)()
            t0 = time.perf_counter()
            L.mtg_compact_unitigs_colored(seq.ctypes.data, off.ctypes.data, len(off) - 1, args.k, 1, rc.ctypes.data, int(which), args.device, C.byref(out),
                                          C.byref(stats), C.byref(ab), C.byref(sums), C.byref(counts), C.byref(masks), C.byref(cs))
            wall = time.perf_counter() - t0
            L.mtg_last_compact_times(times)
            for free, h in ((L.mtg_unitigs_free, out), (L.mtg_abundance_sums_free, sums), (L.mtg_kmer_counts_free, counts), (L.mtg_kmer_colors_free, masks)):
                free(h)
        line[f"colored_{which}"] = {**_rounded(dict(zip(TIMES, list(times)))), "wall_ms": round(1e3 * wall, 3), "unitigs": int(stats.unitigs),
                                    "distinct_kmers": int(stats.distinct_kmers)}
    print(json.dumps(line), flush=True)


def new_step(args) -> None:
    from matchtigs_amd import api

    seq, off, haplotype = _load(args.work)
    line = {"step": "new", "rep": args.rep}
    for which in COLORINGS:
        rc = _colors(which, haplotype)
        for _ in range(2):
            t0 = time.perf_counter()
            plain = api.compact_unitigs_colored((seq, off), args.k, rc, int(which), device_id=args.device)
            wall = time.perf_counter() - t0
        line[f"colored_{which}"] = {**_rounded(api.last_compact_times()), "wall_ms": round(1e3 * wall, 3), "unitigs": plain[1].unitigs}
        for split in (0, 1):
            for _ in range(2):
                t0 = time.perf_counter()
                got = api.compact_unitigs_colored_classes((seq, off), args.k, rc, int(which), split=bool(split), device_id=args.device)
                wall = time.perf_counter() - t0
            cc = got[4]
            entry = {**_rounded(api.last_compact_times()), "wall_ms": round(1e3 * wall, 3), "classes_ms": _rounded(api.last_color_class_times()),
                     "unitigs": got[1].unitigs, "closed_walks": got[1].closed_walks, "longest_unitig_kmers": got[1].longest_unitig_kmers,
                     "classes": len(cc.masks), "runs": int(cc.runs.sum()), "largest_class_kmers": int(cc.kmers.max())}
            if split == 0:
                entry["equals_colored"] = bool(np.array_equal(got[0].arrays()[0], plain[0].arrays()[0]) and np.array_equal(got[0].arrays()[1], plain[0].arrays()[1])
                                               and np.array_equal(got[3].kmer_colors, plain[3].kmer_colors) and np.array_equal(got[2].kmer_counts, plain[2].kmer_counts))
            else:
                entry["monochromatic"] = bool(int(cc.runs.sum()) == got[1].unitigs)
                entry["statistics_equal_colored"] = bool(np.array_equal(got[3].shared, plain[3].shared) and np.array_equal(got[3].occupancy, plain[3].occupancy))
            line[f"classes_{which}_split{split}"] = entry
            del got
        del plain
    print(json.dumps(line), flush=True)


def counts_step(args) -> None:
    from matchtigs_amd import api

    n = args.counts_n
    line = {"step": "counts", "rep": args.rep, "n": n}
    for name, masks, unitigs in (("one_class", np.ones(n, np.uint64), np.ones(n, np.uint64)),
                                 ("own_class", np.arange(1, n + 1, dtype=np.uint64), np.array([n], np.uint64))):
        for _ in range(2):
            cc = api.color_classes(masks, unitigs, args.device)
        assert int(cc.runs.sum()) == n and len(cc.masks) == (1 if name == "one_class" else n) and int(cc.kmers.sum()) == n
        line[name] = {**_rounded(api.last_color_class_times()), "classes": len(cc.masks), "runs": int(cc.runs.sum())}
        del cc
    line["one_class_over_own_class_counts"] = round(line["one_class"]["counts_ms"] / line["own_class"]["counts_ms"], 4)
    print(json.dumps(line), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=100_000_000)
    ap.add_argument("--pieces", type=int, default=64, help="records per haplotype")
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--counts-n", type=int, default=100_000_000)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--parent-library", help="libmatchtigs.so of the parent commit, built aside")
    ap.add_argument("--work", help="directory for the prepared inputs (default: a temporary one)")
    ap.add_argument("--step-timeout", type=int, default=900, help="seconds a child may take")
    ap.add_argument("--step", choices=("prepare", "parent", "new", "counts"), help=argparse.SUPPRESS)
    ap.add_argument("--rep", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.step:
        return {"prepare": prepare, "parent": parent_step, "new": new_step, "counts": counts_step}[args.step](args)
    if args.reps < 5:
        ap.error("a spread needs at least five repetitions")

    with tempfile.TemporaryDirectory() as tmp:
        work = args.work or tmp
        os.makedirs(work, exist_ok=True)

        def child(step, rep=0, env=None):
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, "--rep", str(rep),
                   "--length", str(args.length), "--pieces", str(args.pieces), "--k", str(args.k), "--device", str(args.device), "--work", work,
                   "--counts-n", str(args.counts_n)]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True)
            if r.returncode != 0:  # nothing more is started on the GPU
                sys.stderr.write(r.stderr[-4000:])
                raise SystemExit(f"step {step} (repetition {rep}) ended with status {r.returncode}")
            line = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")][-1]
            print(json.dumps(line), flush=True)
            return line

        doc = {"tool": "color_split_timing", "length": args.length, "haplotypes": 4, "pieces": args.pieces, "k": args.k, "inputs": child("prepare")}
        if args.parent_library:
            env = dict(os.environ, MATCHTIGS_LIBRARY=os.path.abspath(args.parent_library))
            doc["parent"] = [child("parent", rep, env) for rep in range(args.reps)]
        doc["new"] = [child("new", rep) for rep in range(args.reps)]
        doc["counts"] = [child("counts", rep) for rep in range(args.reps)]

    def spread(values):
        return {"min": min(values), "max": max(values), "max_over_min": round(max(values) / min(values), 4)}

    new, s = doc["new"], {}
    calls = [f"colored_{w}" for w in COLORINGS] + [f"classes_{w}_split{x}" for w in COLORINGS for x in (0, 1)]
    for call in calls:
        for f in ("nodes_ms", "rank_ms", "emit_ms", "download_ms", "total_ms"):
            s[f"{call}_{f}"] = spread([r[call][f] for r in new])
    for call in calls[2:]:
        for f in ("heads_ms", "table_ms", "ids_ms", "counts_ms", "download_ms"):
            s[f"{call}_classes_{f}"] = spread([r[call]["classes_ms"][f] for r in new])
        s[f"{call}_peak_arena_bytes"] = new[0][call]["peak_arena_bytes"]
        s[f"{call}_shape"] = {f: new[0][call][f] for f in ("unitigs", "closed_walks", "longest_unitig_kmers", "classes", "runs", "largest_class_kmers")}
    s["split0_equals_colored"] = all(r[f"classes_{w}_split0"]["equals_colored"] for r in new for w in COLORINGS)
    s["split1_monochromatic"] = all(r[f"classes_{w}_split1"]["monochromatic"] and r[f"classes_{w}_split1"]["statistics_equal_colored"] for r in new for w in COLORINGS)
    for name in ("one_class", "own_class"):
        for f in ("heads_ms", "table_ms", "ids_ms", "counts_ms"):
            s[f"synthetic_{name}_{f}"] = spread([r[name][f] for r in doc["counts"]])
    s["synthetic_one_class_over_own_class_counts"] = round(s["synthetic_one_class_counts_ms"]["min"] / s["synthetic_own_class_counts_ms"]["min"], 4)
    s["aggregation_does_its_job"] = bool(s["synthetic_one_class_over_own_class_counts"] <= 1.0)
    if args.parent_library:
        par = doc["parent"]
        for w in COLORINGS:
            for f in ("nodes_ms", "total_ms"):
                p = s[f"parent_colored_{w}_{f}"] = spread([r[f"colored_{w}"][f] for r in par])
                for call in (f"colored_{w}", f"classes_{w}_split0", f"classes_{w}_split1"):
                    s[f"{call}_{f}_over_parent_colored"] = round(s[f"{call}_{f}"]["min"] / p["min"], 4)
                s[f"colored_{w}_{f}_within_parent_spread"] = bool(s[f"colored_{w}_{f}"]["min"] <= p["max"])
    doc["summary"] = s
    print(json.dumps({"summary": s}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
