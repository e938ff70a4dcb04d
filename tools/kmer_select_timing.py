"""kmer_select_timing.py -- what the k-mer selection costs (api.compact_unitigs_selected, mtg_compact_unitigs_selected) on
DESIGN.md 29's workload: the four haplotypes of G-seq as four colours, k = 31; the SUBTRACT file is haplotype 1 cut into reads of 151
bases that overlap by k - 1.

The parent process starts no GPU work. Every GPU step is a child process under its own `timeout -k 10`; the first that fails ends the run:
  prepare         the haplotypes and the reads, written once as .npy files
  parent <rep>    the PARENT commit's library, built aside and named by --parent-library, loaded with plain ctypes (it lacks the new
                  entry points, which matchtigs_amd._lib insists on): the coloured compaction WITHOUT a selection, called twice
  new <rep>       this library: the same call through the same code (it must queue the kernels it queued before), then the selected
                  call (subtract the reads, A = 1) twice, with filter_ms and select_ms, and KmerIndex.query of the same reads on an
                  index of the same haplotypes, twice: the yardstick of the probe -- both are one table lookup per window
Of each child the SECOND call of everything is reported (the first also pays the arena's first chunks). --reps children of either
library (at least five) give the run-to-run spread [min - max]. Nothing about speed is promised. Written down: the probe's kernel time
per filter window beside the membership query's per window and their ratio (DESIGN.md 29 measured the tally's add at 2.5 x the query),
select_ms, and the kernel phases of the unselected call in both libraries. Checked: every child counts the same; the selected call's
rejections and `selected` add up to its input; and (with --parent-library) the unselected call's best kernel time in this library is at
or below the parent's slowest. A check that fails ends the run with a non-zero status after the JSON is written.

usage: python tools/kmer_select_timing.py --parent-library PATH [--length 100000000] [--k 31] [--reps 5] [--device 0] [--read-length 151]
                                          [--work DIR] [--step-timeout 600] [--out profiles/kmer_select_gseq_1e8.json]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))

from kmer_correct_timing import load  # noqa: E402

PHASES = ("upload_ms", "pack_ms", "insert_ms", "ids_ms", "nodes_ms", "rank_ms", "emit_ms", "download_ms", "total_ms", "rounds", "bytes",
          "peak_arena_bytes")
KERNEL_PHASES = ("insert_ms", "ids_ms", "nodes_ms", "rank_ms", "emit_ms")


def prepare(args) -> None:
    from compact_timing import haplotype_arrays
    from kmer_tally_timing import cut_into_reads

    t0 = time.perf_counter()
    haps, haps_off = haplotype_arrays(args.length, 1, 4)
    reads, reads_off = cut_into_reads(haps[args.length:2 * args.length], np.array([0, args.length], np.uint64), args.read_length, args.k)
    for name, a in (("haps_seq", haps), ("haps_off", haps_off), ("reads_seq", reads), ("reads_off", reads_off)):
        np.save(os.path.join(args.work, name + ".npy"), a)
    windows = int((np.diff(reads_off.astype(np.int64)) - (args.k - 1)).clip(0).sum())
    print(json.dumps({"step": "prepare", "characters": int(haps_off[-1]), "reads": len(reads_off) - 1, "read_characters": int(reads_off[-1]),
                      "filter_windows": windows, "seconds": round(time.perf_counter() - t0, 1)}), flush=True)


def unselected(L, args, out) -> None:
    """The coloured compaction both libraries have, through plain ctypes, twice; the second call's phases."""
    from matchtigs_amd import _lib  # (the structures' layouts only)

    vp, u64, ci = C.c_void_p, C.c_uint64, C.c_int
    L.mtg_compact_unitigs_colored.argtypes = [vp, vp, u64, u64, u64, vp, u64, ci, C.POINTER(vp), vp, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp]
    L.mtg_last_compact_times.argtypes = [C.POINTER(C.c_double)]
    for f in ("mtg_unitigs_free", "mtg_abundance_sums_free", "mtg_kmer_counts_free", "mtg_kmer_colors_free"):
        getattr(L, f).argtypes = [vp]
    seq, off = load(args.work, "haps_seq", "haps_off")
    colors = np.arange(len(off) - 1, dtype=np.uint8)
    t = (C.c_double * 12)()
    for _ in range(2):
        store, sums, counts, masks = vp(), vp(), vp(), vp()
        stats, ab, cs = _lib.MtgCompaction(), _lib.MtgAbundance(), _lib.MtgColorStats()
        t0 = time.perf_counter()
        L.mtg_compact_unitigs_colored(seq.ctypes.data, off.ctypes.data, len(off) - 1, args.k, 1, colors.ctypes.data, len(colors), args.device,
                                      C.byref(store), C.addressof(stats), C.addressof(ab), C.byref(sums), C.byref(counts), C.byref(masks),
                                      C.addressof(cs))
        wall = 1e3 * (time.perf_counter() - t0)
        L.mtg_last_compact_times(t)
        L.mtg_unitigs_free(store), L.mtg_abundance_sums_free(sums), L.mtg_kmer_counts_free(counts), L.mtg_kmer_colors_free(masks)
    out.update({f"unselected_{n}": round(v, 3) for n, v in zip(PHASES[:9], list(t)[:9])})
    out.update({"unselected_kernel_ms": round(sum(t[PHASES.index(n)] for n in KERNEL_PHASES), 3), "unselected_wall_ms": round(wall, 3),
                "unselected_distinct_kmers": int(stats.distinct_kmers), "unselected_unitigs": int(stats.unitigs),
                "unselected_core": int(cs.occupancy[len(colors)])})


def parent_step(args) -> None:
    out = {"step": "parent", "rep": args.rep}
    unselected(C.CDLL(os.environ["MATCHTIGS_LIBRARY"]), args, out)
    print(json.dumps(out), flush=True)


def new_step(args) -> None:
    from matchtigs_amd import _lib, api

    out = {"step": "new", "rep": args.rep}
    unselected(C.CDLL(str(_lib.LIB_PATH)), args, out)
    seq, off, r_seq, r_off = load(args.work, "haps_seq", "haps_off", "reads_seq", "reads_off")
    colors = np.arange(len(off) - 1, dtype=np.uint8)
    for _ in range(2):
        t0 = time.perf_counter()
        store, c, a, col, _, _, _, sel = api.compact_unitigs_selected((seq, off), args.k, api.KmerSelection(subtract=(r_seq, r_off)),
                                                                      record_colors=colors, n_colors=len(colors), device_id=args.device)
        wall = 1e3 * (time.perf_counter() - t0)
        t = api.last_compact_times()
        del store, a, col
    out.update({f"selected_{n}": round(t[n], 3) for n in KERNEL_PHASES + ("filter_ms", "select_ms", "total_ms")})
    out.update({"selected_wall_ms": round(wall, 3), "selected_unitigs": c.unitigs, "input_kmers": sel.input_kmers, "selected": sel.selected,
                "rejected_subtract": sel.rejected_subtract, "subtract_windows": sel.subtract_windows, "subtract_hits": sel.subtract_hits,
                "per_color_selected": sel.per_color_selected.tolist(), "filter_ns_per_window": round(1e6 * t["filter_ms"] / sel.subtract_windows, 4),
                "select_ns_per_kmer": round(1e6 * t["select_ms"] / sel.input_kmers, 4)})
    with api.KmerIndex((seq, off), args.k, args.device) as ix:
        for _ in range(2):
            r = ix.query((r_seq, r_off))
        q = api.last_kmer_query_times()
        out.update({"query_probe_ms": round(q["query_probe_ms"], 3), "query_windows": int(r.kmers.sum()), "query_found": int(r.found.sum()),
                    "query_ns_per_window": round(1e6 * q["query_probe_ms"] / int(r.kmers.sum()), 4)})
    print(json.dumps(out), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=100_000_000)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--read-length", type=int, default=151)
    ap.add_argument("--parent-library", help="libmatchtigs.so of the parent commit, built aside")
    ap.add_argument("--work", help="directory for the prepared inputs (default: a temporary one)")
    ap.add_argument("--step-timeout", type=int, default=600, help="seconds a child may take")
    ap.add_argument("--step", choices=("prepare", "parent", "new"), help=argparse.SUPPRESS)
    ap.add_argument("--rep", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.step:
        return {"prepare": prepare, "parent": parent_step, "new": new_step}[args.step](args)
    if args.reps < 5:
        ap.error("the spread needs at least five repetitions")
    if args.read_length < args.k:
        ap.error("--read-length must be at least k")

    with tempfile.TemporaryDirectory() as tmp:
        work = args.work or tmp
        os.makedirs(work, exist_ok=True)

        def child(step, rep=0, env=None):
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, "--rep", str(rep),
                   "--length", str(args.length), "--k", str(args.k), "--device", str(args.device), "--work", work, "--read-length", str(args.read_length)]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True)
            if r.returncode != 0:  # nothing more is started on the GPU
                sys.stderr.write(r.stderr[-4000:])
                raise SystemExit(f"step {step} (repetition {rep}) ended with status {r.returncode}")
            line = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")][-1]
            print(json.dumps(line), flush=True)
            return line

        doc = {"tool": "kmer_select_timing", "length": args.length, "haplotypes": 4, "k": args.k, "read_length": args.read_length,
               "inputs": child("prepare")}
        if args.parent_library:
            env = dict(os.environ, MATCHTIGS_LIBRARY=os.path.abspath(args.parent_library))
            doc["parent"] = [child("parent", rep, env) for rep in range(args.reps)]
        doc["new"] = [child("new", rep) for rep in range(args.reps)]

    def spread(rows, f):
        v = [r[f] for r in rows]
        return {"min": min(v), "max": max(v)}

    new, yard = doc["new"], doc.get("parent") or doc["new"]
    s = {"yardsticks_from": "parent library" if args.parent_library else "this library (no --parent-library given)"}
    for f in ("unselected_kernel_ms", "unselected_total_ms") + tuple("unselected_" + n for n in KERNEL_PHASES):
        s[f], s["parent_" + f] = spread(new, f), spread(yard, f)
    for f in ("selected_filter_ms", "selected_select_ms", "selected_total_ms", "filter_ns_per_window", "select_ns_per_kmer", "query_probe_ms",
              "query_ns_per_window") + tuple("selected_" + n for n in KERNEL_PHASES):
        s[f] = spread(new, f)
    s["filter_probe_over_query_probe_per_window"] = round(s["filter_ns_per_window"]["min"] / s["query_ns_per_window"]["min"], 4)
    for f in ("input_kmers", "selected", "rejected_subtract", "subtract_windows", "subtract_hits", "selected_unitigs", "per_color_selected"):
        s[f] = new[0][f]
    counts = ("unselected_distinct_kmers", "unselected_unitigs", "unselected_core")
    checks = {"counts_equal_in_every_child": all(r[f] == yard[0][f] for r in new + yard for f in counts)
              and all(r[f] == new[0][f] for r in new for f in ("input_kmers", "selected", "rejected_subtract", "subtract_hits", "query_found")),
              "rejections_add_up": all(r["rejected_subtract"] + r["selected"] == r["input_kmers"] == r["unselected_distinct_kmers"] for r in new),
              "probe_and_query_find_the_same_windows": all(r["subtract_hits"] == r["query_found"] and r["subtract_windows"] == r["query_windows"] for r in new)}
    if args.parent_library:  # the unselected call queues what it queued before: this library's best at or below the parent's slowest
        checks["unselected_kernels_within_parent_spread"] = s["unselected_kernel_ms"]["min"] <= s["parent_unselected_kernel_ms"]["max"]
    s["checks"] = checks
    doc["summary"] = s
    print(json.dumps({"summary": s}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    if not all(checks.values()):
        raise SystemExit("a check failed: " + ", ".join(f for f, v in checks.items() if not v))


if __name__ == "__main__":
    main()
