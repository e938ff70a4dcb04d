"""pseudoalign_timing.py -- what pseudoalignment with equivalence classes costs (api.Pseudoaligner, mtg_pseudoaligner_*)
beside the parent's way to the same masks, on DESIGN.md 29's workload: the four haplotypes of G-seq as four colours, k = 31, indexed
as their unitigs with one mask per k-mer (the coloured compaction's); the SAMPLE is the haplotypes cut into reads of 151 bases that
overlap by k - 1, aligned single-end (every read a fragment) and paired (read r of the first half with read r of the second half).

The parent process starts no GPU work. Every GPU step is a child process under its own `timeout -k 10`; the first that fails ends the run:
  prepare         the unitigs and their masks (the coloured GPU compaction) and the reads, written once as .npy files into --work
  parent <rep>    the PARENT commit's library, built aside and named by --parent-library, loaded with plain ctypes (it lacks the new
                  entry points, which matchtigs_amd._lib insists on): on the coloured table and on the annotated sparse index over the
                  unitigs the query, locate and colour probes, each called twice, and the BASELINE -- mtg_*_index_colors on the reads,
                  its counters downloaded, and the rule at threshold 1000 over found in numpy on the host
  new <rep>       this library: the same calls through the same code (their kernels are not touched: they must stay inside the
                  parent's spread), then Pseudoaligner.align single-end and paired on both indexes, each called twice, with its phases
Of each child the SECOND call of everything is reported (the first also pays the arena's first chunks). --reps children of either
library (at least five) give the run-to-run spread (max / min), and the parent's own spread stands beside every ratio (best new /
best parent). No ratio is promised. Checked: the aligner's masks equal the baseline's on both indexes, both indexes give the same
masks, classes and totals, the classes' fragments sum to `assigned`, the paired masks equal the rule applied to the summed counters of
the two halves, every child reports the same digests, and (with --parent-library) the best query, locate and colour probe of this
library's children is at or below the slowest of the parent's. A check that fails ends the run with a non-zero status after the JSON
is written.

usage: python tools/pseudoalign_timing.py --parent-library PATH [--length 100000000] [--k 31] [--m 19] [--reps 5] [--device 0]
                                          [--read-length 151] [--work DIR] [--step-timeout 900] [--out profiles/pseudoalign_gseq_1e8.json]
Without --parent-library the yardsticks are this library's own calls and the JSON says so."""
import argparse
import ctypes as C
import hashlib
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
KINDS = ("table", "sparse")
PROBES = ("query_ms", "locate_ms", "colors_ms")


def load(work, *names):
    return [np.ascontiguousarray(np.load(os.path.join(work, n + ".npy"))) for n in names]


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def halves(seq, off):
    """The reads as pairs: (first half, second half) with as many records each (an odd last read is left out)."""
    n = (len(off) - 1) // 2
    cut, end = int(off[n]), int(off[2 * n])
    return (seq[:cut], off[:n + 1].copy()), (np.ascontiguousarray(seq[cut:end]), (off[n:2 * n + 1] - off[n]).astype(np.uint64))


def rule(per_color, found):
    """Threshold 1000 over found, min_kmers 1, in numpy: the parent's way from the downloaded counters to the masks."""
    hits = per_color.astype(np.uint64)
    on = (hits > 0) & (hits == found[:, None])
    return (on.astype(np.uint64) << np.arange(per_color.shape[1], dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint64)


def prepare(args) -> None:
    import torch  # noqa: F401  (one HIP runtime for torch and the library)

    from compact_timing import haplotype_arrays
    from kmer_tally_timing import cut_into_reads
    from matchtigs_amd import api

    k, t0 = args.k, time.perf_counter()
    haps, haps_off = haplotype_arrays(args.length, 1, N_COLORS)
    store, c, _, colors = api.compact_unitigs_colored((haps, haps_off), k, list(range(N_COLORS)), N_COLORS, 1, args.device)
    reads, reads_off = cut_into_reads(haps, haps_off, args.read_length, k)
    seq, off = store.arrays()
    out = {"unitigs_seq": np.asarray(seq), "unitigs_off": off.astype(np.uint64), "unitigs_masks": np.asarray(colors.kmer_colors, np.uint64),
           "reads_seq": reads, "reads_off": reads_off}
    for name, a in out.items():
        np.save(os.path.join(args.work, name + ".npy"), a)
    print(json.dumps({"step": "prepare", "distinct_kmers": c.distinct_kmers, "unitigs": len(off) - 1, "unitig_characters": int(off[-1]),
                      "unitig_windows": len(out["unitigs_masks"]), "reads": len(reads_off) - 1, "read_characters": int(reads_off[-1]),
                      "pairs": (len(reads_off) - 1) // 2, "seconds": round(time.perf_counter() - t0, 1)}), flush=True)


def yardsticks(L, args, out):
    """The probes both libraries have, through plain ctypes, and the baseline. Returns the baseline's masks per kind."""
    from matchtigs_amd import _lib  # (the structures' layouts only)

    vp, u64, ci = C.c_void_p, C.c_uint64, C.c_int
    L.mtg_kmer_index_build_annotated.restype = L.mtg_tig_index_build_annotated.restype = vp
    L.mtg_kmer_index_build_annotated.argtypes = [vp, vp, u64, u64, vp, u64, vp, u64, u64, ci, ci]
    L.mtg_tig_index_build_annotated.argtypes = [vp, vp, u64, u64, u64, u64, vp, u64, vp, u64, u64, ci, ci]
    L.mtg_kmer_index_get_info.argtypes = [vp, C.POINTER(_lib.MtgKmerIndexInfo)]
    L.mtg_tig_index_get_info.argtypes = [vp, C.POINTER(_lib.MtgTigIndexInfo)]
    L.mtg_kmer_runs_count.restype = u64
    L.mtg_kmer_index_free.argtypes = L.mtg_tig_index_free.argtypes = L.mtg_kmer_runs_count.argtypes = L.mtg_kmer_runs_free.argtypes = [vp]
    for kind in ("kmer", "tig"):
        getattr(L, f"mtg_{kind}_index_query").argtypes = [vp, vp, vp, u64, vp, vp, vp, vp, vp]
        getattr(L, f"mtg_{kind}_index_locate").argtypes = [vp, vp, vp, u64, vp, vp, vp, C.POINTER(vp)]
        getattr(L, f"mtg_{kind}_index_colors").argtypes = [vp, vp, vp, u64, vp, vp, vp, vp, vp]
    for f in ("mtg_last_kmer_query_times", "mtg_last_kmer_locate_times", "mtg_last_kmer_color_times", "mtg_last_tig_index_times",
              "mtg_last_tig_locate_times", "mtg_last_tig_payload_times"):
        getattr(L, f).argtypes = [C.POINTER(C.c_double)]
    k, dev = args.k, args.device
    r_seq, r_off, u_seq, u_off, masks = load(args.work, "reads_seq", "reads_off", "unitigs_seq", "unitigs_off", "unitigs_masks")
    n_r, n_u = len(r_off) - 1, len(u_off) - 1
    p = lambda a: a.ctypes.data
    kmers, valid, found = (np.zeros(n_r, np.uint64) for _ in range(3))
    per_color = np.zeros((n_r, N_COLORS), np.uint32)
    baseline = {}
    for kind in KINDS:
        name = "kmer" if kind == "table" else "tig"
        if kind == "table":
            ix = L.mtg_kmer_index_build_annotated(p(u_seq), p(u_off), n_u, k, None, 0, p(masks), len(masks), N_COLORS, 1, dev)
            info = _lib.MtgKmerIndexInfo()
            L.mtg_kmer_index_get_info(ix, C.byref(info))
        else:
            ix = L.mtg_tig_index_build_annotated(p(u_seq), p(u_off), n_u, k, args.m or 0, 0, None, 0, p(masks), len(masks), N_COLORS, 0, dev)
            info = _lib.MtgTigIndexInfo()
            L.mtg_tig_index_get_info(ix, C.byref(info))
        out[f"{kind}_index_bytes"] = int(info.device_bytes)
        t = (C.c_double * 12)()
        for _ in range(2):  # the second call finds the arena's chunks in place
            getattr(L, f"mtg_{name}_index_query")(ix, p(r_seq), p(r_off), n_r, p(kmers), p(valid), p(found), None, None)
            (L.mtg_last_kmer_query_times if kind == "table" else L.mtg_last_tig_index_times)(t)
        out[f"{kind}_query_ms"] = round(t[5] if kind == "table" else t[7], 3)
        for _ in range(2):
            h = vp()
            getattr(L, f"mtg_{name}_index_locate")(ix, p(r_seq), p(r_off), n_r, p(kmers), p(valid), p(found), C.byref(h))
            (L.mtg_last_kmer_locate_times if kind == "table" else L.mtg_last_tig_locate_times)(t)
            runs = int(L.mtg_kmer_runs_count(h))
            L.mtg_kmer_runs_free(h)
        out.update({f"{kind}_locate_ms": round(t[2], 3), f"{kind}_runs": runs})
        for _ in range(2):
            t0 = time.perf_counter()
            getattr(L, f"mtg_{name}_index_colors")(ix, p(r_seq), p(r_off), n_r, p(kmers), p(valid), p(found), p(per_color), None)
            call = 1e3 * (time.perf_counter() - t0)
            t1 = time.perf_counter()
            baseline[kind] = rule(per_color, found)
            host = 1e3 * (time.perf_counter() - t1)
            (L.mtg_last_kmer_color_times if kind == "table" else L.mtg_last_tig_payload_times)(t)
        # (table: {stats, upload, pack, probe, download}; sparse: [8..11] = {upload, pack, probe, gather})
        out.update({f"{kind}_colors_ms": round(t[3] if kind == "table" else t[10] + t[11], 3), f"{kind}_baseline_call_ms": round(call, 3),
                    f"{kind}_baseline_rule_ms": round(host, 3), f"{kind}_baseline_ms": round(call + host, 3),
                    f"{kind}_found": int(found.sum()), f"{kind}_baseline_digest": digest(baseline[kind], kmers, valid, found),
                    f"{kind}_counters_digest": digest(per_color)})
        (L.mtg_kmer_index_free if kind == "table" else L.mtg_tig_index_free)(ix)
    if not np.array_equal(baseline["table"], baseline["sparse"]):
        raise SystemExit("the two indexes' baselines differ")
    return baseline["table"]


def parent_step(args) -> None:
    out = {"step": "parent", "rep": args.rep}
    yardsticks(C.CDLL(os.environ["MATCHTIGS_LIBRARY"]), args, out)
    print(json.dumps(out), flush=True)


def new_step(args) -> None:
    from matchtigs_amd import _lib, api

    out = {"step": "new", "rep": args.rep}
    base = yardsticks(C.CDLL(str(_lib.LIB_PATH)), args, out)
    k, dev = args.k, args.device
    r_seq, r_off, u_seq, u_off, masks = load(args.work, "reads_seq", "reads_off", "unitigs_seq", "unitigs_off", "unitigs_masks")
    reads, unitigs = (r_seq, r_off), (u_seq, u_off)
    first, second = halves(r_seq, r_off)
    n = len(first[1]) - 1
    state = {}
    for kind in KINDS:
        make = (lambda: api.KmerIndex(unitigs, k, dev, locate=True, colors=masks, n_colors=N_COLORS)) if kind == "table" else (
            lambda: api.TigIndex.annotated(unitigs, k, args.m, dev, colors=masks, n_colors=N_COLORS))
        with make() as ix, api.Pseudoaligner(ix) as a:
            for _ in range(2):
                a.reset()
                t0 = time.perf_counter()
                r = a.align(reads)
                wall = 1e3 * (time.perf_counter() - t0)
            t, cl = api.last_pseudoalign_times(), a.classes()
            out.update({f"{kind}_single_{f}": round(v, 3) for f, v in t.items()})
            out.update({f"{kind}_single_wall_ms": round(wall, 3), f"{kind}_single_kernels_ms": round(t["probe_ms"] + t["mask_ms"] + t["dictionary_ms"], 3),
                        f"{kind}_single_equals_baseline": bool(np.array_equal(r.masks, base)),
                        f"{kind}_single_digest": digest(r.masks, r.kmers, r.valid, r.found), f"{kind}_single_classes": len(cl["mask"]),
                        f"{kind}_single_totals": a.totals, f"{kind}_single_class_sum_ok": int(cl["fragments"].sum()) == a.totals["assigned"]})
            state[kind, "single"] = (cl, a.totals)
            for _ in range(2):
                a.reset()
                t0 = time.perf_counter()
                r = a.align(first, second)
                wall = 1e3 * (time.perf_counter() - t0)
            t, cl = api.last_pseudoalign_times(), a.classes()
            # the same masks the parent's way: two colour calls, the counters summed on the host, the rule in numpy
            c1, c2 = ix.color_hits(first), ix.color_hits(second)
            want = rule(c1.per_color + c2.per_color, c1.found + c2.found)
            out.update({f"{kind}_paired_{f}": round(v, 3) for f, v in t.items()})
            out.update({f"{kind}_paired_wall_ms": round(wall, 3), f"{kind}_paired_kernels_ms": round(t["probe_ms"] + t["mask_ms"] + t["dictionary_ms"], 3),
                        f"{kind}_paired_equals_baseline": bool(np.array_equal(r.masks, want) and len(r.masks) == n),
                        f"{kind}_paired_digest": digest(r.masks, r.kmers, r.valid, r.found), f"{kind}_paired_classes": len(cl["mask"]),
                        f"{kind}_paired_totals": a.totals, f"{kind}_paired_class_sum_ok": int(cl["fragments"].sum()) == a.totals["assigned"]})
            state[kind, "paired"] = (cl, a.totals)
    for mode in ("single", "paired"):
        (ca, ta), (cb, tb) = state["table", mode], state["sparse", mode]
        out[f"{mode}_indexes_agree"] = bool(ta == tb and all(np.array_equal(ca[f], cb[f]) for f in ca))
    print(json.dumps(out), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=100_000_000)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--m", type=int, default=None, help="minimizer length (default: the library's, 19 at k = 31)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--read-length", type=int, default=151)
    ap.add_argument("--parent-library", help="libmatchtigs.so of the parent commit, built aside")
    ap.add_argument("--work", help="directory for the prepared inputs (default: a temporary one)")
    ap.add_argument("--step-timeout", type=int, default=900, help="seconds a child may take")
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
                   "--length", str(args.length), "--k", str(args.k), "--device", str(args.device), "--work", work,
                   "--read-length", str(args.read_length)] + (["--m", str(args.m)] if args.m else [])
            r = subprocess.run(cmd, env=env, capture_output=True, text=True)
            if r.returncode != 0:  # nothing more is started on the GPU
                sys.stderr.write(r.stderr[-4000:])
                raise SystemExit(f"step {step} (repetition {rep}) ended with status {r.returncode}")
            line = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")][-1]
            print(json.dumps(line), flush=True)
            return line

        doc = {"tool": "pseudoalign_timing", "length": args.length, "haplotypes": N_COLORS, "k": args.k, "read_length": args.read_length,
               "rule": {"threshold_permille": 1000, "over": "found", "min_kmers": 1}, "inputs": child("prepare")}
        if args.parent_library:
            env = dict(os.environ, MATCHTIGS_LIBRARY=os.path.abspath(args.parent_library))
            doc["parent"] = [child("parent", rep, env) for rep in range(args.reps)]
        doc["new"] = [child("new", rep) for rep in range(args.reps)]

    def spread(rows, f):
        v = [r[f] for r in rows]
        return {"min": min(v), "max": max(v), "max_over_min": round(max(v) / min(v), 4)}

    new, yard = doc["new"], doc.get("parent") or doc["new"]
    s = {"yardsticks_from": "parent library" if args.parent_library else "this library (no --parent-library given)"}
    checks = {}
    for kind in KINDS:
        for f in PROBES + ("baseline_ms", "baseline_call_ms", "baseline_rule_ms"):
            s[f"{kind}_{f}"] = spread(new, f"{kind}_{f}")
            s[f"yardstick_{kind}_{f}"] = spread(yard, f"{kind}_{f}")
            s[f"{kind}_{f}_over_yardstick"] = round(s[f"{kind}_{f}"]["min"] / s[f"yardstick_{kind}_{f}"]["min"], 4)
        for mode in ("single", "paired"):
            for f in ("wall_ms", "kernels_ms", "upload_ms", "pack_ms", "probe_ms", "mask_ms", "dictionary_ms", "download_ms"):
                s[f"{kind}_{mode}_{f}"] = spread(new, f"{kind}_{mode}_{f}")
            s[f"{kind}_{mode}_classes"] = new[0][f"{kind}_{mode}_classes"]
            s[f"{kind}_{mode}_totals"] = new[0][f"{kind}_{mode}_totals"]
            checks[f"{kind}_{mode}_equals_baseline"] = all(r[f"{kind}_{mode}_equals_baseline"] and r[f"{kind}_{mode}_class_sum_ok"] for r in new)
            checks[f"{kind}_{mode}_same_in_every_child"] = len({r[f"{kind}_{mode}_digest"] for r in new}) == 1
        # the aligner's whole call against the parent's whole way to the same masks (host clock both), and kernels against kernels
        s[f"{kind}_single_wall_over_baseline"] = round(s[f"{kind}_single_wall_ms"]["min"] / s[f"yardstick_{kind}_baseline_ms"]["min"], 4)
        s[f"{kind}_single_kernels_over_colors_probe"] = round(s[f"{kind}_single_kernels_ms"]["min"] / s[f"yardstick_{kind}_colors_ms"]["min"], 4)
        if args.parent_library:  # untouched kernels: the best of this library's children is no slower than the parent's slowest
            for f in PROBES:
                checks[f"{kind}_{f}_within_parent_spread"] = s[f"{kind}_{f}"]["min"] <= s[f"yardstick_{kind}_{f}"]["max"]
        checks[f"{kind}_counts_equal_yardstick"] = all(r[f] == yard[0][f] for r in new + yard for f in (
            f"{kind}_found", f"{kind}_runs", f"{kind}_baseline_digest", f"{kind}_counters_digest"))
    for mode in ("single", "paired"):
        checks[f"{mode}_indexes_agree"] = all(r[f"{mode}_indexes_agree"] for r in new)
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
