"""kmer_thread_timing.py -- what threading reads through the unitig graph costs (api.KmerIndex.thread / api.TigIndex.thread,
mtg_kmer_index_thread) beside `locate` on the same reads, on DESIGN.md 29's workload: the four haplotypes of G-seq,
k = 31, indexed as their unitigs; the READS are the haplotypes cut into reads of 151 bases that overlap by k - 1, with seeded uniform
substitution errors at --rate (1 %), so that walks break where the graph lacks a k-mer.

The parent process starts no GPU work. Every GPU step is a child process under its own `timeout -k 10`; the first that fails ends the run:
  prepare         the unitigs (the GPU compaction) and the reads, written once as .npy files
  parent <rep>    the PARENT commit's library, built aside and named by --parent-library, loaded with plain ctypes (it lacks the new
                  entry points, which matchtigs_amd._lib insists on): on a locating table and a locating sparse index over the
                  unitigs the `query` and `locate` calls of the reads, each called twice
  new <rep>       this library: the same calls through the same code (their kernels are not touched: they must stay inside the
                  parent's spread), then `thread` on both indexes, called twice, with its phases, and the GAF text of the table's walks
Of each child the SECOND call of everything is reported (the first also pays the arena's first chunks). --reps children of either
library (at least five) give the run-to-run spread (max / min), and the parent's own spread stands beside every value. Nothing about
speed is promised. Written down: the walk stage beside the probe and the run stage of the same call on both indexes, the whole `thread`
call beside the whole `locate` call by the host clock, the GAF text's time and bytes, and the walks, steps and reads threaded end to end.
Checked: both indexes give the same walks and steps, the same in every child; the walks' k-mers sum to the found windows; and (with
--parent-library) the best query and locate probe of this library's children is at or below the slowest of the parent's. A check that
fails ends the run with a non-zero status after the JSON is written.

usage: python tools/kmer_thread_timing.py --parent-library PATH [--length 100000000] [--k 31] [--reps 5] [--device 0] [--read-length 151]
                                          [--rate 0.01] [--work DIR] [--step-timeout 900] [--out profiles/kmer_thread_gseq_1e8.json]
Without --parent-library the yardsticks are this library's own calls and the JSON says so."""
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

from kmer_correct_timing import digest, load, plant  # noqa: E402

PROBES = ("table_query_ms", "table_locate_ms", "table_runs_ms", "sparse_query_ms", "sparse_locate_ms", "sparse_runs_ms")


def prepare(args) -> None:
    import torch  # noqa: F401  (one HIP runtime for torch and the library)

    from compact_timing import haplotype_arrays
    from kmer_tally_timing import cut_into_reads
    from matchtigs_amd import api

    k, t0 = args.k, time.perf_counter()
    haps, haps_off = haplotype_arrays(args.length, 1, 4)
    store, c = api.compact_unitigs((haps, haps_off), k, args.device)
    reads, reads_off = cut_into_reads(haps, haps_off, args.read_length, k)
    noisy, where, _ = plant(reads, args.rate, 1036)
    seq, off = store.arrays()
    for name, a in (("unitigs_seq", np.asarray(seq)), ("unitigs_off", off.astype(np.uint64)), ("reads_seq", noisy), ("reads_off", reads_off)):
        np.save(os.path.join(args.work, name + ".npy"), a)
    print(json.dumps({"step": "prepare", "distinct_kmers": c.distinct_kmers, "unitigs": len(off) - 1, "unitig_characters": int(off[-1]),
                      "reads": len(reads_off) - 1, "read_characters": int(reads_off[-1]), "planted_errors": len(where),
                      "seconds": round(time.perf_counter() - t0, 1)}), flush=True)


def yardsticks(L, args, out) -> None:
    """The calls both libraries have, through plain ctypes: query and locate on the table and on the sparse index."""
    vp, u64, ci = C.c_void_p, C.c_uint64, C.c_int
    L.mtg_kmer_index_build_locating.restype = L.mtg_tig_index_build_locating.restype = vp
    L.mtg_kmer_index_build_locating.argtypes = [vp, vp, u64, u64, ci]
    L.mtg_tig_index_build_locating.argtypes = [vp, vp, u64, u64, u64, u64, ci]
    L.mtg_kmer_runs_count.restype = u64
    L.mtg_kmer_index_free.argtypes = L.mtg_tig_index_free.argtypes = L.mtg_kmer_runs_count.argtypes = L.mtg_kmer_runs_free.argtypes = [vp]
    L.mtg_kmer_index_query.argtypes = L.mtg_tig_index_query.argtypes = [vp, vp, vp, u64, vp, vp, vp, vp, vp]
    L.mtg_kmer_index_locate.argtypes = L.mtg_tig_index_locate.argtypes = [vp, vp, vp, u64, vp, vp, vp, C.POINTER(vp)]
    for f in ("mtg_last_kmer_query_times", "mtg_last_kmer_locate_times", "mtg_last_tig_index_times", "mtg_last_tig_locate_times"):
        getattr(L, f).argtypes = [C.POINTER(C.c_double)]
    k, dev = args.k, args.device
    r_seq, r_off, u_seq, u_off = load(args.work, "reads_seq", "reads_off", "unitigs_seq", "unitigs_off")
    n_r, n_u = len(r_off) - 1, len(u_off) - 1
    p = lambda a: a.ctypes.data
    kmers, valid, found = (np.zeros(n_r, np.uint64) for _ in range(3))
    t = (C.c_double * 8)()
    for kind, ix, query, query_times, probe_at, locate, locate_times, free in (
            ("table", L.mtg_kmer_index_build_locating(p(u_seq), p(u_off), n_u, k, dev), L.mtg_kmer_index_query, L.mtg_last_kmer_query_times, 5,
             L.mtg_kmer_index_locate, L.mtg_last_kmer_locate_times, L.mtg_kmer_index_free),
            ("sparse", L.mtg_tig_index_build_locating(p(u_seq), p(u_off), n_u, k, 0, 0, dev), L.mtg_tig_index_query, L.mtg_last_tig_index_times, 7,
             L.mtg_tig_index_locate, L.mtg_last_tig_locate_times, L.mtg_tig_index_free)):
        for _ in range(2):  # the second call finds the arena's chunks in place
            query(ix, p(r_seq), p(r_off), n_r, p(kmers), p(valid), p(found), None, None)
            query_times(t)
        out.update({f"{kind}_query_ms": round(t[probe_at], 3), f"{kind}_found": int(found.sum()), f"{kind}_valid": int(valid.sum())})
        for _ in range(2):
            h = vp()
            t0 = time.perf_counter()
            locate(ix, p(r_seq), p(r_off), n_r, p(kmers), p(valid), p(found), C.byref(h))
            wall = 1e3 * (time.perf_counter() - t0)
            locate_times(t)
            runs = int(L.mtg_kmer_runs_count(h))
            L.mtg_kmer_runs_free(h)
        out.update({f"{kind}_locate_ms": round(t[2], 3), f"{kind}_runs_ms": round(t[3], 3), f"{kind}_locate_wall_ms": round(wall, 3),
                    f"{kind}_runs": runs})
        free(ix)


def parent_step(args) -> None:
    out = {"step": "parent", "rep": args.rep}
    yardsticks(C.CDLL(os.environ["MATCHTIGS_LIBRARY"]), args, out)
    print(json.dumps(out), flush=True)


def new_step(args) -> None:
    from matchtigs_amd import _lib, api

    out = {"step": "new", "rep": args.rep}
    yardsticks(C.CDLL(str(_lib.LIB_PATH)), args, out)
    r_seq, r_off, u_seq, u_off = load(args.work, "reads_seq", "reads_off", "unitigs_seq", "unitigs_off")
    n_r = len(r_off) - 1
    names = (np.char.zfill(np.arange(n_r).astype("S10"), 10).view(np.uint8), np.arange(n_r + 1, dtype=np.uint64) * np.uint64(10))
    for kind, make in (("table", lambda: api.KmerIndex((u_seq, u_off), args.k, args.device, locate=True)),
                       ("sparse", lambda: api.TigIndex((u_seq, u_off), args.k, None, args.device, locate=True))):
        with make() as ix:
            for _ in range(2):
                t0 = time.perf_counter()
                r = ix.thread((r_seq, r_off))
                wall = 1e3 * (time.perf_counter() - t0)
            t = api.last_kmer_thread_times(tig=kind == "sparse")
            w = r.walks
            whole = int(np.count_nonzero((np.bincount(w["q_record"].astype(np.int64), minlength=n_r) == 1)
                                         & (np.bincount(w["q_record"].astype(np.int64), weights=w["kmers"].astype(np.float64), minlength=n_r) == r.kmers)))
            out.update({f"{kind}_thread_{f}": round(v, 3) for f, v in t.items()})
            out.update({f"{kind}_thread_wall_ms": round(wall, 3), f"{kind}_walks": len(w), f"{kind}_steps": len(r.steps),
                        f"{kind}_reads_end_to_end": whole, f"{kind}_walk_kmers": int(w["kmers"].sum()),
                        f"{kind}_thread_found": int(r.found.sum()), f"{kind}_longest_walk_steps": int(w["steps"].max()) if len(w) else 0,
                        f"{kind}_thread_digest": digest(w, r.steps, r.kmers, r.valid, r.found)})
            if kind == "table":
                for _ in range(2):
                    t0 = time.perf_counter()
                    text = r.gaf(names)
                    out["gaf_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
                out.update({"gaf_bytes": len(text), "gaf_lines": text.count(b"\n")})
                del text
            r.close()
    print(json.dumps(out), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=100_000_000)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--read-length", type=int, default=151)
    ap.add_argument("--rate", type=float, default=0.01)
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
                   "--length", str(args.length), "--k", str(args.k), "--device", str(args.device), "--work", work, "--rate", str(args.rate),
                   "--read-length", str(args.read_length)]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True)
            if r.returncode != 0:  # nothing more is started on the GPU
                sys.stderr.write(r.stderr[-4000:])
                raise SystemExit(f"step {step} (repetition {rep}) ended with status {r.returncode}")
            line = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")][-1]
            print(json.dumps(line), flush=True)
            return line

        doc = {"tool": "kmer_thread_timing", "length": args.length, "haplotypes": 4, "k": args.k, "read_length": args.read_length,
               "rate": args.rate, "inputs": child("prepare")}
        if args.parent_library:
            env = dict(os.environ, MATCHTIGS_LIBRARY=os.path.abspath(args.parent_library))
            doc["parent"] = [child("parent", rep, env) for rep in range(args.reps)]
        doc["new"] = [child("new", rep) for rep in range(args.reps)]

    def spread(rows, f):
        v = [r[f] for r in rows]
        return {"min": min(v), "max": max(v), "max_over_min": round(max(v) / min(v), 4) if min(v) > 0 else None}

    new, yard = doc["new"], doc.get("parent") or doc["new"]
    s = {"yardsticks_from": "parent library" if args.parent_library else "this library (no --parent-library given)"}
    checks = {}
    for f in PROBES + ("table_locate_wall_ms", "sparse_locate_wall_ms"):
        s[f] = spread(new, f)
        s[f"parent_{f}"] = spread(yard, f)
        s[f"{f}_over_parent"] = round(s[f]["min"] / s[f"parent_{f}"]["min"], 4)
    if args.parent_library:  # untouched kernels: the best of this library's children is no slower than the parent's slowest
        for f in PROBES:
            checks[f"{f}_within_parent_spread"] = s[f]["min"] <= s[f"parent_{f}"]["max"]
    checks["counts_equal_parent"] = all(r[f] == yard[0][f] for r in new + yard for f in (
        "table_found", "table_valid", "table_runs", "sparse_found", "sparse_valid", "sparse_runs"))
    for kind in ("table", "sparse"):
        for f in ("probe_ms", "runs_ms", "walks_ms", "upload_ms", "pack_ms"):
            s[f"{kind}_thread_{f}"] = spread(new, f"{kind}_thread_{f}")
        s[f"{kind}_thread_wall_ms"] = spread(new, f"{kind}_thread_wall_ms")
        s[f"{kind}_walks_over_probe"] = round(s[f"{kind}_thread_walks_ms"]["min"] / s[f"{kind}_thread_probe_ms"]["min"], 4)
        s[f"{kind}_walks_over_runs"] = round(s[f"{kind}_thread_walks_ms"]["min"] / s[f"{kind}_thread_runs_ms"]["min"], 4)
        s[f"{kind}_thread_wall_over_locate_wall"] = round(s[f"{kind}_thread_wall_ms"]["min"] / s[f"{kind}_locate_wall_ms"]["min"], 4)
        for f in ("walks", "steps", "reads_end_to_end", "walk_kmers", "longest_walk_steps"):
            s[f"{kind}_{f}"] = new[0][f"{kind}_{f}"]
        checks[f"{kind}_walk_kmers_equal_found"] = all(r[f"{kind}_walk_kmers"] == r[f"{kind}_thread_found"] == r[f"{kind}_found"] for r in new)
    checks["both_indexes_and_every_child_agree"] = len({r[f"{kind}_thread_digest"] for r in new for kind in ("table", "sparse")}) == 1
    s["gaf_ms"] = spread(new, "gaf_ms")
    s["gaf_bytes"], s["gaf_lines"] = new[0]["gaf_bytes"], new[0]["gaf_lines"]
    checks["one_gaf_line_per_walk"] = all(r["gaf_lines"] == r["table_walks"] for r in new)
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
