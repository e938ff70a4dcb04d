"""kmer_tally_timing.py -- what counting reads on an index costs (`--count-fa`, mtg_kmer_tally_*) beside the probes it is
modelled on, on the input of DESIGN.md 16: the four haplotypes of G-seq (tools/compact_timing.py's arrays), k = 31. The INDEX holds
their unitigs (the GPU compaction's store); the READS that are counted are the four haplotypes themselves.
  add              against mtg_kmer_index_query on the same index and the same reads: the same walk plus the atomics
  coverage(store)  against mtg_kmer_index_abundance of the store on a weighted index of the store (random uint32 weights): the same
                   walk with an 8-byte counter read per found window for a 4-byte weight, and 64-bit outputs

Every GPU step is a child process of its own, under its own `timeout`, and the first one that fails ends the run:
  prepare         the inputs, written once as .npy files into --work (every later child reads the same bytes)
  parent <rep>    the PARENT commit's library, built aside and named by --parent-library, loaded through MATCHTIGS_LIBRARY with plain
                  ctypes (it lacks the new entry points, which matchtigs_amd._lib insists on): both yardsticks, each called twice
  new <rep>       this library: query, add, coverage and abundance, each called twice; the tally's device bytes; whether add's
                  counts equal the query's and the coverage's sums equal the windows added
Of each child the SECOND call of every probe is reported (the first also pays the arena's first chunks). The yardsticks are the
parent's: at least five repetitions of it give their run-to-run spread (max / min), which stands beside each ratio
(best new / best parent). Also: found windows per second of add -- one 8-byte atomic each unless neighbouring windows share a class.

With --read-length L the haplotypes are counted as records of L bases that overlap by k - 1 -- the same windows, but millions of
records instead of four, so that the per-record counters of the walk (valid, found) are not four contended words.

usage: python tools/kmer_tally_timing.py --parent-library PATH [--length 100000000] [--k 31] [--reps 5] [--device 0] [--work DIR]
                                         [--read-length 0] [--step-timeout 600] [--out profiles/kmer_tally_gseq_1e8.json]
Without --parent-library the ratios are taken against this library's own query and abundance and the JSON says so. One JSON line per
child; --out writes all of it."""
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

FILES = ("index_seq", "index_off", "reads_seq", "reads_off", "weights")


def _load(work):
    return {f: np.ascontiguousarray(np.load(os.path.join(work, f + ".npy"))) for f in FILES}


def prepare(args) -> None:
    from compact_timing import haplotype_arrays
    from matchtigs_amd import api

    reads, reads_off = haplotype_arrays(args.length, 1)
    store, c = api.compact_unitigs((reads, reads_off), args.k, args.device)
    if args.read_length:  # the same windows as records of read_length bases that overlap by k - 1
        reads, reads_off = cut_into_reads(reads, reads_off, args.read_length, args.k)
    seq, off = store.arrays()
    off = off.astype(np.uint64)
    windows = int(np.maximum(np.diff(off).astype(np.int64) - (args.k - 1), 0).sum())
    out = {"index_seq": np.asarray(seq), "index_off": off, "reads_seq": reads, "reads_off": reads_off,
           "weights": np.random.default_rng(1).integers(0, 2 ** 32, windows, dtype=np.uint64).astype(np.uint32)}
    for f in FILES:
        np.save(os.path.join(args.work, f + ".npy"), out[f])
    print(json.dumps({"step": "prepare", "index_records": len(off) - 1, "index_characters": int(off[-1]), "index_windows": windows,
                      "distinct_kmers": c.distinct_kmers, "reads_records": len(reads_off) - 1, "reads_characters": int(reads_off[-1])}), flush=True)


def cut_into_reads(data, off, read_length, k):
    """Every record cut into records of read_length bases that start read_length - (k - 1) apart, and a shorter last one: the same
    windows in the same order, so the same k-mers are found and counted."""
    step = read_length - (k - 1)
    pieces, lengths = [np.zeros(0, np.uint8)], [np.zeros(0, np.uint64)]
    for r in range(len(off) - 1):
        rec = data[int(off[r]):int(off[r + 1])]
        n_full = (len(rec) - read_length) // step + 1 if len(rec) >= read_length else 0
        if n_full:
            pieces.append(np.lib.stride_tricks.as_strided(rec, (n_full, read_length), (step, 1)).reshape(-1))
            lengths.append(np.full(n_full, read_length, np.uint64))
        rest = rec[n_full * step:]  # (the full records hold the windows that start before n_full * step)
        if len(rest) >= k:
            pieces.append(rest)
            lengths.append(np.array([len(rest)], np.uint64))
    return np.concatenate(pieces), np.concatenate([[0], np.cumsum(np.concatenate(lengths))]).astype(np.uint64)


def parent_step(args) -> None:
    from matchtigs_amd import _lib  # (the structure's layout only; the library it would load is never asked for)

    L = C.CDLL(os.environ["MATCHTIGS_LIBRARY"])
    vp, u64 = C.c_void_p, C.c_uint64
    L.mtg_kmer_index_build.restype = L.mtg_kmer_index_build_weighted.restype = vp
    L.mtg_kmer_index_build.argtypes = [vp, vp, u64, u64, C.c_int]
    L.mtg_kmer_index_build_weighted.argtypes = [vp, vp, u64, u64, vp, u64, C.c_int, C.c_int]
    L.mtg_kmer_index_get_info.argtypes = [vp, C.POINTER(_lib.MtgKmerIndexInfo)]
    L.mtg_kmer_index_query.argtypes = [vp, vp, vp, u64, vp, vp, vp, vp, vp]
    L.mtg_kmer_index_abundance.argtypes = [vp, vp, vp, u64, vp, vp, vp, vp, vp, vp, vp]
    L.mtg_kmer_index_free.argtypes = [vp]
    L.mtg_last_kmer_query_times.argtypes = L.mtg_last_kmer_abundance_times.argtypes = [C.POINTER(C.c_double)]
    d = _load(args.work)
    n_ix, n_reads = len(d["index_off"]) - 1, len(d["reads_off"]) - 1
    out = {"step": "parent", "rep": args.rep}
    ix = L.mtg_kmer_index_build(d["index_seq"].ctypes.data, d["index_off"].ctypes.data, n_ix, args.k, args.device)
    info = _lib.MtgKmerIndexInfo()
    L.mtg_kmer_index_get_info(ix, C.byref(info))
    kmers, valid, found = (np.zeros(n_reads, np.uint64) for _ in range(3))
    for _ in range(2):  # the second call finds the arena's chunks in place
        L.mtg_kmer_index_query(ix, d["reads_seq"].ctypes.data, d["reads_off"].ctypes.data, n_reads, kmers.ctypes.data, valid.ctypes.data,
                               found.ctypes.data, None, None)
        t = (C.c_double * 6)()
        L.mtg_last_kmer_query_times(t)
    L.mtg_kmer_index_free(ix)
    out.update(query_probe_ms=round(t[5], 3), index_slots=int(info.slots), windows=int(kmers.sum()), valid=int(valid.sum()), found=int(found.sum()))
    ix = L.mtg_kmer_index_build_weighted(d["index_seq"].ctypes.data, d["index_off"].ctypes.data, n_ix, args.k, d["weights"].ctypes.data,
                                         len(d["weights"]), 0, args.device)
    kmers, valid, found, total = (np.zeros(n_ix, np.uint64) for _ in range(4))
    lo, hi = np.zeros(n_ix, np.uint32), np.zeros(n_ix, np.uint32)
    for _ in range(2):
        L.mtg_kmer_index_abundance(ix, d["index_seq"].ctypes.data, d["index_off"].ctypes.data, n_ix, kmers.ctypes.data, valid.ctypes.data,
                                   found.ctypes.data, total.ctypes.data, lo.ctypes.data, hi.ctypes.data, None)
        t = (C.c_double * 4)()
        L.mtg_last_kmer_abundance_times(t)
    L.mtg_kmer_index_free(ix)
    out.update(abundance_probe_ms=round(t[2], 3), abundance_download_ms=round(t[3], 3), store_found=int(found.sum()))
    print(json.dumps(out), flush=True)


def new_step(args) -> None:
    from matchtigs_amd import api

    d = _load(args.work)
    index, reads = (d["index_seq"], d["index_off"]), (d["reads_seq"], d["reads_off"])
    out = {"step": "new", "rep": args.rep}
    with api.KmerIndex(index, args.k, args.device) as ix, api.KmerTally(ix) as tally:
        out.update(index_slots=ix.info.slots, index_device_bytes=ix.info.device_bytes, tally_device_bytes=tally.device_bytes)
        for _ in range(2):  # the second call finds the arena's chunks in place
            q = ix.query(reads)
        out["query_probe_ms"] = round(api.last_kmer_query_times()["query_probe_ms"], 3)
        for _ in range(2):
            tally.reset()
            t0 = time.perf_counter()
            a = tally.add(reads)
            out["add_wall_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
        t = api.last_kmer_tally_times()
        out.update(add_probe_ms=round(t["probe_ms"], 3), add_upload_ms=round(t["upload_ms"], 3), add_pack_ms=round(t["pack_ms"], 3))
        for _ in range(2):
            t0 = time.perf_counter()
            cov = tally.coverage(index)
            out["coverage_wall_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
        t = api.last_kmer_tally_times()
        out.update(coverage_probe_ms=round(t["probe_ms"], 3), coverage_download_ms=round(t["download_ms"], 3))
        found = int(a.found.sum())
        out.update(windows=int(a.kmers.sum()), valid=int(a.valid.sum()), found=found, store_found=int(cov.found.sum()),
                   add_counts_equal_query=bool(np.array_equal(a.found, q.found) and np.array_equal(a.valid, q.valid)),
                   store_all_found=bool(np.array_equal(cov.found, cov.kmers)), store_covered=int(cov.covered.sum()),
                   coverage_sum=int(cov.sum.sum()), coverage_max=int(cov.max.max()),
                   add_found_per_s=round(found / (1e-3 * out["add_probe_ms"]), 1))
    with api.KmerIndex(index, args.k, args.device, weights=d["weights"]) as ix:
        for _ in range(2):
            ab = ix.abundance(index)
        t = api.last_kmer_abundance_times()
        out.update(abundance_probe_ms=round(t["probe_ms"], 3), abundance_download_ms=round(t["download_ms"], 3),
                   abundance_counts_equal_coverage=bool(np.array_equal(ab.found, cov.found)))
    print(json.dumps(out), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=100_000_000)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--read-length", type=int, default=0,
                    help="count the haplotypes cut into records of this many bases that overlap by k - 1 (0: the four haplotypes whole)")
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
    if args.read_length and args.read_length < args.k:
        ap.error("--read-length must be at least k")

    with tempfile.TemporaryDirectory() as tmp:
        work = args.work or tmp
        os.makedirs(work, exist_ok=True)

        def child(step, rep=0, env=None):
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, "--rep", str(rep),
                   "--length", str(args.length), "--k", str(args.k), "--device", str(args.device), "--work", work,
                   "--read-length", str(args.read_length)]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True)
            if r.returncode != 0:  # nothing more is started on the GPU
                sys.stderr.write(r.stderr[-4000:])
                raise SystemExit(f"step {step} (repetition {rep}) ended with status {r.returncode}")
            line = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")][-1]
            print(json.dumps(line), flush=True)
            return line

        doc = {"tool": "kmer_tally_timing", "length": args.length, "haplotypes": 4, "k": args.k, "read_length": args.read_length,
               "inputs": child("prepare")}
        if args.parent_library:
            env = dict(os.environ, MATCHTIGS_LIBRARY=os.path.abspath(args.parent_library))
            doc["parent"] = [child("parent", rep, env) for rep in range(args.reps)]
        doc["new"] = [child("new", rep) for rep in range(args.reps)]

    def spread(rows, f):
        v = [r[f] for r in rows]
        return {"min": min(v), "max": max(v), "max_over_min": round(max(v) / min(v), 4)}

    new, yard = doc["new"], doc.get("parent") or doc["new"]
    s = {"yardsticks_from": "parent library" if args.parent_library else "this library (no --parent-library given)",
         "tally_device_bytes": new[0]["tally_device_bytes"], "index_device_bytes": new[0]["index_device_bytes"],
         "found": new[0]["found"], "windows": new[0]["windows"]}
    for f in ("query_probe_ms", "add_probe_ms", "coverage_probe_ms", "abundance_probe_ms", "add_found_per_s"):
        s[f] = spread(new, f)
    for f in ("query_probe_ms", "abundance_probe_ms"):
        s["yardstick_" + f] = spread(yard, f)
    s["add_over_query"] = round(s["add_probe_ms"]["min"] / s["yardstick_query_probe_ms"]["min"], 4)
    s["coverage_over_abundance"] = round(s["coverage_probe_ms"]["min"] / s["yardstick_abundance_probe_ms"]["min"], 4)
    s["query_over_yardstick_query"] = round(s["query_probe_ms"]["min"] / s["yardstick_query_probe_ms"]["min"], 4)
    s["checks"] = {f: all(r[f] for r in new) for f in ("add_counts_equal_query", "store_all_found", "abundance_counts_equal_coverage")}
    s["checks"]["coverage_sum_equals_found"] = all(r["coverage_sum"] == r["found"] for r in new)
    s["checks"]["counts_equal_yardstick"] = all(new[0][f] == yard[0][f] for f in ("windows", "valid", "found", "store_found"))
    doc["summary"] = s
    print(json.dumps({"summary": s}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
