"""kmer_abundance_timing.py -- what the abundance query (`--query-abundance-out`, mtg_kmer_index_abundance) costs beside
the membership query, on G-seq: the unitigs are indexed; the query is the unitigs plus an equal volume of the same
unitigs with 3 % substitutions and an `N` every ~10^3 bases (the query set of kmer_query_timing.py). The weights are random uint32.

Every GPU step is a child process of its own, under its own `timeout`, and the first one that fails ends the run:
  prepare         the inputs, written once as .npy files into --work (every later child reads the same bytes)
  parent <rep>    the PARENT commit's library, built aside and named by --parent-library, loaded through MATCHTIGS_LIBRARY with plain
                  ctypes (it lacks the new entry points, which matchtigs_amd._lib insists on): a plain index, `query` without bit arrays
  new <rep>       this library: build ms and device bytes of a plain, a locating and a weighted index; probe ms of `query` on the
                  plain and on the weighted index and of `abundance` without and with per_window on the weighted one; the ratio
                  abundance / query; whether the counts of the three calls agree
The yardstick for "query did not get slower" is the parent's library on the same input: at least five repetitions of it give its
run-to-run spread (min, max, max / min of the probe after the first repetition, which also pays the arena's first chunks), and the
JSON says whether the new library's best query probe lies inside [min, max] of the parent's.

usage: python tools/kmer_abundance_timing.py [--parent-library PATH] [--length 100000000] [--k 31] [--reps 3] [--parent-reps 5]
                                             [--device 0] [--work DIR] [--step-timeout 600] [--out profiles/kmer_abundance_gseq_1e8.json]
Without --parent-library the parent's figures and the verdict are left out. One JSON line per child; --out writes all of it."""
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

FILES = ("index_seq", "index_off", "query_seq", "query_off", "weights")


def _load(work):
    return {f: np.load(os.path.join(work, f + ".npy"), mmap_mode="r") for f in FILES}


def prepare(args) -> None:
    import torch

    from matchtigs_amd import synth

    if torch.cuda.is_available():
        ua = synth.g_seq_arrays_torch(args.length, seed=1, k=31, device=f"cuda:{args.device}")
    else:  # (a rehearsal at a small length)
        ua = synth.g_seq_arrays(args.length, seed=1, k=31)
    rng = np.random.default_rng(1)
    n = len(ua.seq)
    noisy = ua.seq.copy()
    sub = rng.random(n) < 0.03
    noisy[sub] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(sub.sum()))]
    noisy[rng.random(n) < 1e-3] = ord("N")
    off = ua.off.astype(np.uint64)
    windows = int(np.maximum(np.diff(off).astype(np.int64) - (args.k - 1), 0).sum())
    out = {"index_seq": ua.seq, "index_off": off, "query_seq": np.concatenate([ua.seq, noisy]),
           "query_off": np.concatenate([off, off[1:] + off[-1]]).astype(np.uint64),
           "weights": rng.integers(0, 2 ** 32, windows, dtype=np.uint64).astype(np.uint32)}
    for f in FILES:
        np.save(os.path.join(args.work, f + ".npy"), out[f])
    print(json.dumps({"step": "prepare", "index_records": len(off) - 1, "index_characters": int(off[-1]), "index_windows": windows,
                      "query_records": len(out["query_off"]) - 1, "query_characters": int(out["query_off"][-1])}), flush=True)


def parent_step(args) -> None:
    from matchtigs_amd import _lib  # (the structure's layout only; the library it would load is never asked for)

    L = C.CDLL(os.environ["MATCHTIGS_LIBRARY"])
    vp, u64 = C.c_void_p, C.c_uint64
    L.mtg_kmer_index_build.restype = vp
    L.mtg_kmer_index_build.argtypes = [vp, vp, u64, u64, C.c_int]
    L.mtg_kmer_index_get_info.argtypes = [vp, C.POINTER(_lib.MtgKmerIndexInfo)]
    L.mtg_kmer_index_query.argtypes = [vp, vp, vp, u64, vp, vp, vp, vp, vp]
    L.mtg_kmer_index_free.argtypes = [vp]
    L.mtg_last_kmer_query_times.argtypes = [C.POINTER(C.c_double)]
    d = {f: np.ascontiguousarray(a) for f, a in _load(args.work).items()}
    n_q = len(d["query_off"]) - 1
    t0 = time.perf_counter()
    ix = L.mtg_kmer_index_build(d["index_seq"].ctypes.data, d["index_off"].ctypes.data, len(d["index_off"]) - 1, args.k, args.device)
    build_wall = time.perf_counter() - t0
    info = _lib.MtgKmerIndexInfo()
    L.mtg_kmer_index_get_info(ix, C.byref(info))
    kmers, valid, found = (np.zeros(n_q, np.uint64) for _ in range(3))
    probes = []
    for _ in range(2):  # the second call finds the arena's chunks in place
        L.mtg_kmer_index_query(ix, d["query_seq"].ctypes.data, d["query_off"].ctypes.data, n_q, kmers.ctypes.data, valid.ctypes.data,
                               found.ctypes.data, None, None)
        t = (C.c_double * 6)()
        L.mtg_last_kmer_query_times(t)
        probes.append(round(t[5], 3))
    L.mtg_kmer_index_free(ix)
    print(json.dumps({"step": "parent", "rep": args.rep, "plain_build_wall_ms": round(1e3 * build_wall, 3), "plain_build_insert_ms": round(t[2], 3),
                      "plain_device_bytes": int(info.device_bytes), "query_probe_ms_first": probes[0], "query_probe_ms": probes[1],
                      "windows": int(kmers.sum()), "valid": int(valid.sum()), "found": int(found.sum())}), flush=True)


def new_step(args) -> None:
    from matchtigs_amd import api

    d = _load(args.work)
    index, query = (d["index_seq"], d["index_off"]), (d["query_seq"], d["query_off"])
    out = {"step": "new", "rep": args.rep}

    def build(kind, **kw):
        t0 = time.perf_counter()
        ix = api.KmerIndex(index, args.k, args.device, **kw)
        out[f"{kind}_build_wall_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
        tb = api.last_kmer_query_times()
        out[f"{kind}_build_ms"] = round(tb["build_upload_ms"] + tb["build_pack_ms"] + tb["build_insert_ms"], 3)
        out[f"{kind}_build_insert_ms"] = round(tb["build_insert_ms"], 3)
        out[f"{kind}_device_bytes"] = ix.info.device_bytes
        return ix

    def probe_of_query(ix):
        first = None
        for _ in range(2):  # the second call finds the arena's chunks in place
            r = ix.query(query)
            first = api.last_kmer_query_times()["query_probe_ms"] if first is None else first
        return r, round(first, 3), round(api.last_kmer_query_times()["query_probe_ms"], 3)

    with build("plain") as ix:
        r, out["query_probe_ms_first"], out["query_probe_ms"] = probe_of_query(ix)
    build("locating", locate=True).close()
    with build("weighted", weights=d["weights"]) as ix:
        rw, _, out["weighted_query_probe_ms"] = probe_of_query(ix)
        for name, per_window in (("abundance", False), ("abundance_per_window", True)):
            for _ in range(2):
                t0 = time.perf_counter()
                ab = ix.abundance(query, per_window=per_window)
                out[f"{name}_wall_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
            t = api.last_kmer_abundance_times()
            out[f"{name}_probe_ms"], out[f"{name}_download_ms"] = round(t["probe_ms"], 3), round(t["download_ms"], 3)
            out[f"{name}_counts_equal_query"] = bool(np.array_equal(ab.found, r.found) and np.array_equal(ab.valid, r.valid)
                                                     and np.array_equal(rw.found, r.found))
        out["per_window_nonzero_at_most_found"] = int(np.count_nonzero(ab.per_window)) <= int(r.found.sum())
    windows = int(r.kmers.sum())
    out.update({"windows": windows, "valid": int(r.valid.sum()), "found": int(r.found.sum()),
                "query_probe_ns_per_window": round(1e6 * out["query_probe_ms"] / windows, 4),
                "abundance_probe_ns_per_window": round(1e6 * out["abundance_probe_ms"] / windows, 4),
                "abundance_over_query": round(out["abundance_probe_ms"] / out["weighted_query_probe_ms"], 3),
                "abundance_per_window_over_query": round(out["abundance_per_window_probe_ms"] / out["weighted_query_probe_ms"], 3)})
    print(json.dumps(out), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=100_000_000)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--parent-library", help="libmatchtigs.so of the parent commit, built aside")
    ap.add_argument("--work", help="directory for the prepared inputs (default: a temporary one)")
    ap.add_argument("--step-timeout", type=int, default=600, help="seconds a child may take")
    ap.add_argument("--step", choices=("prepare", "parent", "new"), help=argparse.SUPPRESS)
    ap.add_argument("--rep", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.step:
        return {"prepare": prepare, "parent": parent_step, "new": new_step}[args.step](args)
    if args.parent_library and args.parent_reps < 5:
        ap.error("the parent's spread needs at least five repetitions")

    with tempfile.TemporaryDirectory() as tmp:
        work = args.work or tmp
        os.makedirs(work, exist_ok=True)

        def child(step, rep=0, env=None):
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, "--rep", str(rep),
                   "--length", str(args.length), "--k", str(args.k), "--device", str(args.device), "--work", work]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True)
            if r.returncode != 0:  # nothing more is started on the GPU
                sys.stderr.write(r.stderr[-4000:])
                raise SystemExit(f"step {step} (repetition {rep}) ended with status {r.returncode}")
            line = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")][-1]
            print(json.dumps(line), flush=True)
            return line

        doc = {"tool": "kmer_abundance_timing", "length": args.length, "k": args.k, "inputs": child("prepare")}
        if args.parent_library:
            env = dict(os.environ, MATCHTIGS_LIBRARY=os.path.abspath(args.parent_library))
            doc["parent"] = [child("parent", rep, env) for rep in range(args.parent_reps)]
        doc["new"] = [child("new", rep) for rep in range(args.reps)]

    steady = doc["new"][1:] or doc["new"]
    doc["summary"] = {f: [min(r[f] for r in steady), max(r[f] for r in steady)] for f in (
        "query_probe_ms", "weighted_query_probe_ms", "abundance_probe_ms", "abundance_per_window_probe_ms", "abundance_over_query",
        "abundance_per_window_over_query", "plain_build_ms", "locating_build_ms", "weighted_build_ms")}
    doc["summary"].update({f: doc["new"][0][f] for f in ("plain_device_bytes", "locating_device_bytes", "weighted_device_bytes")})
    if args.parent_library:
        probes = [r["query_probe_ms"] for r in doc["parent"][1:]]
        lo, hi = min(probes), max(probes)
        best = doc["summary"]["query_probe_ms"][0]
        doc["summary"]["parent_query_probe_ms_min_max"] = [lo, hi]
        doc["summary"]["parent_spread_max_over_min"] = round(hi / lo, 4)
        doc["summary"]["query_probe_best_over_parent_best"] = round(best / lo, 4)
        doc["summary"]["query_probe_within_parent_spread"] = bool(best <= hi)
        doc["summary"]["counts_equal_parent"] = all(doc["new"][0][f] == doc["parent"][0][f] for f in ("windows", "valid", "found"))
    print(json.dumps({"summary": doc["summary"]}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
