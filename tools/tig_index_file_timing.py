"""tig_index_file_timing.py -- what saving and reopening the sparse minimizer index costs (api.TigIndex.save / .load) on
the workload of tools/tig_payload_timing.py: G-seq, its unitigs and greedy tigs, plain (locating) and with that tool's synthetic
payloads; the query = the unitigs plus an equal volume with 3 % substitutions and an `N` every ~10^3 bases.

The parent process starts no GPU work. Every GPU step is a child process under its own `timeout`; the first that fails ends the run:
  prepare   tools/tig_payload_timing.py's: the sequences, the query and the payloads as .npy files in --work
  file      per (over, payloads), --reps times (at least five): build the index, save it, load the file, ask the LOADED index --
            file bytes against info.device_bytes, the phases of the save and the load (mtg_last_tig_index_file_times), the digest
            kernels' bytes per second over all sections (the launches of the 13 sections included) and as a fraction of --hbm-peak,
            the largest section's share of the bytes, the wall time of the load beside that of the build, and the query and locate
            probes of the loaded index
  parent    with --parent-library (libmatchtigs.so of the parent commit, built aside), plain ctypes: the build of the same locating
            index from its sequences and its query and locate probes on the built index -- the yardstick. The ratios are written
            down, not gated; the answers (valid, found) must agree, which the parent process checks.
Values are the median of the repetitions after the first, with min and max beside them. No speed is promised.

usage: python tools/tig_index_file_timing.py [--length 100000000] [--k 31] [--reps 5] [--device 0] [--parent-library PATH] [--work DIR]
                                             [--hbm-peak 8e12] [--step-timeout 900] [--out profiles/tig_index_file_gseq_1e8.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import tig_payload_timing as TP  # noqa: E402


def file_step(args) -> None:
    from matchtigs_amd import api

    k = args.k
    seq, off = TP.load(args.work, args.over + "_seq", args.over + "_off")
    weights, masks = TP.load(args.work, args.over + "_weights", args.over + "_masks") if args.payloads else (None, None)
    query = tuple(TP.load(args.work, "query_seq", "query_off"))
    path = os.path.join(args.work, "index.mtgx")
    for rep in range(args.reps):
        t0 = time.perf_counter()
        if args.payloads:
            ix = api.TigIndex.annotated((seq, off), k, None, args.device, weights=weights, colors=masks, n_colors=TP.N_COLORS)
        else:
            ix = api.TigIndex((seq, off), k, None, args.device, locate=True)
        build_wall_ms = 1e3 * (time.perf_counter() - t0)
        tb = api.last_tig_index_times()
        t0 = time.perf_counter()
        file_bytes = ix.save(path, {"indexed": args.over})
        save_wall_ms = 1e3 * (time.perf_counter() - t0)
        save = api.last_tig_index_file_times()["save"]
        device_bytes = ix.info.device_bytes
        ix.close()
        t0 = time.perf_counter()
        loaded = api.TigIndex.load(path, args.device)
        load_wall_ms = 1e3 * (time.perf_counter() - t0)
        load = api.last_tig_index_file_times()["load"]
        assert loaded.info.device_bytes == device_bytes
        q = loaded.query(query)
        query_probe_ms = api.last_tig_index_times()["query_probe_ms"]
        loc = loaded.locate(query)
        locate_probe_ms = api.last_tig_locate_times()["probe_ms"]
        loaded.close()
        head = api.tig_index_file_info(path)
        sections = {name: p["device_bytes"] for name, p in head["payload_info"].items()}
        i = head["info"]
        sections.update(packed=((i.characters + 15) // 16 + 2) * 4, off=(i.records + 1) * 8, dir=(i.buckets + 1) * 8, entries=i.anchors * 8,
                        table=i.table_slots * 8, heavy_where=i.table_slots * 8, win_off=head["win_offset_bytes"])
        digested = sum(sections.values())
        print(json.dumps({
            "step": "file", "over": args.over, "payloads": bool(args.payloads), "rep": rep, "file_bytes": file_bytes, "device_bytes": device_bytes,
            "section_bytes": digested, "largest_section": max(sections, key=sections.get), "largest_section_bytes": max(sections.values()),
            "build_wall_ms": round(build_wall_ms, 3),
            "build_kernels_ms": round(sum(v for f, v in tb.items() if f.startswith("build_") and f != "build_upload_ms"), 3),
            "save_wall_ms": round(save_wall_ms, 3), "save": {f: round(v, 3) for f, v in save.items()},
            "load_wall_ms": round(load_wall_ms, 3), "load": {f: round(v, 3) for f, v in load.items()},
            "save_digest_bytes_per_s": round(digested / (save["digest_ms"] / 1e3)), "load_digest_bytes_per_s": round(digested / (load["digest_ms"] / 1e3)),
            "query_probe_ms": round(query_probe_ms, 3), "locate_probe_ms": round(locate_probe_ms, 3),
            "answers": {"valid": int(q.valid.sum()), "found": int(q.found.sum()), "located": int(loc.found.sum()), "runs": len(loc.runs)}}), flush=True)
        os.remove(path)


def parent_step(args) -> None:
    """The parent commit's library through plain ctypes (it lacks the new entry points): build, query, locate."""
    L = C.CDLL(args.library)
    vp, u64 = C.c_void_p, C.c_uint64
    L.mtg_tig_index_build_locating.restype = vp
    L.mtg_tig_index_build_locating.argtypes = [vp, vp, u64, u64, u64, u64, C.c_int]
    L.mtg_tig_index_query.argtypes = [vp, vp, vp, u64, vp, vp, vp, vp, vp]
    L.mtg_tig_index_locate.argtypes = [vp, vp, vp, u64, vp, vp, vp, C.POINTER(vp)]
    L.mtg_kmer_runs_count.restype = u64
    L.mtg_kmer_runs_count.argtypes = [vp]
    L.mtg_kmer_runs_free.argtypes = [vp]
    L.mtg_tig_index_free.argtypes = [vp]
    L.mtg_last_tig_index_times.argtypes = [C.POINTER(C.c_double)]
    L.mtg_last_tig_locate_times.argtypes = [C.POINTER(C.c_double)]
    seq, off = TP.load(args.work, args.over + "_seq", args.over + "_off")
    q_seq, q_off = TP.load(args.work, "query_seq", "query_off")
    n, n_q = len(off) - 1, len(q_off) - 1
    kmers, valid, found = (np.zeros(n_q, np.uint64) for _ in range(3))
    for rep in range(args.reps):
        t0 = time.perf_counter()
        ix = L.mtg_tig_index_build_locating(seq.ctypes.data, off.ctypes.data, n, args.k, 0, 0, args.device)
        build_wall_ms = 1e3 * (time.perf_counter() - t0)
        t = (C.c_double * 8)()
        L.mtg_last_tig_index_times(t)
        build_kernels_ms = sum(t[1:5])
        L.mtg_tig_index_query(ix, q_seq.ctypes.data, q_off.ctypes.data, n_q, kmers.ctypes.data, valid.ctypes.data, found.ctypes.data, None, None)
        L.mtg_last_tig_index_times(t)
        answers = {"valid": int(valid.sum()), "found": int(found.sum())}
        runs, tl = vp(), (C.c_double * 4)()
        L.mtg_tig_index_locate(ix, q_seq.ctypes.data, q_off.ctypes.data, n_q, kmers.ctypes.data, valid.ctypes.data, found.ctypes.data, C.byref(runs))
        L.mtg_last_tig_locate_times(tl)
        answers.update(located=int(found.sum()), runs=int(L.mtg_kmer_runs_count(runs)))
        L.mtg_kmer_runs_free(runs)
        L.mtg_tig_index_free(ix)
        print(json.dumps({"step": "parent", "over": args.over, "rep": rep, "build_wall_ms": round(build_wall_ms, 3),
                          "build_kernels_ms": round(build_kernels_ms, 3), "query_probe_ms": round(t[7], 3), "locate_probe_ms": round(tl[2], 3),
                          "answers": answers}), flush=True)


def spread(reps, field, sub=None):
    later = reps[1:] or reps
    values = [(x[sub][field] if sub else x[field]) for x in later]
    return {"median": round(statistics.median(values), 3), "min": min(values), "max": max(values)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=100_000_000)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--change", type=float, default=0.4, help="the payload model of tools/tig_payload_timing.py")
    ap.add_argument("--parent-library", help="libmatchtigs.so of the parent commit, built aside: the yardstick")
    ap.add_argument("--hbm-peak", type=float, default=8e12, help="bytes per second the digest's rate is held against (MI355X: 8 TB/s)")
    ap.add_argument("--work", help="directory for the steps' inputs and the index file (default: a temporary one)")
    ap.add_argument("--step-timeout", type=int, default=900, help="seconds a child may take")
    ap.add_argument("--out")
    ap.add_argument("--step", choices=("prepare", "file", "parent"), help=argparse.SUPPRESS)
    ap.add_argument("--over", default="unitigs", help=argparse.SUPPRESS)
    ap.add_argument("--payloads", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--library", help=argparse.SUPPRESS)
    ap.add_argument("--m", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step == "prepare":
        return TP.prepare_step(args)
    if args.step == "file":
        return file_step(args)
    if args.step == "parent":
        return parent_step(args)
    if args.reps < 5:
        ap.error("the spread needs at least five repetitions")

    with tempfile.TemporaryDirectory() as tmp:
        work = args.work or tmp
        os.makedirs(work, exist_ok=True)

        def child(step, *extra):
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, "--k", str(args.k),
                   "--device", str(args.device), "--work", work, "--reps", str(args.reps), "--length", str(args.length), "--change", str(args.change),
                   *extra]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:  # nothing more is started on the GPU
                sys.stderr.write(r.stderr[-4000:])
                raise SystemExit(f"step {step} {' '.join(extra)} ended with status {r.returncode}")
            rows = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
            for row in rows:
                print(json.dumps(row), flush=True)
            return rows

        doc = {"tool": "tig_index_file_timing", "length": args.length, "k": args.k, "reps": args.reps, "hbm_peak_bytes_per_s": args.hbm_peak,
               "values": "median of the repetitions after the first, min and max beside it", "workload": child("prepare")[-1], "runs": {}, "parent": {}}
        for over in ("unitigs", "greedytigs"):
            if args.parent_library:
                reps = child("parent", "--over", over, "--library", os.path.abspath(args.parent_library))
                doc["parent"][over] = {"answers": reps[0]["answers"], "reps": reps,
                                       **{f: spread(reps, f) for f in ("build_wall_ms", "build_kernels_ms", "query_probe_ms", "locate_probe_ms")}}
            for payloads in (0, 1):
                reps = child("file", "--over", over, "--payloads", str(payloads))
                run = {f: reps[0][f] for f in ("file_bytes", "device_bytes", "section_bytes", "largest_section", "largest_section_bytes", "answers")}
                run["file_over_device_bytes"] = round(run["file_bytes"] / run["device_bytes"], 5)
                run.update({f: spread(reps, f) for f in ("build_wall_ms", "build_kernels_ms", "save_wall_ms", "load_wall_ms", "query_probe_ms",
                                                         "locate_probe_ms", "save_digest_bytes_per_s", "load_digest_bytes_per_s")})
                run["save"] = {f: spread(reps, f, "save") for f in reps[0]["save"]}
                run["load"] = {f: spread(reps, f, "load") for f in reps[0]["load"]}
                run["load_digest_fraction_of_hbm_peak"] = round(run["load_digest_bytes_per_s"]["median"] / args.hbm_peak, 5)
                run["save_digest_fraction_of_hbm_peak"] = round(run["save_digest_bytes_per_s"]["median"] / args.hbm_peak, 5)
                run["load_over_build_wall"] = round(run["load_wall_ms"]["median"] / run["build_wall_ms"]["median"], 4)
                if over in doc["parent"] and not payloads:
                    p = doc["parent"][over]
                    run["against_parent"] = {"load_wall_over_parent_build_wall": round(run["load_wall_ms"]["median"] / p["build_wall_ms"]["median"], 4),
                                             "query_probe_over_parent": round(run["query_probe_ms"]["median"] / p["query_probe_ms"]["median"], 4),
                                             "locate_probe_over_parent": round(run["locate_probe_ms"]["median"] / p["locate_probe_ms"]["median"], 4),
                                             "answers_equal": run["answers"] == p["answers"]}
                run["reps"] = reps
                doc["runs"][f"{over}/{'payloads' if payloads else 'plain'}"] = run
    if not args.parent_library:
        doc["parent"] = "not measured (no --parent-library given)"
    print(json.dumps({name: {f: r[f] for f in ("file_over_device_bytes", "load_over_build_wall", "load_digest_fraction_of_hbm_peak", "against_parent")
                             if f in r} for name, r in doc["runs"].items()}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    if any(not r.get("against_parent", {}).get("answers_equal", True) for r in doc["runs"].values()):
        raise SystemExit("the loaded index and the parent's built index disagree on the answers")


if __name__ == "__main__":
    main()
