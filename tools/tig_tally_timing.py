"""tig_tally_timing.py -- what counting reads on the sparse minimizer index costs (api.TigTally, mtg_tig_tally_*) beside
the table's tally and beside the sparse index's own locate probe, on DESIGN.md 29's workload: the four haplotypes of G-seq, k = 31,
indexed as their unitigs and as their greedy tigs; the SAMPLE is the haplotypes cut into reads of 151 bases that overlap by k - 1.

The parent process starts no GPU work. Every GPU step is a child process under its own `timeout -k 10`; the first that fails ends the run:
  prepare         the unitigs (the GPU compaction's store), the greedy tigs (device order, spelled on the GPU) and the reads, written
                  once as .npy files into --work (every later child reads the same bytes)
  parent <rep>    the PARENT commit's library, built aside and named by --parent-library, loaded through MATCHTIGS_LIBRARY with plain
                  ctypes (it lacks the new entry points, which matchtigs_amd._lib insists on): the yardsticks -- mtg_kmer_tally_add /
                  _coverage on the table over the unitigs, and mtg_tig_index_query / mtg_tig_index_locate on the locating sparse index
                  over the unitigs and over the greedy tigs (the locate probe is the floor add cannot beat), each called twice
  new <rep>       this library: the same calls (their kernels are not touched: they must stay inside the parent's spread) and
                  TigTally.add(reads) / .coverage(unitigs) over both texts, each called twice; device bytes; the checks below
Of each child the SECOND call of every probe is reported (the first also pays the arena's first chunks). --reps children of either
library (at least five) give the run-to-run spread (max / min), and the parent's own spread stands beside every ratio
(best new / best parent). No ratio is promised. Checked: the sparse tallies' add counts and coverage arrays equal the table's, every
window of the unitigs is found, the sum of `sum` over the unitigs equals the windows added, the counters sum to the same, as many
counters are non-zero as there are distinct k-mers, every child of either library reports the same counts, runs and digest, and
(with --parent-library) the best query and locate probe of this library's children, over either text, is at or below the slowest of
the parent's: inside the parent's own spread. A check that fails ends the run with a non-zero status after the JSON is written.

usage: python tools/tig_tally_timing.py --parent-library PATH [--length 100000000] [--k 31] [--m 19] [--reps 5] [--device 0]
                                        [--read-length 151] [--work DIR] [--step-timeout 900] [--out profiles/tig_tally_gseq_1e8.json]
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

TEXTS = ("unitigs", "greedytigs")


def load(work, *names):
    return [np.ascontiguousarray(np.load(os.path.join(work, n + ".npy"))) for n in names]


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def prepare(args) -> None:
    import torch  # noqa: F401  (one HIP runtime for torch and the library)

    from compact_timing import haplotype_arrays
    from kmer_compare_timing import fasta_sequence_arrays
    from kmer_tally_timing import cut_into_reads
    from matchtigs_amd import api

    k, t0 = args.k, time.perf_counter()
    reads, reads_off = haplotype_arrays(args.length, 1)
    store, c = api.compact_unitigs((reads, reads_off), k, args.device)
    reads, reads_off = cut_into_reads(reads, reads_off, args.read_length, k)
    seq, off = store.arrays()
    seq, off = np.asarray(seq), off.astype(np.uint64)
    graph = api.Bigraph.from_sequences((seq, off), k, args.device)  # (the `--seq-in` route's graph of the store)
    lim, ed = api.GreedytigAlgorithm.compute_tigs_np(graph, api.GreedytigAlgorithmConfiguration(1, k, euler_mode=api.EulerMode.Device,
                                                                                                device_ids=(args.device,)))
    tig_seq, tig_off = fasta_sequence_arrays(api.write_walks_text_device(graph, (lim, ed), (seq, off), k, device_id=args.device))
    del graph, lim, ed
    api.release_device_memory(args.device)
    out = {"unitigs_seq": seq, "unitigs_off": off, "greedytigs_seq": tig_seq, "greedytigs_off": tig_off.astype(np.uint64), "reads_seq": reads,
           "reads_off": reads_off}
    for name, a in out.items():
        np.save(os.path.join(args.work, name + ".npy"), a)
    win = lambda o: int(np.maximum(np.diff(o.astype(np.int64)) - (k - 1), 0).sum())
    print(json.dumps({"step": "prepare", "distinct_kmers": c.distinct_kmers, "unitigs": len(off) - 1, "unitig_characters": int(off[-1]),
                      "unitig_windows": win(off), "greedytigs": len(tig_off) - 1, "greedytig_characters": int(tig_off[-1]),
                      "greedytig_windows": win(tig_off), "reads": len(reads_off) - 1, "read_characters": int(reads_off[-1]),
                      "read_windows": win(reads_off), "seconds": round(time.perf_counter() - t0, 1)}), flush=True)


def parent_step(args) -> None:
    """The yardsticks through plain ctypes: only entry points the parent commit has."""
    from matchtigs_amd import _lib  # (the structures' layouts only; the library it would load is never asked for)

    L = C.CDLL(os.environ["MATCHTIGS_LIBRARY"])
    vp, u64 = C.c_void_p, C.c_uint64
    for f in ("mtg_kmer_index_build", "mtg_kmer_tally_create", "mtg_tig_index_build_locating"):
        getattr(L, f).restype = vp
    L.mtg_kmer_tally_device_bytes.restype = L.mtg_kmer_runs_count.restype = u64
    L.mtg_kmer_index_build.argtypes = [vp, vp, u64, u64, C.c_int]
    L.mtg_kmer_index_get_info.argtypes = [vp, C.POINTER(_lib.MtgKmerIndexInfo)]
    L.mtg_kmer_index_free.argtypes = L.mtg_kmer_tally_create.argtypes = L.mtg_kmer_tally_free.argtypes = L.mtg_kmer_tally_reset.argtypes = [vp]
    L.mtg_kmer_tally_device_bytes.argtypes = L.mtg_tig_index_free.argtypes = L.mtg_kmer_runs_count.argtypes = L.mtg_kmer_runs_free.argtypes = [vp]
    L.mtg_kmer_tally_add.argtypes = [vp, vp, vp, u64, vp, vp, vp]
    L.mtg_kmer_tally_coverage.argtypes = [vp, vp, vp, u64, vp, vp, vp, vp, vp, vp, vp]
    L.mtg_tig_index_build_locating.argtypes = [vp, vp, u64, u64, u64, u64, C.c_int]
    L.mtg_tig_index_get_info.argtypes = [vp, C.POINTER(_lib.MtgTigIndexInfo)]
    L.mtg_tig_index_query.argtypes = [vp, vp, vp, u64, vp, vp, vp, vp, vp]
    L.mtg_tig_index_locate.argtypes = [vp, vp, vp, u64, vp, vp, vp, C.POINTER(vp)]
    for f in ("mtg_last_kmer_tally_times", "mtg_last_tig_index_times", "mtg_last_tig_locate_times"):
        getattr(L, f).argtypes = [C.POINTER(C.c_double)]
    k, dev = args.k, args.device
    r_seq, r_off, u_seq, u_off = load(args.work, "reads_seq", "reads_off", "unitigs_seq", "unitigs_off")
    n_r, n_u = len(r_off) - 1, len(u_off) - 1
    out = {"step": "parent", "rep": args.rep}
    p = lambda a: a.ctypes.data
    # the table's tally over the unitigs
    ix = L.mtg_kmer_index_build(p(u_seq), p(u_off), n_u, k, dev)
    info = _lib.MtgKmerIndexInfo()
    L.mtg_kmer_index_get_info(ix, C.byref(info))
    tally = L.mtg_kmer_tally_create(ix)
    kmers, valid, found = (np.zeros(n_r, np.uint64) for _ in range(3))
    t = (C.c_double * 4)()
    for _ in range(2):  # the second call finds the arena's chunks in place
        L.mtg_kmer_tally_reset(tally)
        L.mtg_kmer_tally_add(tally, p(r_seq), p(r_off), n_r, p(kmers), p(valid), p(found))
        L.mtg_last_kmer_tally_times(t)
    out.update(table_add_ms=round(t[2], 3), windows=int(kmers.sum()), valid=int(valid.sum()), found=int(found.sum()),
               table_index_bytes=int(info.device_bytes), table_tally_bytes=int(L.mtg_kmer_tally_device_bytes(tally)))
    ck, cv, cf, cc, cs, cm = (np.zeros(n_u, np.uint64) for _ in range(6))
    for _ in range(2):
        L.mtg_kmer_tally_coverage(tally, p(u_seq), p(u_off), n_u, p(ck), p(cv), p(cf), p(cc), p(cs), p(cm), None)
        L.mtg_last_kmer_tally_times(t)
    out.update(table_coverage_ms=round(t[2], 3), store_found=int(cf.sum()), coverage_sum=int(cs.sum()), coverage_digest=digest(cc, cs, cm))
    L.mtg_kmer_tally_free(tally)
    L.mtg_kmer_index_free(ix)
    # the sparse index's own probes: membership and locate
    for text in TEXTS:
        seq, off = load(args.work, text + "_seq", text + "_off")
        ix = L.mtg_tig_index_build_locating(p(seq), p(off), len(off) - 1, k, args.m or 0, 0, dev)
        ti = _lib.MtgTigIndexInfo()
        L.mtg_tig_index_get_info(ix, C.byref(ti))
        t8, t4 = (C.c_double * 8)(), (C.c_double * 4)()
        for _ in range(2):
            L.mtg_tig_index_query(ix, p(r_seq), p(r_off), n_r, p(kmers), p(valid), p(found), None, None)
            L.mtg_last_tig_index_times(t8)
        out[f"{text}_query_ms"] = round(t8[7], 3)
        for _ in range(2):
            h = vp()
            L.mtg_tig_index_locate(ix, p(r_seq), p(r_off), n_r, p(kmers), p(valid), p(found), C.byref(h))
            L.mtg_last_tig_locate_times(t4)
            runs = int(L.mtg_kmer_runs_count(h))
            L.mtg_kmer_runs_free(h)
        out.update({f"{text}_locate_ms": round(t4[2], 3), f"{text}_index_bytes": int(ti.device_bytes), f"{text}_found": int(found.sum()),
                    f"{text}_runs": runs})
        L.mtg_tig_index_free(ix)
    print(json.dumps(out), flush=True)


def new_step(args) -> None:
    from matchtigs_amd import api

    k, dev = args.k, args.device
    r_seq, r_off, u_seq, u_off = load(args.work, "reads_seq", "reads_off", "unitigs_seq", "unitigs_off")
    reads, unitigs = (r_seq, r_off), (u_seq, u_off)
    out = {"step": "new", "rep": args.rep}
    with api.KmerIndex(unitigs, k, dev) as ix, api.KmerTally(ix) as tally:
        for _ in range(2):  # the second call finds the arena's chunks in place
            tally.reset()
            a = tally.add(reads)
        out.update(table_add_ms=round(api.last_kmer_tally_times()["probe_ms"], 3), windows=int(a.kmers.sum()), valid=int(a.valid.sum()),
                   found=int(a.found.sum()), table_index_bytes=ix.info.device_bytes, table_tally_bytes=tally.device_bytes)
        for _ in range(2):
            want = tally.coverage(unitigs)
        out.update(table_coverage_ms=round(api.last_kmer_tally_times()["probe_ms"], 3), store_found=int(want.found.sum()),
                   coverage_sum=int(want.sum.sum()), coverage_digest=digest(want.covered, want.sum, want.max))
    want_add = a
    for text in TEXTS:
        indexed = tuple(load(args.work, text + "_seq", text + "_off"))
        with api.TigIndex(indexed, k, args.m, dev, locate=True) as ix, api.TigTally(ix) as tally:
            for _ in range(2):
                q = ix.query(reads)
            out[f"{text}_query_ms"] = round(api.last_tig_index_times()["query_probe_ms"], 3)
            for _ in range(2):
                loc = ix.locate(reads)
            out.update({f"{text}_locate_ms": round(api.last_tig_locate_times()["probe_ms"], 3), f"{text}_runs": len(loc.runs),
                        f"{text}_found": int(loc.found.sum())})
            del loc
            for _ in range(2):
                tally.reset()
                t0 = time.perf_counter()
                a = tally.add(reads)
                wall = 1e3 * (time.perf_counter() - t0)
            t = api.last_tig_tally_times()
            out.update({f"{text}_add_probe_ms": round(t["probe_ms"], 3), f"{text}_add_pass2_ms": round(t["pass2_ms"], 3),
                        f"{text}_add_ms": round(t["probe_ms"] + t["pass2_ms"], 3), f"{text}_add_wall_ms": round(wall, 3)})
            for _ in range(2):
                cov = tally.coverage(unitigs)
            t = api.last_tig_tally_times()
            counters = tally.counters()
            out.update({f"{text}_coverage_probe_ms": round(t["probe_ms"], 3), f"{text}_coverage_pass2_ms": round(t["pass2_ms"], 3),
                        f"{text}_coverage_ms": round(t["probe_ms"] + t["pass2_ms"], 3), f"{text}_index_bytes": ix.info.device_bytes,
                        f"{text}_tally_bytes": tally.device_bytes, f"{text}_windows": tally.windows,
                        f"{text}_counters_sum": int(counters.sum()), f"{text}_counters_nonzero": int(np.count_nonzero(counters)),
                        f"{text}_add_equals_table": bool(all(np.array_equal(getattr(a, f), getattr(want_add, f)) for f in ("kmers", "valid", "found"))),
                        f"{text}_add_equals_query": bool(np.array_equal(a.found, q.found) and np.array_equal(a.valid, q.valid)),
                        f"{text}_coverage_equals_table": bool(all(np.array_equal(getattr(cov, f), getattr(want, f))
                                                                  for f in ("kmers", "valid", "found", "covered", "sum", "max"))),
                        f"{text}_store_all_found": bool(np.array_equal(cov.found, cov.kmers)),
                        f"{text}_coverage_sum": int(cov.sum.sum())})
            del counters, cov, q
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

        doc = {"tool": "tig_tally_timing", "length": args.length, "haplotypes": 4, "k": args.k, "read_length": args.read_length,
               "inputs": child("prepare")}
        if args.parent_library:
            env = dict(os.environ, MATCHTIGS_LIBRARY=os.path.abspath(args.parent_library))
            doc["parent"] = [child("parent", rep, env) for rep in range(args.reps)]
        doc["new"] = [child("new", rep) for rep in range(args.reps)]

    def spread(rows, f):
        v = [r[f] for r in rows]
        return {"min": min(v), "max": max(v), "max_over_min": round(max(v) / min(v), 4)}

    new, yard = doc["new"], doc.get("parent") or doc["new"]
    distinct = doc["inputs"]["distinct_kmers"]
    s = {"yardsticks_from": "parent library" if args.parent_library else "this library (no --parent-library given)",
         "found": new[0]["found"], "windows": new[0]["windows"],
         "table_bytes_per_distinct_kmer": round((new[0]["table_index_bytes"] + new[0]["table_tally_bytes"]) / distinct, 3)}
    for f in ("table_add_ms", "table_coverage_ms"):
        s[f] = spread(new, f)
        s["yardstick_" + f] = spread(yard, f)
    for text in TEXTS:
        for f in ("query_ms", "locate_ms"):
            s[f"{text}_{f}"] = spread(new, f"{text}_{f}")
            s[f"yardstick_{text}_{f}"] = spread(yard, f"{text}_{f}")
            s[f"{text}_{f}_over_yardstick"] = round(s[f"{text}_{f}"]["min"] / s[f"yardstick_{text}_{f}"]["min"], 4)
        for f in ("add_ms", "add_probe_ms", "add_pass2_ms", "coverage_ms", "coverage_probe_ms", "coverage_pass2_ms"):
            s[f"{text}_{f}"] = spread(new, f"{text}_{f}")
        locate, n0 = s[f"yardstick_{text}_locate_ms"]["min"], new[0]
        s[f"{text}_bytes_per_distinct_kmer"] = round((n0[f"{text}_index_bytes"] + n0[f"{text}_tally_bytes"]) / distinct, 3)
        s[f"{text}_bytes_over_table"] = round((n0[f"{text}_index_bytes"] + n0[f"{text}_tally_bytes"]) / (n0["table_index_bytes"] + n0["table_tally_bytes"]), 4)
        s[f"{text}_add_over_locate_probe"] = round(s[f"{text}_add_ms"]["min"] / locate, 4)
        s[f"{text}_coverage_over_locate_probe"] = round(s[f"{text}_coverage_ms"]["min"] / locate, 4)  # (another query: the unitigs, not the reads)
        s[f"{text}_add_over_table_add"] = round(s[f"{text}_add_ms"]["min"] / s["yardstick_table_add_ms"]["min"], 4)
        s[f"{text}_coverage_over_table_coverage"] = round(s[f"{text}_coverage_ms"]["min"] / s["yardstick_table_coverage_ms"]["min"], 4)
    checks = {}
    for text in TEXTS:
        for f in ("add_equals_table", "add_equals_query", "coverage_equals_table", "store_all_found"):
            checks[f"{text}_{f}"] = all(r[f"{text}_{f}"] for r in new)
        checks[f"{text}_coverage_sum_equals_found"] = all(r[f"{text}_coverage_sum"] == r["found"] == r[f"{text}_counters_sum"] for r in new)
        checks[f"{text}_nonzero_counters_equal_distinct_kmers"] = all(r[f"{text}_counters_nonzero"] == distinct for r in new)
        if args.parent_library:  # (without it the yardstick is this run itself)
            for f in ("query_ms", "locate_ms"):  # untouched kernels: the best of this library's children is no slower than the parent's slowest
                # (tools/tig_locate_timing.py's guard; a best below the parent's is noise in the welcome direction)
                checks[f"{text}_{f}_within_parent_spread"] = s[f"{text}_{f}"]["min"] <= s[f"yardstick_{text}_{f}"]["max"]
    checks["counts_equal_yardstick"] = all(r[f] == yard[0][f] for r in new + yard for f in (
        "windows", "valid", "found", "store_found", "coverage_sum", "coverage_digest", "unitigs_found", "greedytigs_found", "unitigs_runs",
        "greedytigs_runs"))
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
