"""kmer_color_timing.py -- what colours cost (mtg_compact_unitigs_colored, mtg_kmer_index_colors) on the input of
DESIGN.md 16: the four haplotypes of G-seq (tools/compact_timing.py's arrays), k = 31, each cut into --pieces records that overlap by
k - 1 bases (the same k-mer set). Two colourings of the same records: one colour per haplotype (C = 4), and 64 colours dealt
round-robin over the records (C = 64). The query set is that of kmer_query_timing.py over the compaction's unitigs: the unitigs plus
an equal volume of them with 3 % substitutions and an `N` every ~10^3 bases.

Every GPU step is a child process of its own, under its own `timeout`, and the first one that fails ends the run:
  prepare         the records, written once as .npy files into --work (every later child reads the same bytes)
  parent <rep>    the PARENT commit's library, built aside and named by --parent-library, loaded through MATCHTIGS_LIBRARY with plain
                  ctypes: mtg_compact_unitigs_counted_kmers at m = 1 (the yardstick of the compaction), then a plain index of its
                  unitigs and `query` without bit arrays (the yardstick of the probe)
  new <rep>       this library: the coloured call at C = 4 and C = 64 -- the twelve figures of mtg_last_compact_times, the peak arena,
                  the statistics kernel alone --, the counted and the plain call (unchanged machine code: they must stay within the
                  parent's spread), and the build and the probe of a coloured index against a plain one
At least five repetitions of the parent give its run-to-run spread (min, max, max / min after the first repetition, which also pays
the arena's first chunks); it is written beside each ratio: coloured insert / parent counted insert, whole call / parent whole call,
colour probe / plain probe.

usage: python tools/kmer_color_timing.py [--parent-library PATH] [--length 100000000] [--pieces 64] [--k 31] [--reps 5]
                                         [--device 0] [--work DIR] [--step-timeout 900] [--out profiles/kmer_color_gseq_1e8.json]
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

TIMES = ("upload_ms", "pack_ms", "insert_ms", "ids_ms", "nodes_ms", "rank_ms", "emit_ms", "download_ms", "total_ms", "rounds", "bytes",
         "peak_arena_bytes")


def _rounded(t: dict) -> dict:
    return {f: (round(v, 3) if isinstance(v, float) else int(v)) for f, v in t.items()}


def _noisy_query(seq, off):
    rng = np.random.default_rng(1)
    noisy = seq.copy()
    sub = rng.random(len(seq)) < 0.03
    noisy[sub] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(sub.sum()))]
    noisy[rng.random(len(seq)) < 1e-3] = ord("N")
    return np.concatenate([seq, noisy]), np.concatenate([off, off[1:] + off[-1]]).astype(np.uint64)


def prepare(args) -> None:
    from compact_timing import haplotype_arrays

    data, hap_off = haplotype_arrays(args.length, 1)
    step = -(-args.length // args.pieces)
    starts = np.concatenate([h + np.arange(0, args.length, step) for h in hap_off[:-1].astype(np.int64)])
    ends = np.minimum(starts + step + args.k - 1, (starts // args.length + 1) * args.length)
    seq = np.concatenate([data[a:b] for a, b in zip(starts.tolist(), ends.tolist())])
    off = np.concatenate([[0], np.cumsum(ends - starts)]).astype(np.uint64)
    np.save(os.path.join(args.work, "seq.npy"), seq)
    np.save(os.path.join(args.work, "off.npy"), off)
    np.save(os.path.join(args.work, "haplotype.npy"), (starts // args.length).astype(np.uint8))
    print(json.dumps({"step": "prepare", "records": len(off) - 1, "characters": int(off[-1])}), flush=True)


def _load(work):
    return tuple(np.ascontiguousarray(np.load(os.path.join(work, f + ".npy"))) for f in ("seq", "off", "haplotype"))


def parent_step(args) -> None:
    from matchtigs_amd import _lib  # (the structures' layout only; the library it would load is never asked for)

    L = C.CDLL(os.environ["MATCHTIGS_LIBRARY"])
    vp, u64, P = C.c_void_p, C.c_uint64, C.POINTER
    L.mtg_compact_unitigs_counted_kmers.argtypes = [vp, vp, u64, u64, u64, C.c_int, P(vp), P(_lib.MtgCompaction), P(_lib.MtgAbundance), P(vp), P(vp)]
    L.mtg_last_compact_times.argtypes = [P(C.c_double)]
    for f, res, a in (("mtg_unitigs_count", u64, [vp]), ("mtg_unitigs_data", vp, [vp]), ("mtg_unitigs_offsets", vp, [vp]), ("mtg_unitigs_free", None, [vp]),
                      ("mtg_abundance_sums_free", None, [vp]), ("mtg_kmer_counts_free", None, [vp]), ("mtg_kmer_index_build_store", vp, [vp, u64, C.c_int]),
                      ("mtg_kmer_index_query", None, [vp, vp, vp, u64, vp, vp, vp, vp, vp]), ("mtg_kmer_index_free", None, [vp]),
                      ("mtg_last_kmer_query_times", None, [P(C.c_double)])):
        getattr(L, f).restype, getattr(L, f).argtypes = res, a
    seq, off, _ = _load(args.work)
    out, sums, counts, stats, ab, times = vp(), vp(), vp(), _lib.MtgCompaction(), _lib.MtgAbundance(), (C.c_double * 12)()
    t0 = time.perf_counter()
    L.mtg_compact_unitigs_counted_kmers(seq.ctypes.data, off.ctypes.data, len(off) - 1, args.k, 1, args.device, C.byref(out), C.byref(stats),
                                        C.byref(ab), C.byref(sums), C.byref(counts))
    wall = time.perf_counter() - t0
    L.mtg_last_compact_times(times)
    line = {"step": "parent", "rep": args.rep, "counted": {**_rounded(dict(zip(TIMES, list(times)))), "wall_ms": round(1e3 * wall, 3)},
            "distinct_kmers": int(stats.distinct_kmers), "unitigs": int(stats.unitigs)}
    n = int(L.mtg_unitigs_count(out))
    u_off = np.ctypeslib.as_array(C.cast(L.mtg_unitigs_offsets(out), P(u64)), shape=(n + 1,)).copy()
    u_seq = np.ctypeslib.as_array(C.cast(L.mtg_unitigs_data(out), P(C.c_uint8)), shape=(int(u_off[-1]),)).copy()
    q_seq, q_off = _noisy_query(u_seq, u_off)
    ix = L.mtg_kmer_index_build_store(out, args.k, args.device)
    kmers, valid, found = (np.zeros(len(q_off) - 1, np.uint64) for _ in range(3))
    probes = []
    for _ in range(2):  # the second call finds the arena's chunks in place
        L.mtg_kmer_index_query(ix, q_seq.ctypes.data, q_off.ctypes.data, len(q_off) - 1, kmers.ctypes.data, valid.ctypes.data, found.ctypes.data, None, None)
        t = (C.c_double * 6)()
        L.mtg_last_kmer_query_times(t)
        probes.append(round(t[5], 3))
    line.update(plain_build_insert_ms=round(t[2], 3), query_probe_ms_first=probes[0], query_probe_ms=probes[1], found=int(found.sum()))
    L.mtg_kmer_index_free(ix)
    for free, h in ((L.mtg_unitigs_free, out), (L.mtg_abundance_sums_free, sums), (L.mtg_kmer_counts_free, counts)):
        free(h)
    print(json.dumps(line), flush=True)


def new_step(args) -> None:
    from matchtigs_amd import api

    seq, off, haplotype = _load(args.work)
    n = len(off) - 1
    line = {"step": "new", "rep": args.rep}

    def timed(call):
        t0 = time.perf_counter()
        r = call()
        return r, {**_rounded(api.last_compact_times()), "wall_ms": round(1e3 * (time.perf_counter() - t0), 3)}

    _, line["plain"] = timed(lambda: api.compact_unitigs((seq, off), args.k, args.device))
    counted, line["counted"] = timed(lambda: api.compact_unitigs_counted((seq, off), args.k, 1, args.device, kmer_counts=True))
    for name, colors, c in (("colored_4", haplotype, 4), ("colored_64", (np.arange(n) % 64).astype(np.uint8), 64)):
        r, line[name] = timed(lambda: api.compact_unitigs_colored((seq, off), args.k, colors, c, 1, args.device))
        line[name]["stats_ms"] = round(api.last_kmer_color_times()["stats_ms"], 3)
        line[name]["core"], line[name]["private"] = r[3].core, r[3].private
        line[name]["equals_counted"] = bool(np.array_equal(r[0].arrays()[0], counted[0].arrays()[0]) and np.array_equal(r[2].kmer_counts, counted[2].kmer_counts))
    store, col = r[0], r[3]
    q = _noisy_query(*store.arrays())
    with api.KmerIndex(store, args.k, args.device) as ix:
        line["plain_build_insert_ms"] = round(api.last_kmer_query_times()["build_insert_ms"], 3)
        for _ in range(2):  # the second call finds the arena's chunks in place
            plain = ix.query(q)
        line["query_probe_ms"] = round(api.last_kmer_query_times()["query_probe_ms"], 3)
    with api.KmerIndex(store, args.k, args.device, colors=col.kmer_colors, n_colors=64) as ix:
        line["colored_build_insert_ms"] = round(api.last_kmer_query_times()["build_insert_ms"], 3)
        for name, per_window in (("color_probe_ms", False), ("color_per_window_probe_ms", True)):
            for _ in range(2):
                hits = ix.color_hits(q, per_window=per_window)
            line[name] = round(api.last_kmer_color_times()["probe_ms"], 3)
        line["counts_equal_query"] = bool(np.array_equal(hits.found, plain.found) and np.array_equal(hits.valid, plain.valid))
    line["found"] = int(plain.found.sum())
    line["color_probe_over_plain_probe"] = round(line["color_probe_ms"] / line["query_probe_ms"], 3)
    print(json.dumps(line), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=100_000_000)
    ap.add_argument("--pieces", type=int, default=64, help="records per haplotype")
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
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
        ap.error("a spread needs at least five repetitions")

    with tempfile.TemporaryDirectory() as tmp:
        work = args.work or tmp
        os.makedirs(work, exist_ok=True)

        def child(step, rep=0, env=None):
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, "--rep", str(rep),
                   "--length", str(args.length), "--pieces", str(args.pieces), "--k", str(args.k), "--device", str(args.device), "--work", work]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True)
            if r.returncode != 0:  # nothing more is started on the GPU
                sys.stderr.write(r.stderr[-4000:])
                raise SystemExit(f"step {step} (repetition {rep}) ended with status {r.returncode}")
            line = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")][-1]
            print(json.dumps(line), flush=True)
            return line

        doc = {"tool": "kmer_color_timing", "length": args.length, "haplotypes": 4, "pieces": args.pieces, "k": args.k, "inputs": child("prepare")}
        if args.parent_library:
            env = dict(os.environ, MATCHTIGS_LIBRARY=os.path.abspath(args.parent_library))
            doc["parent"] = [child("parent", rep, env) for rep in range(args.reps)]
        doc["new"] = [child("new", rep) for rep in range(args.reps)]

    def spread(values):
        values = values[1:] or values  # (the first repetition also pays the arena's first chunks)
        return {"min": min(values), "max": max(values), "max_over_min": round(max(values) / min(values), 4)}

    new = doc["new"]
    s = doc["summary"] = {f"{call}_{f}": spread([r[call][f] for r in new]) for call in ("plain", "counted", "colored_4", "colored_64")
                          for f in ("insert_ms", "total_ms")}
    s.update({f: spread([r[f] for r in new]) for f in ("query_probe_ms", "color_probe_ms", "color_per_window_probe_ms", "color_probe_over_plain_probe")})
    s.update({f"{call}_stats_ms": spread([r[call]["stats_ms"] for r in new]) for call in ("colored_4", "colored_64")})
    s["colored_peak_arena_bytes"] = new[0]["colored_64"]["peak_arena_bytes"]
    s["counted_peak_arena_bytes"] = new[0]["counted"]["peak_arena_bytes"]
    s["outputs_equal_counted"] = all(r[c]["equals_counted"] for r in new for c in ("colored_4", "colored_64"))
    if args.parent_library:
        par = doc["parent"]
        for f in ("insert_ms", "total_ms"):
            p = s[f"parent_counted_{f}"] = spread([r["counted"][f] for r in par])
            for call in ("colored_4", "colored_64"):
                s[f"{call}_{f}_over_parent_counted"] = round(s[f"{call}_{f}"]["min"] / p["min"], 4)
            s[f"counted_{f}_within_parent_spread"] = bool(s[f"counted_{f}"]["min"] <= p["max"])
        p = s["parent_query_probe_ms"] = spread([r["query_probe_ms"] for r in par])
        s["query_probe_within_parent_spread"] = bool(s["query_probe_ms"]["min"] <= p["max"])
        s["color_probe_over_parent_query_probe"] = round(s["color_probe_ms"]["min"] / p["min"], 4)
    print(json.dumps({"summary": s}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
