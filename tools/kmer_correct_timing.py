"""kmer_correct_timing.py -- what read correction costs (api.ReadCorrector, mtg_kmer_index_correct) beside the parent's
`query` probe on the same reads, on DESIGN.md 29's workload: the four haplotypes of G-seq, k = 31, the table over their unitigs; the
READS are the haplotypes cut into reads of 151 bases that overlap by k - 1, with seeded uniform substitution errors planted at every
rate of --rates (0.5 % and 2 %). A correction run cannot cost less than its query passes, so that probe is the yardstick.

The parent process starts no GPU work. Every GPU step is a child process under its own `timeout -k 10`; the first that fails ends the run:
  prepare         the unitigs (the GPU compaction) and, per rate, the reads with their planted errors, written once as .npy files
  parent <rep>    the PARENT commit's library, built aside and named by --parent-library, loaded with plain ctypes (it lacks the new
                  entry points, which matchtigs_amd._lib insists on): on a locating, coloured table over the unitigs the query, locate
                  and colour probes of the reads of every rate, each called twice
  new <rep>       this library: the same calls through the same code (their kernels are not touched: they must stay inside the
                  parent's spread), then ReadCorrector.correct at R = 1 and R = 2 per rate, each called twice, with its phases
Of each child the SECOND call of everything is reported (the first also pays the arena's first chunks). --reps children of either
library (at least five) give the run-to-run spread (max / min), and the parent's own spread stands beside every ratio. Nothing about
speed is promised. Written down per rate and R: the kernels by HIP events and the whole call by the host clock, the ratio of either to
the yardstick, the candidates per read, and per round the share of planted errors restored, the substitutions that are wrong (the
position was not planted, or the base is not the original) and the errors left. Checked: the substitution lists are identical across
the children, they equal the restatement's (tests/kmer_correct_ref.py over the unitigs' k-mer set) on a seeded sample of --sample reads,
and (with --parent-library) the best query, locate and colour probe of this library's children is at or below the slowest of the
parent's. A check that fails ends the run with a non-zero status after the JSON is written.

usage: python tools/kmer_correct_timing.py --parent-library PATH [--length 100000000] [--k 31] [--reps 5] [--device 0] [--read-length 151]
                                           [--rates 0.005,0.02] [--min-solid 4] [--sample 40] [--work DIR] [--step-timeout 900]
                                           [--out profiles/kmer_correct_gseq_1e8.json]
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

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))

N_COLORS = 4
PROBES = ("query_ms", "locate_ms", "colors_ms")
ROUNDS = (1, 2)


def load(work, *names):
    return [np.ascontiguousarray(np.load(os.path.join(work, n + ".npy"))) for n in names]


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def tag(rate):
    return f"e{int(round(rate * 100000)):05d}"


def plant(reads, rate, seed):
    """Uniform substitution errors at `rate`, seeded: (the reads with errors, the positions, the original bases)."""
    from matchtigs_amd import synth

    n = len(reads)
    where = np.flatnonzero(synth._uniform01(synth.splitmix64(seed, n, 70)) < rate)
    shift = (synth.splitmix64(seed, n, 71)[where] % np.uint64(3)).astype(np.int64) + 1
    codes = np.zeros(256, np.int64)
    codes[np.frombuffer(b"ACGT", np.uint8)] = np.arange(4)
    out = reads.copy()
    out[where] = np.frombuffer(b"ACGT", np.uint8)[(codes[reads[where]] + shift) % 4]
    return out, where.astype(np.uint64), reads[where].copy()


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
           "reads_off": reads_off}
    planted = {}
    for i, rate in enumerate(args.rate_list):
        noisy, where, original = plant(reads, rate, 1000 + i)
        out.update({f"reads_{tag(rate)}": noisy, f"planted_{tag(rate)}": where, f"original_{tag(rate)}": original})
        planted[tag(rate)] = len(where)
    for name, a in out.items():
        np.save(os.path.join(args.work, name + ".npy"), a)
    print(json.dumps({"step": "prepare", "distinct_kmers": c.distinct_kmers, "unitigs": len(off) - 1, "unitig_characters": int(off[-1]),
                      "reads": len(reads_off) - 1, "read_characters": int(reads_off[-1]), "planted": planted,
                      "seconds": round(time.perf_counter() - t0, 1)}), flush=True)


def yardsticks(L, args, out) -> None:
    """The probes both libraries have, through plain ctypes, on the reads of every rate."""
    vp, u64, ci = C.c_void_p, C.c_uint64, C.c_int
    L.mtg_kmer_index_build_annotated.restype = vp
    L.mtg_kmer_index_build_annotated.argtypes = [vp, vp, u64, u64, vp, u64, vp, u64, u64, ci, ci]
    L.mtg_kmer_runs_count.restype = u64
    L.mtg_kmer_index_free.argtypes = L.mtg_kmer_runs_count.argtypes = L.mtg_kmer_runs_free.argtypes = [vp]
    L.mtg_kmer_index_query.argtypes = [vp, vp, vp, u64, vp, vp, vp, vp, vp]
    L.mtg_kmer_index_locate.argtypes = [vp, vp, vp, u64, vp, vp, vp, C.POINTER(vp)]
    L.mtg_kmer_index_colors.argtypes = [vp, vp, vp, u64, vp, vp, vp, vp, vp]
    for f in ("mtg_last_kmer_query_times", "mtg_last_kmer_locate_times", "mtg_last_kmer_color_times"):
        getattr(L, f).argtypes = [C.POINTER(C.c_double)]
    k, dev = args.k, args.device
    r_off, u_seq, u_off, masks = load(args.work, "reads_off", "unitigs_seq", "unitigs_off", "unitigs_masks")
    n_r, n_u = len(r_off) - 1, len(u_off) - 1
    p = lambda a: a.ctypes.data
    kmers, valid, found = (np.zeros(n_r, np.uint64) for _ in range(3))
    per_color = np.zeros((n_r, N_COLORS), np.uint32)
    ix = L.mtg_kmer_index_build_annotated(p(u_seq), p(u_off), n_u, k, None, 0, p(masks), len(masks), N_COLORS, 1, dev)
    t = (C.c_double * 8)()
    for rate in args.rate_list:
        e = tag(rate)
        (r_seq,) = load(args.work, f"reads_{e}")
        for _ in range(2):  # the second call finds the arena's chunks in place
            t0 = time.perf_counter()
            L.mtg_kmer_index_query(ix, p(r_seq), p(r_off), n_r, p(kmers), p(valid), p(found), None, None)
            wall = 1e3 * (time.perf_counter() - t0)
            L.mtg_last_kmer_query_times(t)
        out.update({f"{e}_query_ms": round(t[5], 3), f"{e}_query_wall_ms": round(wall, 3), f"{e}_found": int(found.sum()),
                    f"{e}_valid": int(valid.sum()), f"{e}_query_digest": digest(kmers, valid, found)})
        for _ in range(2):
            h = vp()
            L.mtg_kmer_index_locate(ix, p(r_seq), p(r_off), n_r, p(kmers), p(valid), p(found), C.byref(h))
            L.mtg_last_kmer_locate_times(t)
            runs = int(L.mtg_kmer_runs_count(h))
            L.mtg_kmer_runs_free(h)
        out.update({f"{e}_locate_ms": round(t[2], 3), f"{e}_runs": runs})
        for _ in range(2):
            L.mtg_kmer_index_colors(ix, p(r_seq), p(r_off), n_r, p(kmers), p(valid), p(found), p(per_color), None)
            L.mtg_last_kmer_color_times(t)
        out.update({f"{e}_colors_ms": round(t[3], 3), f"{e}_counters_digest": digest(per_color)})
    L.mtg_kmer_index_free(ix)


def parent_step(args) -> None:
    out = {"step": "parent", "rep": args.rep}
    yardsticks(C.CDLL(os.environ["MATCHTIGS_LIBRARY"]), args, out)
    print(json.dumps(out), flush=True)


def new_step(args) -> None:
    import kmer_correct_ref as CR
    from matchtigs_amd import _lib, api

    out = {"step": "new", "rep": args.rep}
    yardsticks(C.CDLL(str(_lib.LIB_PATH)), args, out)
    k, dev = args.k, args.device
    r_off, u_seq, u_off = load(args.work, "reads_off", "unitigs_seq", "unitigs_off")
    n_r = len(r_off) - 1
    with api.KmerIndex((u_seq, u_off), k, dev) as ix:
        for rate in args.rate_list:
            e = tag(rate)
            r_seq, planted, original = load(args.work, f"reads_{e}", f"planted_{e}", f"original_{e}")
            for R in ROUNDS:
                with api.ReadCorrector(ix, args.min_solid, R) as c:
                    for _ in range(2):
                        t0 = time.perf_counter()
                        r = c.correct((r_seq, r_off))
                        wall = 1e3 * (time.perf_counter() - t0)
                t = api.last_kmer_correct_times()
                key = f"{e}_r{R}"
                # what the substitutions did to the planted errors
                at = np.searchsorted(planted, r.positions)
                hit = (at < len(planted)) & (planted[np.minimum(at, len(planted) - 1)] == r.positions) if len(planted) else np.zeros(len(at), bool)
                restored = hit & (original[np.minimum(at, max(len(planted) - 1, 0))] == r.bases) if len(planted) else hit
                out.update({f"{key}_{f}": round(v, 3) for f, v in t.items()})
                out.update({f"{key}_wall_ms": round(wall, 3),
                            f"{key}_kernels_ms": round(t["query_ms"] + t["flag_ms"] + t["evaluate_ms"] + t["apply_ms"], 3),
                            f"{key}_candidates": int(r.candidates.sum()), f"{key}_candidates_per_read": round(float(r.candidates.sum()) / n_r, 4),
                            f"{key}_ambiguous": int(r.ambiguous.sum()), f"{key}_round_corrected": [int(x) for x in r.round_corrected[:R]],
                            f"{key}_substitutions": len(r.positions), f"{key}_restored": int(restored.sum()),
                            f"{key}_wrong": int(len(r.positions) - restored.sum()), f"{key}_errors_left": int(len(planted) - restored.sum()),
                            f"{key}_share_restored": round(float(restored.sum()) / max(len(planted), 1), 5),
                            f"{key}_found": int(r.found.sum()), f"{key}_found_after": int(r.found_after.sum()),
                            f"{key}_digest": digest(r.positions, r.bases, r.found_after, r.candidates, r.ambiguous, r.corrected)})
                # the restatement on a seeded sample of reads, against the unitigs' own k-mers around them: the set is too large for
                # Python, so membership is asked of the index itself, window by window, through the memo the restatement takes
                rng = np.random.default_rng(34 + R)
                sample = np.sort(rng.choice(n_r, size=min(args.sample, n_r), replace=False))
                reads = [bytes(r_seq[int(r_off[q]):int(r_off[q + 1])]).decode() for q in sample]
                memo = _Membership(ix, k)
                memo.prime(reads)
                want = CR.correct(None, k, reads, args.min_solid, R, memo)
                got_pos, got_base = [], []
                start = 0
                for q, x in zip(sample, reads):
                    lo, hi = np.searchsorted(r.positions, [r_off[q], r_off[q + 1]])
                    got_pos += (r.positions[lo:hi] - r_off[q] + np.uint64(start)).tolist()
                    got_base += [chr(b) for b in r.bases[lo:hi]]
                    start += len(x)
                out[f"{key}_sample_equals_restatement"] = bool(got_pos == want["positions"] and got_base == want["bases"]
                                                               and r.found_after[sample].tolist() == want["found_after"]
                                                               and r.candidates[sample].tolist() == want["candidates"]
                                                               and r.ambiguous[sample].tolist() == want["ambiguous"])
    print(json.dumps(out), flush=True)


class _Membership(dict):
    """The restatement's memo (window -> in the set), answered by the index's own query: the set is too large for Python. prime()
    asks in ONE call for every window of the reads and every single-base variant of it -- all that round 1 can ask for --; what a
    later round asks beyond that is asked window by window. The restatement still decides candidates, scores, ties and rounds."""

    def __init__(self, ix, k):
        super().__init__()
        self.ix, self.k = ix, k

    def prime(self, reads):
        k, rows = self.k, []
        others = {c: [b for b in b"ACGT" if b != c] for c in b"ACGT"}
        for x in reads:
            a = np.frombuffer(x.encode(), np.uint8)
            if len(a) < k:
                continue
            w = np.lib.stride_tricks.sliding_window_view(a, k)
            rows.append(w)
            for j in range(k):
                for s in range(3):
                    v = w.copy()
                    v[:, j] = [others.get(int(c), [65, 67, 71])[s] for c in w[:, j]]
                    rows.append(v)
        if not rows:
            return
        flat = np.unique(np.concatenate(rows), axis=0)
        r = self.ix.query((np.ascontiguousarray(flat).reshape(-1), np.arange(len(flat) + 1, dtype=np.uint64) * np.uint64(k)))
        for row, f in zip(flat, r.found.tolist()):
            self[row.tobytes().decode()] = bool(f)

    def get(self, w, default=None):
        if w not in self:
            self[w] = bool(self.ix.query([w]).found[0])
        return self[w]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=100_000_000)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--read-length", type=int, default=151)
    ap.add_argument("--rates", default="0.005,0.02")
    ap.add_argument("--min-solid", type=int, default=4)
    ap.add_argument("--sample", type=int, default=40, help="reads held against the restatement per rate and R")
    ap.add_argument("--parent-library", help="libmatchtigs.so of the parent commit, built aside")
    ap.add_argument("--work", help="directory for the prepared inputs (default: a temporary one)")
    ap.add_argument("--step-timeout", type=int, default=900, help="seconds a child may take")
    ap.add_argument("--step", choices=("prepare", "parent", "new"), help=argparse.SUPPRESS)
    ap.add_argument("--rep", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--out")
    args = ap.parse_args()
    args.rate_list = [float(x) for x in args.rates.split(",")]
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
                   "--length", str(args.length), "--k", str(args.k), "--device", str(args.device), "--work", work, "--rates", args.rates,
                   "--read-length", str(args.read_length), "--min-solid", str(args.min_solid), "--sample", str(args.sample)]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True)
            if r.returncode != 0:  # nothing more is started on the GPU
                sys.stderr.write(r.stderr[-4000:])
                raise SystemExit(f"step {step} (repetition {rep}) ended with status {r.returncode}")
            line = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")][-1]
            print(json.dumps(line), flush=True)
            return line

        doc = {"tool": "kmer_correct_timing", "length": args.length, "haplotypes": N_COLORS, "k": args.k, "read_length": args.read_length,
               "rates": args.rate_list, "min_solid": args.min_solid, "inputs": child("prepare")}
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
    for rate in args.rate_list:
        e = tag(rate)
        for f in PROBES + ("query_wall_ms",):
            s[f"{e}_{f}"] = spread(new, f"{e}_{f}")
            s[f"yardstick_{e}_{f}"] = spread(yard, f"{e}_{f}")
            s[f"{e}_{f}_over_yardstick"] = round(s[f"{e}_{f}"]["min"] / s[f"yardstick_{e}_{f}"]["min"], 4)
        if args.parent_library:  # untouched kernels: the best of this library's children is no slower than the parent's slowest
            for f in PROBES:
                checks[f"{e}_{f}_within_parent_spread"] = s[f"{e}_{f}"]["min"] <= s[f"yardstick_{e}_{f}"]["max"]
        checks[f"{e}_counts_equal_yardstick"] = all(r[f] == yard[0][f] for r in new + yard for f in (
            f"{e}_found", f"{e}_valid", f"{e}_runs", f"{e}_query_digest", f"{e}_counters_digest"))
        for R in ROUNDS:
            key = f"{e}_r{R}"
            for f in ("wall_ms", "kernels_ms", "upload_ms", "pack_ms", "query_ms", "flag_ms", "evaluate_ms", "apply_ms", "download_ms", "total_ms"):
                s[f"{key}_{f}"] = spread(new, f"{key}_{f}")
            for f in ("candidates", "candidates_per_read", "ambiguous", "round_corrected", "substitutions", "restored", "wrong", "errors_left",
                      "share_restored", "found", "found_after"):
                s[f"{key}_{f}"] = new[0][f"{key}_{f}"]
            s[f"{key}_kernels_over_query_probe"] = round(s[f"{key}_kernels_ms"]["min"] / s[f"yardstick_{e}_query_ms"]["min"], 4)
            s[f"{key}_wall_over_query_wall"] = round(s[f"{key}_wall_ms"]["min"] / s[f"yardstick_{e}_query_wall_ms"]["min"], 4)
            checks[f"{key}_same_in_every_child"] = len({r[f"{key}_digest"] for r in new}) == 1
            checks[f"{key}_sample_equals_restatement"] = all(r[f"{key}_sample_equals_restatement"] for r in new)
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
