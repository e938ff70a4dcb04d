"""fastq_timing.py -- what reading FASTQ on the GPU costs (api.read_fastq) next to the host FASTA reader.

Writes a synthetic read set -- reads of 151 bases from a genome of the project's sequence generator (synth.random_genome), either
case, one base in a thousand an `N`, qualities on a ramp from about 38 at the start of a read to about 24 at its end with noise --
as reads.fq, reads.fq.gz and its FASTA twin (the same reads as one-line records). Then, per repetition and in one process:
read_fastq on the plain file and on the .gz file with the six figures of mtg_last_fastq_times and the wall clock, at Q = 0 and
at --min-base-quality, and api.read_sequences(twin.fa, split_non_acgt=True) -- the host reader this repository had before the FASTQ
reader, unchanged by it; it reads half the bytes -- by the wall clock. The Q = 0 store is compared with the host reader's, byte for
byte. Recorded: the fastest repetition after the first of each, the plain call over the host reader, and the share of the .gz call
that is reading and inflating.

usage: python tools/fastq_timing.py [--reads 2000000] [--genome 10000000] [--min-base-quality 20] [--reps 3] [--device 0]
                                    [--dir DIR] [--out profiles/fastq_scan_2e6.json]"""
import argparse
import gzip
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

READ = 151


def write_read_set(directory: str, n_reads: int, genome_bases: int, seed: int = 5):
    """reads.fq, reads.fq.gz, twin.fa in `directory`; returns their paths and sizes."""
    from matchtigs_amd import synth

    rng = np.random.default_rng(seed)
    genome = np.frombuffer(synth.random_genome(genome_bases, seed=seed, haplotypes=1)[0].encode(), np.uint8)
    starts = rng.integers(0, genome_bases - READ + 1, n_reads)
    bases = genome[starts[:, None] + np.arange(READ)[None, :]]
    bases = np.where(rng.random(bases.shape, dtype=np.float32) < 0.001, np.uint8(ord("N")), bases)
    lower = rng.random(n_reads) < 0.02
    bases[lower] |= 0x20
    ramp = 38.0 - 14.0 * (np.arange(READ) / (READ - 1)) ** 2
    quals = np.clip(np.rint(ramp[None, :] + rng.normal(0.0, 4.0, bases.shape).astype(np.float32)), 2, 41).astype(np.uint8) + 33
    names = np.frombuffer(b"".join(b"r%09d" % i for i in range(n_reads)), np.uint8).reshape(n_reads, 10)
    nl = np.full((n_reads, 1), 0x0A, np.uint8)
    fq = np.concatenate([np.full((n_reads, 1), ord("@"), np.uint8), names, nl, bases, nl, np.full((n_reads, 1), ord("+"), np.uint8), nl, quals, nl],
                        axis=1)
    fa = np.concatenate([np.full((n_reads, 1), ord(">"), np.uint8), names, nl, bases, nl], axis=1)
    paths = {n: os.path.join(directory, n) for n in ("reads.fq", "reads.fq.gz", "twin.fa")}
    fq.tofile(paths["reads.fq"])
    fa.tofile(paths["twin.fa"])
    with gzip.open(paths["reads.fq.gz"], "wb", compresslevel=1) as f:
        f.write(fq.tobytes())
    return paths, {n: os.path.getsize(p) for n, p in paths.items()}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--genome", type=int, default=10_000_000)
    ap.add_argument("--min-base-quality", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--dir", help="where the read set is written (default: a temporary directory)")
    ap.add_argument("--out")
    args = ap.parse_args()

    from matchtigs_amd import _lib, api

    if _lib.load().mtg_device_count() < 1:
        raise SystemExit("fastq_timing needs a GPU: read_fastq has no CPU path")
    with tempfile.TemporaryDirectory(dir=args.dir) as d:
        t0 = time.perf_counter()
        paths, sizes = write_read_set(d, args.reads, args.genome)
        print(json.dumps({"written": sizes, "seconds": round(time.perf_counter() - t0, 1)}), flush=True)
        doc = {"tool": "fastq_timing", "reads": args.reads, "read_bases": READ, "genome": args.genome, "min_base_quality": args.min_base_quality,
               "file_bytes": sizes, "runs": []}
        host_store = None
        for rep in range(args.reps):  # the three readers take turns inside a repetition
            for what, name, q in (("host_fasta_twin", "twin.fa", None), ("fastq_plain", "reads.fq", 0),
                                  ("fastq_plain_q", "reads.fq", args.min_base_quality), ("fastq_gz", "reads.fq.gz", 0)):
                t0 = time.perf_counter()
                if q is None:
                    store = api.read_sequences(paths[name], split_non_acgt=True)
                    row = {"pieces": len(store), "pieces_cut": store.pieces_cut}
                else:
                    store, st = api.read_fastq(paths[name], q, args.device)
                    row = {**{f: round(v, 3) for f, v in api.last_fastq_times().items()}, "pieces": st.pieces, "pieces_cut": st.pieces_cut,
                           "bases_kept": st.bases_kept, "masked_bases": st.masked_bases}
                row = {"what": what, "rep": rep, "wall_ms": round(1e3 * (time.perf_counter() - t0), 3), **row}
                if rep == 0 and q is None:
                    host_store = store
                elif rep == 0 and q == 0:  # the contract: byte for byte the host reader's store
                    (d1, o1), (d2, o2) = store.arrays(), host_store.arrays()
                    row["equals_host_reader"] = bool(np.array_equal(d1, d2) and np.array_equal(o1, o2) and store.pieces_cut == host_store.pieces_cut)
                doc["runs"].append(row)
                print(json.dumps(row), flush=True)
                del store
        api.release_device_memory(args.device)

    def best(what):  # the first repetition also pays the arena's first chunk and the page cache
        rows = [r for r in doc["runs"] if r["what"] == what]
        return min(rows[1:] or rows, key=lambda r: r["wall_ms"])

    plain, gz, host = best("fastq_plain"), best("fastq_gz"), best("host_fasta_twin")
    doc["summary"] = {
        "fastq_plain": plain, "fastq_plain_q": best("fastq_plain_q"), "fastq_gz": gz, "host_fasta_twin_wall_ms": host["wall_ms"],
        "fastq_plain_over_host_twin": round(plain["wall_ms"] / host["wall_ms"], 3),
        "gz_read_and_inflate_share": round(gz["read_ms"] / gz["total_ms"], 3),
        "all_equal_host_reader": all(r["equals_host_reader"] for r in doc["runs"] if "equals_host_reader" in r),
    }
    print(json.dumps({"summary": doc["summary"]}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
