"""`python -m matchtigs_amd` -- the reference CLI's flag surface for the path this engine serves.

Flag names, defaults and exclusivity rules follow /root/reference/src/bin.rs:56-205, 850-862 for the subset that maps onto
the engine (the rest of the reference CLI -- GFA input, pathtigs -- is out of scope). Two inputs are served:
`--bcalm-in` (BCALM2/GGCAT FASTA whose `L:` annotations carry the links) and `--fa-in` (plain unitig FASTA, no topology: the
graph comes from the (k-1)-mer overlaps of the unitig ends, joined on the GPU). A third, `--seq-in` (not in the
reference), takes ANY sequences -- an assembly, haplotypes, another tool's tigs; `N` runs split records -- and compacts their k-mer
set into maximal unitigs on the GPU first, then goes the `--fa-in` way; `--unitigs-fa-out` writes the unitigs of
any input. All work happens inside
libmatchtigs.so; this file only parses flags and prints the reference's closing log line (bin.rs:1209-1211). `--verify` and
`--verify-fa` (not in the reference) check on the GPU that tigs spell exactly the input's k-mer set.
`--query-fa` with `--query-out` (not in the reference) asks, after the tig outputs, which k-mers of other sequences -- reads,
contigs, `N` and all -- are in the input's k-mer set: per record the windows, the valid ones (ACGT only) and those found, as a TSV,
and with `--query-presence-out` one `1` / `0` / `-` character per window; the set is indexed once on the GPU.
`--query-locate-out` adds where those k-mers are: one TSV row per maximal run of consecutive query k-mers that lie one after the
other in an input record, on either strand, with both half-open base intervals.
`--query-index minimizer` answers `--query-out` / `--query-presence-out` from a sparse minimizer index -- the packed bases plus one word
per minimizer anchor (`--query-minimizer-length M`) instead of a table slot per k-mer --, and `--query-index-over greedytigs` /
`eulertigs` indexes the tigs this run wrote instead of the input: the same answers from an index the size of the tigs.
`--query-index-locate-out` (with `--query-index minimizer`) writes `--query-locate-out`'s rows from that sparse index, at the coordinates
of whatever it indexes -- the input's records, or the records of the tig FASTA this run wrote.
`--query-index-abundance-out` (with `--query-index-abundance-profile-out`) and `--query-index-colors-out` write `--query-abundance-out`'s,
`--query-abundance-profile-out`'s and `--query-colors-out`'s files from that sparse index, byte for byte, whatever it indexes: the
weights and masks hang off the positions of its text, one per window, dense or as runs of equal values.
`--min-abundance N` (with `--seq-in`; not in the reference) keeps only the k-mers that at least N windows of the input show, on either
strand -- sequencing reads, where a k-mer seen once is mostly an error -- before the unitigs are formed;
`--kmer-spectrum-out` writes how many distinct k-mers have each abundance, `--unitig-abundance-out` the summed and mean abundance
of every unitig.
`--require-colors LIST`, `--forbid-colors LIST`, `--min-colors N`, `--max-colors N` (with `--seq-in`; not in the reference) select, at
the same place, the k-mers by the files that carry them (LIST: 0-based file numbers in `--seq-in` order, e.g. 0,2,5-7), and
`--subtract-fa F` / `--intersect-fa F` against the k-mers of other files, which are looked up on the GPU and never inserted: they add
no k-mer, count or colour. `--selection-out` says what each rule rejected.
`--query-abundance-out` (with `--seq-in` and `--query-fa`) reports how often the k-mers of each query record were seen in the input: the
index is weighted with the abundance of every kept k-mer, and a TSV row per query record gives the k-mers found and the sum, the
smallest, the largest and the mean of their abundances; `--query-abundance-profile-out` adds one abundance per k-mer of every
query record, and `--unitig-kmer-abundance-out` writes the abundance of every k-mer of every unitig.
`--seq-in` and `--query-fa` also take FASTQ reads (optionally `.gz`), told from FASTA by the first character of the content and read
on the GPU; `--seq-in` may be given several times (R1 / R2; FASTA and FASTQ may be mixed), the records of the files
follow each other in the order given. `--min-base-quality Q` treats a base of a `--seq-in` read whose Phred quality is below Q like
an `N`, so that it never reaches a k-mer; `--query-min-base-quality Q` does the same to the `--query-fa` reads.
With several `--seq-in` files every file is a COLOUR (a sample, a haplotype; at most 64), in the order given, and every k-mer knows which
files show it, on either strand: `--color-matrix-out` writes how many k-mers each file has and each pair of files
shares, `--unitig-colors-out` the colours along every unitig as runs `count:hexmask` (bit i = file i), and `--query-colors-out` (with
`--query-fa`) per query record how many of its k-mers each file carries.
`--monochromatic-unitigs` cuts the unitigs wherever the set of files changes, so that every k-mer of a unitig is carried by the same
files; `--color-classes-out` writes the distinct sets of files (the colour classes, numbered in the order the unitigs show them) with
their k-mers and runs, and `--unitig-color-classes-out` the classes along every unitig as runs `count:class`.
`--clip-tips L` (with `--seq-in`; not in the reference) removes the tips -- dead-end unitigs of fewer than L k-mers that hang off a fork,
what a sequencing error near a read end leaves behind even above `--min-abundance` -- and `--remove-isolated L` the unitigs of fewer
than L k-mers that touch nothing, both inside the GPU compaction and before the unitigs are formed for good; `--clean-rounds R`
repeats that up to R times on the unitigs the round before left. Every output sees the cleaned unitigs.
`--pop-bubbles L` (with `--seq-in`) pops simple bubbles in the same rounds: of the unitigs of fewer than L k-mers that join the same
two nodes -- what a sequencing error in the middle of a read seen twice, or a heterozygous SNP, leaves -- the one with the largest
mean abundance stays; a SNP's arms have k k-mers, so L = k + 1 is the least that pops them and 2 k the usual value. `--bubble-ratio R`
pops an arm only if the best has at least R times its mean abundance, which keeps variation between samples.
`--unitigs-bcalm-out` and `--unitigs-gfa-out` (any input; not in the reference) write the unitigs WITH their links, beside
`--unitigs-fa-out` and before the tig algorithms: as BCALM2/GGCAT FASTA (`>id LN:i: KC:i: km:f: L:+:id:-`, what `--bcalm-in` reads) and
as GFA1 (`S` and `L` lines with a k-1 overlap). The link lists and the whole text are made on the GPU; `KC` is the summed abundance of
the unitig's k-mers where the compaction counted them, else their number.
`--components-out` and `--unitig-components-out` (any input; not in the reference) describe how that graph falls apart: one TSV row
per connected component over the links -- unitigs, k-mers, bases, abundance, links, dead ends, whether it is a closed ring -- and
the component of every unitig, line i for record i of `--unitigs-fa-out`; the labels and the sums are made on the GPU without the
link lists. `--min-component-kmers N` (`--seq-in`, `--fa-in`) removes every component of fewer than N k-mers -- the clusters of two
or three short unitigs that are neither tip nor isolated nor bubble -- once, before `--verify` and every output; links exist only
inside a component, so what stays is still maximal and nothing is compacted again.
`--bubbles-out` (`--seq-in`, `--fa-in`; not in the reference) says what the variation is that the cleaning left: every bubble of that
graph -- two or more unitigs of fewer than `--bubbles-max-kmers` (default 2 k) k-mers between the same two nodes -- is a site, the arm
with the largest mean abundance its reference allele, and the TSV gets one row per arm with its unitig and strand, k-mers, abundance,
the kind of the difference (snp, mnp, ins, del, complex), its 0-based position on the reference arm's record, both alleles
(left-aligned, `-` for none) and, with several `--seq-in` files, how many of the arm's k-mers each file carries.
`--count-fa` with `--count-out` (any input; not in the reference) asks the opposite of `--query-fa`: how much of the input's k-mer set
did OTHER reads see? Every `--count-fa` file is a sample (FASTA or FASTQ, `.gz` or not, told apart by the content); its k-mers are
counted on the k-mers of the unitigs -- as written, after cleaning, splitting and the component filter -- on the GPU, either strand,
repeats included, and `--count-out` gets one row per unitig with, per sample, the k-mers of the unitig the sample saw at all and the sum
of their counts: a unitig x sample depth matrix of exact integers. `--count-min-base-quality Q` masks the bases of FASTQ count files
whose Phred quality is below Q.
`--count-index minimizer` counts on the sparse minimizer index instead of the table (`--count-minimizer-length M`), with one counter per
window of the indexed text, and `--count-index-over greedytigs` / `eulertigs` indexes the tigs this run wrote: `--count-out` is byte for
byte the table route's. Queries that asked the same sparse index hand it over.
`--pseudoalign-fa` (with several `--seq-in` files as colours; not in the reference) pseudoaligns reads to the coloured k-mer set: every
file is a sample, `--pseudoalign-mate-fa` its second mates, and per fragment the files whose k-mers cover at least
`--pseudoalign-threshold` of its found (`--pseudoalign-over valid`: valid) k-mers are its colours -- at the default 1, the
intersection of the colour sets of its found k-mers. `--pseudoalign-out` gets one row per fragment, `--pseudoalign-classes-out` the
distinct colour sets of each sample with their fragments (the equivalence classes) and `--pseudoalign-summary-out` per colour the
fragments assigned to it and to it alone. The per-colour counters never leave the GPU; `--pseudoalign-index minimizer` aligns on the
sparse index with the same files, byte for byte.
`--correct-fa` (not in the reference) corrects the substitution errors of reads against the k-mers of the run's unitigs, after all
cleaning: a base that no k-mer of the set covers is replaced by the one base that makes at least `--correct-min-solid` of its covering
k-mers solid, in `--correct-rounds` rounds on the GPU. `--correct-out` is the file with exactly those bytes replaced -- headers, line
wrapping, qualities and line ends as they were -- and `--correct-report-out` one row per read with its substitutions.
`--index-out PATH` (not in the reference) saves a locating sparse minimizer index -- over the input or, with `--index-over`, over the
tigs this run wrote; with `--index-weights` / `--index-colors` the abundances and the colours of the `--seq-in` files hang off it -- as
one file, and `--index-in PATH` is a fifth kind of input: a run on such a file reads no sequences of the indexed set, compacts nothing
and answers `--query-fa` and `--pseudoalign-fa` byte for byte as the building run did. `--index-info PATH` prints the file's header and
metadata without a GPU.
`--thread-fa` (not in the reference) threads reads, genes or haplotypes through the unitig graph: over the unitigs every k-mer has one
place, so the located runs of a record, joined wherever one ends at a unitig's end and the next starts at another's start, are the
segments of its path. `--thread-gaf-out` gets one GAF line per maximal walk -- the `>`/`<` oriented `S` names of `--unitigs-gfa-out`,
the path's length and the exact interval on it, a walk may start and end inside a segment -- and `--thread-report-out` one row per
read; a read with an error k-mer the cleaning removed is broken exactly there. `--thread-min-kmers N` drops shorter walks,
`--thread-index minimizer` threads on the sparse index with the same files, and with `--index-in` the walks run over the records of
whatever the file indexed, where repeated k-mers (tigs) only shorten them.
"""
from __future__ import annotations

import argparse
import sys
import time


MAX_COLORS = 64  # the colours of one call: the bits of a mask


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="matchtigs_amd", description=__doc__.split("\n\n")[0])
    ap.add_argument("--bcalm-in", help="bcalm2/GGCAT unitig fasta (optionally .gz); requires -k (bin.rs:76-83)")
    ap.add_argument("--gfa-in", help="(not served by this engine)")
    ap.add_argument("--fa-in", help="plain unitig fasta (optionally .gz), graph from (k-1)-mer overlaps on the GPU; requires -k (bin.rs:71-75)")
    ap.add_argument("--seq-in", action="append", metavar="PATH",
                    help="any sequences as fasta or fastq (optionally .gz; non-ACGT runs split records): their k-mer set is compacted "
                         "into maximal unitigs on the GPU, then as --fa-in; repeatable; requires -k (not in the reference)")
    ap.add_argument("--min-base-quality", type=int, metavar="Q",
                    help="with fastq --seq-in files: a base whose Phred quality is below Q (0..93) splits a read like an N "
                         "(not in the reference)")
    ap.add_argument("--query-min-base-quality", type=int, metavar="Q",
                    help="with fastq --query-fa files: a base whose Phred quality is below Q (0..93) is replaced by N")
    ap.add_argument("--unitigs-fa-out", help="write the input's unitigs as fasta (.gz => gzip): with --seq-in, the GPU compactor's output "
                                             "(not in the reference)")
    ap.add_argument("--unitigs-bcalm-out", metavar="PATH",
                    help="write the input's unitigs with their links as bcalm2/GGCAT fasta, `>id LN:i: KC:i: km:f: L:+:id:-` "
                         "(.gz => gzip), the format --bcalm-in reads (not in the reference)")
    ap.add_argument("--unitigs-gfa-out", metavar="PATH",
                    help="write the input's unitigs with their links as GFA1: S lines with LN, KC and km tags, L lines with a k-1 "
                         "overlap (.gz => gzip) (not in the reference)")
    ap.add_argument("--components-out", metavar="PATH",
                    help="write one TSV row per connected component of the unitig graph over its links: component, first_unitig, "
                         "unitigs, kmers, bases, abundance, mean, links, dead_ends, circular (.gz => gzip) (not in the reference)")
    ap.add_argument("--unitig-components-out", metavar="PATH",
                    help="write the component of every unitig, line i for record i of --unitigs-fa-out (.gz => gzip) (not in the reference)")
    ap.add_argument("--min-component-kmers", type=int, metavar="N",
                    help="with --seq-in or --fa-in: remove the connected components of fewer than N k-mers before --verify and every "
                         "output (not in the reference)")
    ap.add_argument("--bubbles-out", metavar="PATH",
                    help="with --seq-in or --fa-in: write the bubbles of the unitig graph as variant calls, one TSV row per arm: bubble, "
                         "arm, unitig, strand, kmers, abundance, mean, type, pos, ref, alt, differences and, with several --seq-in files, "
                         "the k-mers of the arm each file carries (.gz => gzip) (not in the reference)")
    ap.add_argument("--bubbles-max-kmers", type=int, metavar="L",
                    help="with --bubbles-out: an arm has fewer than L k-mers (default 2 k; at least 2)")
    ap.add_argument("-k", type=int, help="k-mer size used to build the de Bruijn graph (bin.rs:139-141)")
    ap.add_argument("-t", "--threads", type=int, default=1, help="accepted; results always equal the 1-thread order (bin.rs:148-149)")
    ap.add_argument("--greedytigs-fa-out", help="write greedy matchtigs as fasta (.gz => gzip) (bin.rs:107-109)")
    ap.add_argument("--eulertigs-fa-out", help="write eulertigs as fasta (bin.rs:99-101)")
    ap.add_argument("--greedytigs-gfa-out", help="write greedy matchtigs as GFA (bin.rs:107-109, 667-818)")
    ap.add_argument("--eulertigs-gfa-out", help="write eulertigs as GFA (bin.rs:97-99)")
    ap.add_argument("--greedytigs-duplication-bitvector-out",
                    help="per greedy matchtig a line of 1 (original k-mer) / 0 (duplicate) characters (bin.rs:129-132)")
    ap.add_argument("--matchtigs-fa-out", help="write optimal matchtigs as fasta; needs the external matcher (bin.rs:123-125)")
    ap.add_argument("--matchtigs-gfa-out", help="write optimal matchtigs as GFA (bin.rs:117-119)")
    ap.add_argument("--matchtigs-duplication-bitvector-out", help="duplication bitvector of the optimal matchtigs")
    ap.add_argument("--blossom5-command", default="blossom5", help="the command used to run blossom5 (bin.rs:151-153)")
    ap.add_argument("--compression-level", type=int, default=6, help="0-9 (bin.rs:203-218)")
    ap.add_argument("--device", type=int, default=0, help="GPU ordinal (not in the reference)")
    ap.add_argument("--verify", action="store_true",
                    help="after writing, check on the GPU that each algorithm's tigs spell exactly the input's k-mer set; exit 1 if not "
                         "(not in the reference)")
    ap.add_argument("--verify-fa", action="append", metavar="PATH",
                    help="check an existing tig fasta (optionally .gz) against the input's k-mer set; repeatable; computes nothing "
                         "(not in the reference)")
    ap.add_argument("--query-fa", action="append", metavar="PATH",
                    help="sequences (fasta, optionally .gz; any characters) whose k-mers are looked up in the input's k-mer set on the "
                         "GPU; repeatable; needs --query-out (not in the reference)")
    ap.add_argument("--query-out", metavar="PATH",
                    help="TSV (.gz => gzip) with one row per record of the --query-fa files: record, length, kmers, valid, found")
    ap.add_argument("--query-presence-out", metavar="PATH",
                    help="per query record a line with one character per k-mer: 1 in the set, 0 not, - holds a non-ACGT character (.gz => gzip)")
    ap.add_argument("--query-locate-out", metavar="PATH",
                    help="TSV (.gz => gzip) with one row per maximal collinear run of found k-mers: record, qstart, qend, strand, target "
                         "(0-based input record), tstart, tend, kmers; a repeated k-mer is placed at its first occurrence; "
                         "needs --query-fa and --query-out")
    ap.add_argument("--query-index", choices=("table", "minimizer"),
                    help="the index --query-fa asks: table (default; a slot per k-mer) or minimizer (the packed bases plus one word per "
                         "minimizer anchor: a fraction of the memory, the same answers; serves --query-out and --query-presence-out)")
    ap.add_argument("--query-index-locate-out", metavar="PATH",
                    help="with --query-index minimizer: --query-locate-out's TSV (.gz => gzip) from the sparse index; target is the 0-based "
                         "record of what --query-index-over names (the input, or the tig FASTA this run wrote); needs --query-fa and "
                         "--query-out")
    ap.add_argument("--query-index-abundance-out", metavar="PATH",
                    help="with --query-index minimizer and --seq-in: --query-abundance-out's TSV (.gz => gzip) from the sparse index, over "
                         "whatever --query-index-over names; needs --query-fa and --query-out")
    ap.add_argument("--query-index-abundance-profile-out", metavar="PATH",
                    help="with --query-index-abundance-out: --query-abundance-profile-out's lines (.gz => gzip) from the sparse index")
    ap.add_argument("--query-index-colors-out", metavar="PATH",
                    help="with --query-index minimizer and --seq-in: --query-colors-out's TSV (.gz => gzip) from the sparse index, over "
                         "whatever --query-index-over names; needs --query-fa and --query-out")
    ap.add_argument("--query-minimizer-length", type=int, metavar="M",
                    help="with --query-index minimizer: the minimizer length, 1 .. min(k, 31) (default min(19, ceil(2k/3)))")
    ap.add_argument("--query-index-over", choices=("input", "greedytigs", "eulertigs"),
                    help="the sequences --query-fa indexes: the input (default) or the tigs this run wrote, read back from "
                         "--greedytigs-fa-out / --eulertigs-fa-out; they spell the same k-mer set")
    ap.add_argument("--min-abundance", type=int, metavar="N",
                    help="with --seq-in: compact only the k-mers seen in at least N windows of the input, both strands counted "
                         "(N >= 1; not in the reference)")
    ap.add_argument("--kmer-spectrum-out", metavar="PATH",
                    help="with --seq-in: TSV (.gz => gzip) abundance, kmers: the distinct k-mers of the input per abundance, before "
                         "the filter; the last bin is 255+")
    ap.add_argument("--unitig-abundance-out", metavar="PATH",
                    help="with --seq-in: TSV (.gz => gzip) unitig, kmers, abundance, mean: per record of --unitigs-fa-out (0-based) "
                         "its k-mers, the sum of their abundances and the mean")
    ap.add_argument("--query-abundance-out", metavar="PATH",
                    help="with --seq-in, --query-fa and --query-out: TSV (.gz => gzip) with one row per query record: record, kmers, "
                         "valid, found, then sum, min, max and mean of the input abundances of its found k-mers (mean `-` if none)")
    ap.add_argument("--query-abundance-profile-out", metavar="PATH",
                    help="per query record a line with one integer per k-mer: its abundance in the input, 0 not in the set, - holds a "
                         "non-ACGT character (.gz => gzip); needs --query-abundance-out")
    ap.add_argument("--unitig-kmer-abundance-out", metavar="PATH",
                    help="with --seq-in: per record of --unitigs-fa-out a line with the abundance of each of its k-mers (.gz => gzip)")
    ap.add_argument("--color-matrix-out", metavar="PATH",
                    help="with --seq-in, each file one colour (at most 64): TSV (.gz => gzip) color, kmers, then one column per file: "
                         "the k-mers of file i and those it shares with every file; a closing row #occupancy: the k-mers carried by "
                         "exactly 1, 2, ... files (not in the reference)")
    ap.add_argument("--unitig-colors-out", metavar="PATH",
                    help="with --seq-in: per record of --unitigs-fa-out a line of runs count:hexmask over its k-mers, left to right; "
                         "bit i of a mask = --seq-in file i (.gz => gzip)")
    ap.add_argument("--query-colors-out", metavar="PATH",
                    help="with --seq-in, --query-fa and --query-out: TSV (.gz => gzip) with one row per query record: record, kmers, "
                         "valid, found, then per --seq-in file the found k-mers that file carries")
    ap.add_argument("--monochromatic-unitigs", action="store_true",
                    help="with --seq-in, each file one colour: cut the unitigs wherever the set of files that carry the k-mers changes; "
                         "every output then sees the split unitigs (not in the reference)")
    ap.add_argument("--color-classes-out", metavar="PATH",
                    help="with --seq-in: TSV (.gz => gzip) class, mask, carriers, kmers, runs: one row per distinct set of files, numbered "
                         "in the order the unitigs show them; mask as in --unitig-colors-out, carriers its files")
    ap.add_argument("--unitig-color-classes-out", metavar="PATH",
                    help="with --seq-in: per record of --unitigs-fa-out a line of runs count:class over its k-mers, left to right; the "
                         "classes are those of --color-classes-out (.gz => gzip)")
    ap.add_argument("--clip-tips", type=int, metavar="L",
                    help="with --seq-in: remove the dead-end unitigs of fewer than L k-mers that hang off a fork (L >= 2; the "
                         "conventional value is k; not in the reference)")
    ap.add_argument("--remove-isolated", type=int, metavar="L",
                    help="with --seq-in: remove the unitigs of fewer than L k-mers with two dead ends (L >= 1)")
    ap.add_argument("--clean-rounds", type=int, metavar="R",
                    help="with --clip-tips / --remove-isolated / --pop-bubbles: at most R rounds (1..64, default 1), each on the unitigs the "
                         "one before left")
    ap.add_argument("--pop-bubbles", type=int, metavar="L",
                    help="with --seq-in: of the unitigs of fewer than L k-mers between the same two nodes keep the one with the largest mean "
                         "abundance (L >= 2; k + 1 is the least that pops a SNP, 2 k the usual value; not in the reference)")
    ap.add_argument("--bubble-ratio", type=int, metavar="R",
                    help="with --pop-bubbles: pop an arm only if the best arm has at least R times its mean abundance (1..255, default 1)")
    ap.add_argument("--require-colors", metavar="LIST",
                    help="with --seq-in: keep only the k-mers that every file of LIST carries; LIST holds 0-based file numbers in "
                         "--seq-in order as commas and ranges, e.g. 0,2,5-7 (not in the reference)")
    ap.add_argument("--forbid-colors", metavar="LIST", help="with --seq-in: drop the k-mers that a file of LIST carries")
    ap.add_argument("--min-colors", type=int, metavar="N",
                    help="with --seq-in: keep only the k-mers that at least N files carry (N = the number of files: the core)")
    ap.add_argument("--max-colors", type=int, metavar="N", help="with --seq-in: keep only the k-mers that at most N files carry (1: the private ones)")
    ap.add_argument("--subtract-fa", action="append", metavar="PATH",
                    help="with --seq-in: drop the k-mers that the sequences of this file show (fasta or fastq, optionally .gz; either "
                         "strand); the file is looked up, never inserted: it adds no k-mer, count or colour; repeatable (not in the reference)")
    ap.add_argument("--subtract-min-abundance", type=int, metavar="A",
                    help="with --subtract-fa: drop a k-mer only if the files show it at least A times (default 1)")
    ap.add_argument("--intersect-fa", action="append", metavar="PATH",
                    help="with --seq-in: keep only the k-mers that the sequences of these files show; repeatable, all files form one set")
    ap.add_argument("--intersect-min-abundance", type=int, metavar="B",
                    help="with --intersect-fa: keep a k-mer only if the files show it at least B times (default 1)")
    ap.add_argument("--filter-min-base-quality", type=int, metavar="Q",
                    help="with fastq --subtract-fa / --intersect-fa files: a base whose Phred quality is below Q (0..93) splits a read like an N")
    ap.add_argument("--selection-out", metavar="PATH",
                    help="TSV (.gz => gzip): name<TAB>k-mers for input, abundance_kept, the k-mers each selection rule rejected (forbid, "
                         "require, carriers, subtract, intersect) and selected; then per file color<TAB>file<TAB>k-mers<TAB>selected")
    ap.add_argument("--count-fa", action="append", metavar="PATH",
                    help="reads of one sample (fasta or fastq, optionally .gz; any characters) whose k-mers are counted on the k-mers of "
                         "the input's unitigs on the GPU; repeatable, one sample per file; needs --count-out (not in the reference)")
    ap.add_argument("--count-out", metavar="PATH",
                    help="TSV (.gz => gzip) with one row per record of --unitigs-fa-out (0-based): unitig, kmers, then per --count-fa "
                         "file <file>:covered (its k-mers the file saw) and <file>:sum (the sum of their counts)")
    ap.add_argument("--count-min-base-quality", type=int, metavar="Q",
                    help="with fastq --count-fa files: a base whose Phred quality is below Q (0..93) is replaced by N")
    ap.add_argument("--count-index", choices=("table", "minimizer"),
                    help="the index --count-fa counts on: table (default; a slot and a counter per k-mer) or minimizer (the sparse index "
                         "with a counter per window of its text: a fraction of the memory, the same --count-out)")
    ap.add_argument("--count-minimizer-length", type=int, metavar="M",
                    help="with --count-index minimizer: the minimizer length, 1 .. min(k, 31) (default min(19, ceil(2k/3)))")
    ap.add_argument("--count-index-over", choices=("input", "greedytigs", "eulertigs"),
                    help="with --count-index minimizer: the sequences --count-fa indexes: the input (default) or the tigs this run wrote, "
                         "read back from --greedytigs-fa-out / --eulertigs-fa-out; --count-out keeps one row per unitig")
    ap.add_argument("--pseudoalign-fa", action="append", metavar="PATH",
                    help="reads of one sample (fasta or fastq, optionally .gz; any characters) that are pseudoaligned to the colours, the "
                         "--seq-in files, on the GPU; repeatable, one sample per file; needs --seq-in and one of the three "
                         "--pseudoalign-*-out (not in the reference)")
    ap.add_argument("--pseudoalign-mate-fa", action="append", metavar="PATH",
                    help="the second mates of the i-th --pseudoalign-fa file, record by record: a pair is one fragment; none, or as many "
                         "as --pseudoalign-fa")
    ap.add_argument("--pseudoalign-out", metavar="PATH",
                    help="TSV (.gz => gzip) with one row per fragment of all samples: record (the first mate's name), kmers, valid, found, "
                         "colors (the 0-based --seq-in files assigned, ascending, comma separated; - for none)")
    ap.add_argument("--pseudoalign-classes-out", metavar="PATH",
                    help="TSV (.gz => gzip) sample, class, mask, carriers, fragments: per sample its distinct colour sets, numbered from 0 "
                         "by their first fragment; mask as in --color-classes-out")
    ap.add_argument("--pseudoalign-summary-out", metavar="PATH",
                    help="TSV (.gz => gzip) with one row per colour: color, then per sample <sample>:assigned and <sample>:unique; closing "
                         "rows #fragments, #eligible, #assigned, #ambiguous: a sample's total under :assigned, - under :unique")
    ap.add_argument("--pseudoalign-threshold", metavar="T",
                    help="the share of a fragment's k-mers a colour must carry: a decimal in (0, 1] with at most three places (default 1)")
    ap.add_argument("--pseudoalign-over", choices=("found", "valid"),
                    help="the k-mers the threshold is a share of: those found in the set (default) or all valid ones")
    ap.add_argument("--pseudoalign-min-kmers", type=int, metavar="N",
                    help="a fragment with fewer than N such k-mers gets no colour (N >= 1, default 1)")
    ap.add_argument("--pseudoalign-min-base-quality", type=int, metavar="Q",
                    help="with fastq --pseudoalign-fa / --pseudoalign-mate-fa files: a base whose Phred quality is below Q (0..93) is "
                         "replaced by N")
    ap.add_argument("--pseudoalign-index", choices=("table", "minimizer"),
                    help="the index the reads are aligned on: table (default) or minimizer (the sparse index with the masks by position: "
                         "the same files)")
    ap.add_argument("--pseudoalign-minimizer-length", type=int, metavar="M",
                    help="with --pseudoalign-index minimizer: the minimizer length, 1 .. min(k, 31) (default min(19, ceil(2k/3)))")
    ap.add_argument("--correct-fa", action="append", metavar="PATH",
                    help="reads (fasta or fastq, optionally .gz; any characters) whose substitution errors are corrected on the GPU against "
                         "the k-mers of the run's unitigs, after all cleaning; repeatable; needs --correct-out or --correct-report-out "
                         "(not in the reference)")
    ap.add_argument("--correct-out", action="append", metavar="PATH",
                    help="the i-th --correct-fa file's text with exactly the substituted bytes replaced (.gz => gzip): none, or one per "
                         "--correct-fa, in order")
    ap.add_argument("--correct-report-out", metavar="PATH",
                    help="TSV (.gz => gzip) with one row per read of all --correct-fa files: file, record, length, kmers, valid, found, "
                         "found_after, candidates, ambiguous, corrected, corrections (pos:X>Y,... with 0-based positions, ascending; - for none)")
    ap.add_argument("--correct-min-solid", type=int, metavar="W",
                    help="a substitution must make at least min(W, the valid k-mers that cover the base) of them solid (W >= 1, default 4)")
    ap.add_argument("--correct-rounds", type=int, metavar="R", help="rounds of correction, each on the text the one before left (1..8, default 2)")
    ap.add_argument("--thread-fa", action="append", metavar="PATH",
                    help="reads, genes or haplotypes (fasta or fastq, optionally .gz; any characters) that are threaded through the "
                         "unitig graph on the GPU: every maximal walk their k-mers take over the unitigs as written; repeatable; needs "
                         "--thread-gaf-out or --thread-report-out (not in the reference)")
    ap.add_argument("--thread-gaf-out", metavar="PATH",
                    help="GAF (.gz => gzip) with one line per walk of all --thread-fa files, in file and query order: the path over the "
                         "segments of --unitigs-gfa-out, exact, with cg:Z: and km:i: (the walk's k-mers)")
    ap.add_argument("--thread-report-out", metavar="PATH",
                    help="TSV (.gz => gzip) with one row per read of all --thread-fa files: file, record, length, kmers, valid, found, "
                         "walks, steps, longest (the most k-mers of one of its walks)")
    ap.add_argument("--thread-min-kmers", type=int, metavar="N", help="drop walks of fewer than N k-mers (N >= 1, default 1)")
    ap.add_argument("--thread-min-base-quality", type=int, metavar="Q",
                    help="with fastq --thread-fa files: a base whose Phred quality is below Q (0..93) is replaced by N")
    ap.add_argument("--thread-index", choices=("table", "minimizer"),
                    help="the locating index the reads are threaded on: table (default) or minimizer (the sparse index: the same files)")
    ap.add_argument("--thread-minimizer-length", type=int, metavar="M",
                    help="with --thread-index minimizer: the minimizer length, 1 .. min(k, 31) (default min(19, ceil(2k/3)))")
    ap.add_argument("--index-out", metavar="PATH",
                    help="after the tig outputs: build a locating sparse minimizer index and save it as one file (conventional suffix "
                         ".mtgx) that --index-in reopens (not in the reference)")
    ap.add_argument("--index-over", choices=("input", "greedytigs", "eulertigs"),
                    help="with --index-out: the sequences it indexes: the input (default) or the tigs this run wrote, read back from "
                         "--greedytigs-fa-out / --eulertigs-fa-out")
    ap.add_argument("--index-minimizer-length", type=int, metavar="M",
                    help="with --index-out: the minimizer length, 1 .. min(k, 31) (default min(19, ceil(2k/3)))")
    ap.add_argument("--index-weights", action="store_true", help="with --index-out and --seq-in: the file also keeps the abundance of every k-mer")
    ap.add_argument("--index-colors", action="store_true",
                    help="with --index-out and --seq-in: the file also keeps which --seq-in files carry every k-mer (at most 64 files)")
    ap.add_argument("--index-in", metavar="PATH",
                    help="an index file written by --index-out, instead of sequences: serves --query-fa with --query-out, "
                         "--query-presence-out, --query-index-locate-out, on a weighted file --query-index-abundance-out, on a coloured "
                         "one --query-index-colors-out and --pseudoalign-fa; -k is the file's (not in the reference)")
    ap.add_argument("--index-info", metavar="PATH",
                    help="print the header fields and the metadata of an index file as key<TAB>value lines and exit; needs no other "
                         "input and no GPU; exit 2 if the header is refused")
    args = ap.parse_args(argv)

    if args.index_info is not None:
        return _index_info(args.index_info)
    if args.index_in is not None:
        return _main_index_in(ap, args)
    for flag, value in (("--index-over", args.index_over), ("--index-minimizer-length", args.index_minimizer_length),
                        ("--index-weights", args.index_weights or None), ("--index-colors", args.index_colors or None)):
        if value is not None and not args.index_out:
            ap.error(f"{flag} needs --index-out")
    for flag, value in (("--index-weights", args.index_weights), ("--index-colors", args.index_colors)):
        if value and args.seq_in is None:
            ap.error(f"{flag} needs --seq-in")
    for over, out in (("greedytigs", args.greedytigs_fa_out), ("eulertigs", args.eulertigs_fa_out)):
        if args.index_over == over and not out:
            ap.error(f"--index-over {over} needs --{over}-fa-out")

    classed = bool(args.monochromatic_unitigs or args.color_classes_out or args.unitig_color_classes_out)
    colored = bool(args.color_matrix_out or args.unitig_colors_out or args.query_colors_out or args.query_index_colors_out or classed
                   or args.pseudoalign_fa or args.index_colors or _selects_by_color(args) or args.bubbles_out is not None)
    if colored and args.seq_in is not None and len(args.seq_in) > MAX_COLORS:
        ap.error(f"{len(args.seq_in)} --seq-in files: at most {MAX_COLORS} files can be told apart as colours")

    n_inputs = sum(x is not None for x in (args.bcalm_in, args.gfa_in, args.fa_in, args.seq_in))
    if n_inputs == 0:  # bin.rs:855-858
        ap.error("Missing input argument. Specify exactly least one of --fa-in, --gfa-in or --bcalm-in")
    if n_inputs > 1:  # bin.rs:860-862
        ap.error("Too many input arguments. Specify exactly least one of --fa-in, --gfa-in or --bcalm-in")
    if args.gfa_in is not None:
        ap.error("only --bcalm-in and --fa-in are served by the MI355X engine (SURVEY.md 8 f-2)")
    if args.k is None:
        ap.error("--bcalm-in requires -k" if args.bcalm_in is not None else
                 "--seq-in requires -k" if args.seq_in is not None else "--fa-in requires -k")
    if not 0 <= args.compression_level <= 9:
        ap.error("compression level must be in 0..9")
    if args.matchtigs_duplication_bitvector_out and not (args.matchtigs_fa_out or args.matchtigs_gfa_out):
        ap.error("--matchtigs-duplication-bitvector-out needs --matchtigs-fa-out or --matchtigs-gfa-out (bin.rs:955-957)")
    if args.query_locate_out and not (args.query_fa and args.query_out):
        ap.error("--query-locate-out needs --query-fa and --query-out")
    if args.query_index_locate_out:
        if not args.query_fa:
            ap.error("--query-index-locate-out needs --query-fa")
        if not args.query_out:
            ap.error("--query-index-locate-out needs --query-out")
        if args.query_index != "minimizer":
            ap.error("--query-index-locate-out needs --query-index minimizer (the table index writes --query-locate-out)")
    if args.query_index_abundance_profile_out and not args.query_index_abundance_out:
        ap.error("--query-index-abundance-profile-out needs --query-index-abundance-out")
    for flag, value, table_flag in (("--query-index-abundance-out", args.query_index_abundance_out, "--query-abundance-out"),
                                    ("--query-index-colors-out", args.query_index_colors_out, "--query-colors-out")):
        if not value:
            continue
        if not args.seq_in:
            ap.error(f"{flag} needs --seq-in")
        if not args.query_fa:
            ap.error(f"{flag} needs --query-fa")
        if not args.query_out:
            ap.error(f"{flag} needs --query-out")
        if args.query_index != "minimizer":
            ap.error(f"{flag} needs --query-index minimizer (the table index writes {table_flag})")
    if bool(args.query_fa) != bool(args.query_out):
        ap.error("--query-fa needs --query-out" if args.query_fa else "--query-out needs --query-fa")
    if args.query_presence_out and not args.query_fa:
        ap.error("--query-presence-out needs --query-fa and --query-out")
    if args.query_abundance_out and not (args.seq_in and args.query_fa and args.query_out):
        ap.error("--query-abundance-out needs --seq-in, --query-fa and --query-out")
    if args.query_abundance_profile_out and not args.query_abundance_out:
        ap.error("--query-abundance-profile-out needs --query-abundance-out")
    if args.query_colors_out and not (args.seq_in and args.query_fa and args.query_out):
        ap.error("--query-colors-out needs --seq-in, --query-fa and --query-out")
    if bool(args.count_fa) != bool(args.count_out):
        ap.error("--count-fa needs --count-out" if args.count_fa else "--count-out needs --count-fa")
    if args.count_min_base_quality is not None and not args.count_fa:
        ap.error("--count-min-base-quality needs --count-fa")
    if args.count_index is not None and not args.count_fa:
        ap.error("--count-index needs --count-fa")
    for flag, value in (("--count-minimizer-length", args.count_minimizer_length), ("--count-index-over", args.count_index_over)):
        if value is not None and args.count_index != "minimizer":
            ap.error(f"{flag} needs --count-index minimizer")
    if args.count_minimizer_length is not None and not 1 <= args.count_minimizer_length <= min(args.k, 31):
        ap.error(f"--count-minimizer-length must be in 1..{min(args.k, 31)} (1 .. min(k, 31), as --query-minimizer-length)")
    _check_pseudoalign(ap, args)
    if args.correct_fa:
        if not (args.correct_out or args.correct_report_out):
            ap.error("--correct-fa needs --correct-out or --correct-report-out")
        if args.correct_out and len(args.correct_out) != len(args.correct_fa):
            ap.error(f"{len(args.correct_out)} --correct-out files for {len(args.correct_fa)} --correct-fa files: give none, or one per "
                     "--correct-fa, in order")
        if args.correct_min_solid is not None and not 1 <= args.correct_min_solid < 1 << 32:
            ap.error("--correct-min-solid must be >= 1")
        if args.correct_rounds is not None and not 1 <= args.correct_rounds <= 8:
            ap.error("--correct-rounds must be in 1..8")
    else:
        for flag, value in (("--correct-out", args.correct_out), ("--correct-report-out", args.correct_report_out),
                            ("--correct-min-solid", args.correct_min_solid), ("--correct-rounds", args.correct_rounds)):
            if value is not None:
                ap.error(f"{flag} needs --correct-fa")
    _check_thread(ap, args)
    if args.thread_minimizer_length is not None and not 1 <= args.thread_minimizer_length <= min(args.k, 31):
        ap.error(f"--thread-minimizer-length must be in 1..{min(args.k, 31)} (1 .. min(k, 31), as --query-minimizer-length)")
    for over, out in (("greedytigs", args.greedytigs_fa_out), ("eulertigs", args.eulertigs_fa_out)):
        if args.count_index_over == over and not out:
            ap.error(f"--count-index-over {over} needs --{over}-fa-out")
    for flag, value in (("--query-index", args.query_index), ("--query-minimizer-length", args.query_minimizer_length),
                        ("--query-index-over", args.query_index_over)):
        if value is not None and not args.query_fa:
            ap.error(f"{flag} needs --query-fa")
    if args.index_minimizer_length is not None and not 1 <= args.index_minimizer_length <= min(args.k, 31):
        ap.error(f"--index-minimizer-length must be in 1..{min(args.k, 31)} (1 .. min(k, 31), as --query-minimizer-length)")
    if args.min_component_kmers is not None and args.index_colors:
        ap.error("--min-component-kmers cannot be combined with --index-colors")
    if args.query_minimizer_length is not None:
        if args.query_index != "minimizer":
            ap.error("--query-minimizer-length needs --query-index minimizer")
        if not 1 <= args.query_minimizer_length <= min(args.k, 31):
            ap.error(f"--query-minimizer-length must be in 1..{min(args.k, 31)} (1 .. min(k, 31))")
    for over, out in (("greedytigs", args.greedytigs_fa_out), ("eulertigs", args.eulertigs_fa_out)):
        if args.query_index_over == over and not out:
            ap.error(f"--query-index-over {over} needs --{over}-fa-out")
    for flag, value in (("--query-locate-out", args.query_locate_out), ("--query-abundance-profile-out", args.query_abundance_profile_out),
                        ("--query-abundance-out", args.query_abundance_out), ("--query-colors-out", args.query_colors_out)):
        if value is None:
            continue
        if args.query_index == "minimizer":  # (a slot per class is what carries positions, weights and colours)
            ap.error(f"{flag} cannot be combined with --query-index minimizer: it needs the table index")
        if args.query_index_over not in (None, "input"):
            ap.error(f"{flag} cannot be combined with --query-index-over {args.query_index_over}: it needs the index over the input")
    for flag, value in (("--min-abundance", args.min_abundance), ("--kmer-spectrum-out", args.kmer_spectrum_out),
                        ("--unitig-abundance-out", args.unitig_abundance_out), ("--unitig-kmer-abundance-out", args.unitig_kmer_abundance_out),
                        ("--color-matrix-out", args.color_matrix_out), ("--unitig-colors-out", args.unitig_colors_out),
                        ("--monochromatic-unitigs", args.monochromatic_unitigs or None), ("--color-classes-out", args.color_classes_out),
                        ("--unitig-color-classes-out", args.unitig_color_classes_out), ("--clip-tips", args.clip_tips),
                        ("--remove-isolated", args.remove_isolated), ("--clean-rounds", args.clean_rounds),
                        ("--pop-bubbles", args.pop_bubbles), ("--bubble-ratio", args.bubble_ratio)) + _SELECTION_FLAGS(args):
        if value is not None and args.seq_in is None:
            ap.error(f"{flag} needs --seq-in")
    _check_selection(ap, args)
    if args.clip_tips is not None and args.clip_tips < 2:
        ap.error("--clip-tips must be >= 2")
    if args.remove_isolated is not None and args.remove_isolated < 1:
        ap.error("--remove-isolated must be >= 1")
    if args.pop_bubbles is not None and args.pop_bubbles < 2:
        ap.error("--pop-bubbles must be >= 2")
    if args.bubble_ratio is not None and args.pop_bubbles is None:
        ap.error("--bubble-ratio needs --pop-bubbles")
    if args.bubble_ratio is not None and not 1 <= args.bubble_ratio <= 255:
        ap.error("--bubble-ratio must be in 1..255")
    if args.clean_rounds is not None and args.clip_tips is None and args.remove_isolated is None and args.pop_bubbles is None:
        ap.error("--clean-rounds needs --clip-tips or --remove-isolated")
    if args.clean_rounds is not None and not 1 <= args.clean_rounds <= 64:
        ap.error("--clean-rounds must be in 1..64")
    if args.min_abundance is not None and args.min_abundance < 1:
        ap.error("--min-abundance must be >= 1")
    if args.min_component_kmers is not None:
        if args.min_component_kmers < 1:
            ap.error("--min-component-kmers must be >= 1")
        if args.bcalm_in is not None:
            ap.error("--min-component-kmers needs --seq-in or --fa-in")
        for flag, value in (("--color-matrix-out", args.color_matrix_out), ("--unitig-colors-out", args.unitig_colors_out),
                            ("--query-colors-out", args.query_colors_out), ("--query-index-colors-out", args.query_index_colors_out),
                            ("--monochromatic-unitigs", args.monochromatic_unitigs or None), ("--color-classes-out", args.color_classes_out), ("--unitig-color-classes-out", args.unitig_color_classes_out),
                            ("--pseudoalign-fa", args.pseudoalign_fa), ("--require-colors", args.require_colors),
                            ("--forbid-colors", args.forbid_colors), ("--min-colors", args.min_colors), ("--max-colors", args.max_colors)):
            if value is not None:
                ap.error(f"--min-component-kmers cannot be combined with {flag}")
    if args.bubbles_max_kmers is not None:
        if args.bubbles_out is None:
            ap.error("--bubbles-max-kmers needs --bubbles-out")
        if args.bubbles_max_kmers < 2:
            ap.error("--bubbles-max-kmers must be >= 2")
    if args.bubbles_out is not None:
        if args.bcalm_in is not None:  # (a graph built from links does not join two unitig ends that merely leave the same (k-1)-mer)
            ap.error("--bubbles-out needs --seq-in or --fa-in")
        if args.monochromatic_unitigs:  # (unitigs cut at the colour changes are no arms)
            ap.error("--bubbles-out cannot be combined with --monochromatic-unitigs")
    for flag, value in (("--min-base-quality", args.min_base_quality), ("--query-min-base-quality", args.query_min_base_quality),
                        ("--count-min-base-quality", args.count_min_base_quality),
                        ("--pseudoalign-min-base-quality", args.pseudoalign_min_base_quality),
                        ("--filter-min-base-quality", args.filter_min_base_quality)):
        if value is not None and not 0 <= value <= 93:
            ap.error(f"{flag} must be in 0..93")
    if not (args.selection_out or args.color_classes_out or args.unitig_color_classes_out or args.color_matrix_out or args.unitig_colors_out or args.kmer_spectrum_out or args.unitig_abundance_out or args.unitig_kmer_abundance_out or args.query_fa or args.count_fa or args.pseudoalign_fa or args.correct_fa or args.thread_fa or args.greedytigs_fa_out or args.eulertigs_fa_out or args.greedytigs_gfa_out or args.eulertigs_gfa_out
            or args.greedytigs_duplication_bitvector_out or args.matchtigs_fa_out or args.matchtigs_gfa_out or args.verify_fa or args.unitigs_fa_out
            or args.unitigs_bcalm_out or args.unitigs_gfa_out or args.components_out or args.unitig_components_out or args.index_out
            or args.bubbles_out):
        ap.error("nothing to do: give --greedytigs-fa-out / --greedytigs-gfa-out and/or --eulertigs-fa-out / --eulertigs-gfa-out")

    from . import api

    # FASTQ is told from FASTA by the content; the quality flags need a file they can apply to
    aligned = (args.pseudoalign_fa or []) + (args.pseudoalign_mate_fa or [])
    filters = (args.subtract_fa or []) + (args.intersect_fa or [])
    fastq = {path for path in (args.seq_in or []) + (args.query_fa or []) + (args.count_fa or []) + aligned + (args.correct_fa or [])
             + (args.thread_fa or []) + filters if api.sequence_file_format(path) == 2}
    if args.filter_min_base_quality is not None and not fastq.intersection(filters):
        ap.error("--filter-min-base-quality needs a fastq file among --subtract-fa / --intersect-fa")
    if args.min_base_quality is not None and not fastq.intersection((args.seq_in or []) + (args.query_fa or [])):
        ap.error("--min-base-quality needs a fastq file among --seq-in / --query-fa")
    if args.query_min_base_quality is not None and not fastq.intersection(args.query_fa or []):
        ap.error("--query-min-base-quality needs a fastq file among --query-fa")
    if args.count_min_base_quality is not None and not fastq.intersection(args.count_fa):
        ap.error("--count-min-base-quality needs a fastq file among --count-fa")
    if args.pseudoalign_min_base_quality is not None and not fastq.intersection(aligned):
        ap.error("--pseudoalign-min-base-quality needs a fastq file among --pseudoalign-fa / --pseudoalign-mate-fa")
    if args.thread_min_base_quality is not None and not fastq.intersection(args.thread_fa):
        ap.error("--thread-min-base-quality needs a fastq file among --thread-fa")
    try:
        return _run(api, args, fastq)
    except api.FastqFormatError as e:  # an error of the input: the message names file, record, line and reason
        print(e, file=sys.stderr)
        return 2


def _SELECTION_FLAGS(args):
    """(flag, value) of every flag of the k-mer selection."""
    return (("--require-colors", args.require_colors), ("--forbid-colors", args.forbid_colors), ("--min-colors", args.min_colors),
            ("--max-colors", args.max_colors), ("--subtract-fa", args.subtract_fa), ("--subtract-min-abundance", args.subtract_min_abundance),
            ("--intersect-fa", args.intersect_fa), ("--intersect-min-abundance", args.intersect_min_abundance),
            ("--filter-min-base-quality", args.filter_min_base_quality), ("--selection-out", args.selection_out))


def _selects_by_color(args) -> bool:
    return any(v is not None for v in (args.require_colors, args.forbid_colors, args.min_colors, args.max_colors))


def _selects(args) -> bool:
    return any(value is not None for _, value in _SELECTION_FLAGS(args))


def _color_list(text: str):
    """`0,2,5-7` -> [0, 2, 5, 6, 7]; None for what is no such list."""
    out = []
    for part in text.split(","):
        lo, dash, hi = part.partition("-")
        if not lo.isdigit() or (dash and not hi.isdigit()) or (dash and int(hi) < int(lo)):
            return None
        out += list(range(int(lo), int(hi if dash else lo) + 1))
    return out


def _check_selection(ap, args) -> None:
    """The argument errors of the selection flags: each names its flag, before any sequence is read."""
    if not _selects(args):
        return
    n = len(args.seq_in)
    masks = {}
    for flag, text in (("--require-colors", args.require_colors), ("--forbid-colors", args.forbid_colors)):
        numbers = _color_list(text) if text is not None else []
        if numbers is None:
            ap.error(f"{flag} {text}: a list of 0-based file numbers as commas and ranges, e.g. 0,2,5-7")
        if numbers and max(numbers) >= n:
            ap.error(f"{flag} names file {max(numbers)}: there are {n} --seq-in files, numbered from 0")
        masks[flag] = set(numbers)
    both = masks["--require-colors"] & masks["--forbid-colors"]
    if both:
        ap.error(f"--require-colors and --forbid-colors both name file {min(both)}")
    for flag, value in (("--min-colors", args.min_colors), ("--max-colors", args.max_colors)):
        if value is not None and not 0 <= value <= MAX_COLORS:
            ap.error(f"{flag} must be in 0..{MAX_COLORS}")
    if (args.min_colors or 0) > (MAX_COLORS if args.max_colors is None else args.max_colors):
        ap.error(f"--min-colors {args.min_colors} exceeds --max-colors {MAX_COLORS if args.max_colors is None else args.max_colors}")
    for flag, value, files, needs in (("--subtract-min-abundance", args.subtract_min_abundance, args.subtract_fa, "--subtract-fa"),
                                      ("--intersect-min-abundance", args.intersect_min_abundance, args.intersect_fa, "--intersect-fa")):
        if value is not None and not files:
            ap.error(f"{flag} needs {needs}")
        if value is not None and value < 1:
            ap.error(f"{flag} must be >= 1")
    if args.filter_min_base_quality is not None and not (args.subtract_fa or args.intersect_fa):
        ap.error("--filter-min-base-quality needs --subtract-fa or --intersect-fa")
    args.require_mask = sum(1 << c for c in masks["--require-colors"])
    args.forbid_mask = sum(1 << c for c in masks["--forbid-colors"])


def _check_thread(ap, args) -> None:
    """The rules of the `--thread-*` flags among themselves (those that need neither k nor a file)."""
    if args.thread_fa:
        if not (args.thread_gaf_out or args.thread_report_out):
            ap.error("--thread-fa needs --thread-gaf-out or --thread-report-out")
        if args.thread_min_kmers is not None and not 1 <= args.thread_min_kmers < 1 << 63:
            ap.error("--thread-min-kmers must be >= 1")
        if args.thread_min_base_quality is not None and not 0 <= args.thread_min_base_quality <= 93:
            ap.error("--thread-min-base-quality must be in 0..93")
        if args.thread_minimizer_length is not None and args.thread_index != "minimizer":
            ap.error("--thread-minimizer-length needs --thread-index minimizer")
    else:
        for flag, value in (("--thread-gaf-out", args.thread_gaf_out), ("--thread-report-out", args.thread_report_out),
                            ("--thread-min-kmers", args.thread_min_kmers), ("--thread-min-base-quality", args.thread_min_base_quality),
                            ("--thread-index", args.thread_index), ("--thread-minimizer-length", args.thread_minimizer_length)):
            if value is not None:
                ap.error(f"{flag} needs --thread-fa")


def _check_pseudoalign(ap, args) -> None:
    """The rules of the `--pseudoalign-*` flags among themselves; sets args.pseudoalign_permille."""
    args.pseudoalign_permille = None
    if args.pseudoalign_fa:
        if args.seq_in is None and args.index_in is None:
            ap.error("--pseudoalign-fa needs --seq-in: the colours are the --seq-in files")
        if not (args.pseudoalign_out or args.pseudoalign_classes_out or args.pseudoalign_summary_out):
            ap.error("--pseudoalign-fa needs --pseudoalign-out, --pseudoalign-classes-out or --pseudoalign-summary-out")
        if args.pseudoalign_mate_fa and len(args.pseudoalign_mate_fa) != len(args.pseudoalign_fa):
            ap.error(f"{len(args.pseudoalign_mate_fa)} --pseudoalign-mate-fa files for {len(args.pseudoalign_fa)} --pseudoalign-fa files: "
                     "give none, or one per --pseudoalign-fa")
        args.pseudoalign_permille = _permille(args.pseudoalign_threshold if args.pseudoalign_threshold is not None else "1")
        if args.pseudoalign_permille is None:
            ap.error(f"--pseudoalign-threshold must be a decimal in (0, 1] with at most three places, not {args.pseudoalign_threshold!r}")
        if args.pseudoalign_min_kmers is not None and args.pseudoalign_min_kmers < 1:
            ap.error("--pseudoalign-min-kmers must be >= 1")
        if args.pseudoalign_minimizer_length is not None:
            if args.pseudoalign_index != "minimizer":
                ap.error("--pseudoalign-minimizer-length needs --pseudoalign-index minimizer")
            if not 1 <= args.pseudoalign_minimizer_length <= min(args.k, 31):
                ap.error(f"--pseudoalign-minimizer-length must be in 1..{min(args.k, 31)} (1 .. min(k, 31), as --count-minimizer-length)")
    else:
        for flag, value in (("--pseudoalign-mate-fa", args.pseudoalign_mate_fa), ("--pseudoalign-out", args.pseudoalign_out),
                            ("--pseudoalign-classes-out", args.pseudoalign_classes_out), ("--pseudoalign-summary-out", args.pseudoalign_summary_out),
                            ("--pseudoalign-threshold", args.pseudoalign_threshold), ("--pseudoalign-over", args.pseudoalign_over),
                            ("--pseudoalign-min-kmers", args.pseudoalign_min_kmers),
                            ("--pseudoalign-min-base-quality", args.pseudoalign_min_base_quality), ("--pseudoalign-index", args.pseudoalign_index),
                            ("--pseudoalign-minimizer-length", args.pseudoalign_minimizer_length)):
            if value is not None:
                ap.error(f"{flag} needs --pseudoalign-fa")


def _permille(text: str):
    """`--pseudoalign-threshold`: a decimal in (0, 1] with at most three places -> its thousandths, 1 .. 1000; None for anything else.
    Never through a float."""
    import decimal

    try:
        t = decimal.Decimal(text)
    except decimal.InvalidOperation:
        return None
    if not t.is_finite() or not 0 < t <= 1 or t * 1000 != (t * 1000).to_integral_value():
        return None
    return int(t * 1000)


# what a run on an index file may be asked (`--index-in`): everything else needs sequences of the indexed set
_INDEX_IN_SERVES = {"help", "index_in", "k", "threads", "device", "compression_level", "blossom5_command", "query_fa", "query_out",
                    "query_presence_out", "query_index_locate_out", "query_min_base_quality", "query_index", "query_index_abundance_out",
                    "query_index_abundance_profile_out", "query_index_colors_out", "pseudoalign_fa", "pseudoalign_mate_fa", "pseudoalign_out",
                    "pseudoalign_classes_out", "pseudoalign_summary_out", "pseudoalign_threshold", "pseudoalign_over", "pseudoalign_min_kmers",
                    "pseudoalign_min_base_quality", "pseudoalign_index", "thread_fa", "thread_gaf_out", "thread_report_out", "thread_min_kmers",
                    "thread_min_base_quality", "thread_index"}


def _index_info(path) -> int:
    """`--index-info`: the header's fields and the metadata of an index file as `key\tvalue` lines; the header checks of a load on
    the host, no GPU. 2 if the header is refused."""
    import json

    from . import api

    try:
        head = api.tig_index_file_info(path)
    except api.IndexFileError as e:
        print(e, file=sys.stderr)
        return 2
    import dataclasses

    rows = [("file", path), ("file_bytes", head["file_bytes"]), ("format_version", 1)]
    rows += list(dataclasses.asdict(head["info"]).items())
    rows += [("locating", int(head["locating"])), ("weighted", int(head["weighted"])), ("colored", int(head["colored"])), ("n_colors", head["n_colors"]),
             ("win_offset_bytes", head["win_offset_bytes"])]
    for what, p in head["payload_info"].items():
        rows += [(f"{what}.{key}", value) for key, value in p.items()]
    rows += [(f"meta.{key}", value if isinstance(value, str) else json.dumps(value, ensure_ascii=False, sort_keys=True))
             for key, value in sorted(head["meta"].items())]
    sys.stdout.write("".join(f"{key}\t{value}\n" for key, value in rows))
    return 0


def _main_index_in(ap, args) -> int:
    """`--index-in`: the checks that need no file first (argparse errors, before the GPU is touched), then the file's header on the
    host, then the run. A refused file ends the run with status 2 and the library's message, as a malformed FASTQ does."""
    for action in ap._actions:
        value = getattr(args, action.dest, None)
        if action.dest in _INDEX_IN_SERVES or value is None or value == action.default or not action.option_strings:
            continue
        flag = action.option_strings[-1]
        if action.dest in ("bcalm_in", "gfa_in", "fa_in", "seq_in"):
            ap.error(f"--index-in cannot be combined with {flag}: the index file is the input")
        if action.dest in ("query_index_over", "query_minimizer_length", "pseudoalign_minimizer_length", "thread_minimizer_length"):
            ap.error(f"{flag} cannot be combined with --index-in: what is indexed and its minimizer length are the file's to say")
        ap.error(f"{flag} cannot be combined with --index-in: it needs the sequences of the indexed set, and a run on an index file reads none")
    if args.query_index == "table":
        ap.error("--query-index table cannot be combined with --index-in: the file holds the minimizer index")
    if args.pseudoalign_index == "table":
        ap.error("--pseudoalign-index table cannot be combined with --index-in: the file holds the minimizer index")
    if args.thread_index == "table":
        ap.error("--thread-index table cannot be combined with --index-in: the file holds the minimizer index")
    if not (args.query_fa or args.pseudoalign_fa or args.thread_fa):
        ap.error("nothing to do with --index-in: give --query-fa with --query-out, --pseudoalign-fa and/or --thread-fa")
    _check_thread(ap, args)
    if bool(args.query_fa) != bool(args.query_out):
        ap.error("--query-fa needs --query-out" if args.query_fa else "--query-out needs --query-fa")
    for flag, value in (("--query-presence-out", args.query_presence_out), ("--query-index-locate-out", args.query_index_locate_out),
                        ("--query-index-abundance-out", args.query_index_abundance_out), ("--query-index-colors-out", args.query_index_colors_out),
                        ("--query-index", args.query_index), ("--query-min-base-quality", args.query_min_base_quality)):
        if value is not None and not args.query_fa:
            ap.error(f"{flag} needs --query-fa")
    if args.query_index_abundance_profile_out and not args.query_index_abundance_out:
        ap.error("--query-index-abundance-profile-out needs --query-index-abundance-out")
    _check_pseudoalign(ap, args)
    for flag, value in (("--query-min-base-quality", args.query_min_base_quality), ("--pseudoalign-min-base-quality", args.pseudoalign_min_base_quality)):
        if value is not None and not 0 <= value <= 93:
            ap.error(f"{flag} must be in 0..93")
    if not 0 <= args.compression_level <= 9:
        ap.error("compression level must be in 0..9")

    from . import api

    aligned = (args.pseudoalign_fa or []) + (args.pseudoalign_mate_fa or [])
    fastq = {path for path in (args.query_fa or []) + aligned + (args.thread_fa or []) if api.sequence_file_format(path) == 2}
    if args.query_min_base_quality is not None and not fastq.intersection(args.query_fa or []):
        ap.error("--query-min-base-quality needs a fastq file among --query-fa")
    if args.pseudoalign_min_base_quality is not None and not fastq.intersection(aligned):
        ap.error("--pseudoalign-min-base-quality needs a fastq file among --pseudoalign-fa / --pseudoalign-mate-fa")
    if args.thread_min_base_quality is not None and not fastq.intersection(args.thread_fa):
        ap.error("--thread-min-base-quality needs a fastq file among --thread-fa")
    try:
        head = api.tig_index_file_info(args.index_in)  # (on the host: what the file can serve is known before the GPU is touched)
        if args.k is not None and args.k != head["info"].k:
            print(f"--index-in {args.index_in}: the file was built with k = {head['info'].k}, not -k {args.k}", file=sys.stderr)
            return 2
        for flag, value, has, lacks in (("--query-index-locate-out", args.query_index_locate_out, head["locating"], "the positions of its heavy buckets"),
                                        ("--query-index-abundance-out", args.query_index_abundance_out, head["weighted"], "weights (--index-weights)"),
                                        ("--query-index-colors-out", args.query_index_colors_out, head["colored"], "colours (--index-colors)"),
                                        ("--pseudoalign-fa", args.pseudoalign_fa, head["colored"], "colours (--index-colors)"),
                                        ("--thread-fa", args.thread_fa, head["locating"], "the positions of its heavy buckets")):
            if value and not has:
                ap.error(f"{flag} cannot be served by --index-in {args.index_in}: the file keeps no {lacks}")
        names = head["meta"].get("colors") or []
        if head["colored"] and len(names) != head["n_colors"]:  # (a file of the library alone: its colours have no names)
            names = [f"color{c}" for c in range(head["n_colors"])]
        args.k, args.seq_in, args.query_index = head["info"].k, list(names), "minimizer"
        t0 = time.perf_counter()
        with api.TigIndex.load(args.index_in, args.device) as index:
            print(f"Loaded the index of {args.index_in} ({head['file_bytes']} bytes, over the {head['meta'].get('indexed', 'sequences')}) in "
                  f"{time.perf_counter() - t0:.1f}s: {index.info.describe()}", file=sys.stderr)
            if args.query_fa:
                _query(api, args, None, True if args.query_index_abundance_out else None, fastq, True if args.query_index_colors_out else None,
                       loaded=index)
            if args.thread_fa:  # (the segments are the records of whatever the file indexed, by number)
                _thread(api, args, None, fastq, index, keep=True)
            if args.pseudoalign_fa:
                return _pseudoalign(api, args, None, None, fastq, loaded=index)
        return 0
    except (api.IndexFileError, api.FastqFormatError) as e:  # an error of the input: the message names the file and the reason
        print(e, file=sys.stderr)
        return 2


def _index_out(api, args, store, kmer_counts, colors, cleaning, bubbles) -> None:
    """`--index-out`: a locating sparse index over the unitig store or the tigs this run wrote, with the abundances and / or the
    colours by position if asked for, saved as one file. The metadata says what was indexed, the colours' names (the
    `--seq-in` paths as given, in order), `min_abundance` and the cleaning flags used."""
    t0 = time.perf_counter()
    over = args.index_over or "input"
    indexed = store if over == "input" else api.read_sequences(args.greedytigs_fa_out if over == "greedytigs" else args.eulertigs_fa_out)
    if kmer_counts is not None or colors is not None:
        weights, masks = (kmer_counts, None if colors is None else colors.kmer_colors) if over == "input" else _tig_payloads(
            api, args, store, indexed, kmer_counts, colors, over)
        index = api.TigIndex.annotated(indexed, args.k, args.index_minimizer_length, args.device, weights=weights, colors=masks,
                                       n_colors=None if colors is None else colors.n_colors)
    else:
        index = api.TigIndex(indexed, args.k, args.index_minimizer_length, args.device, locate=True)
    cleaning_flags = {name: value for name, value in (("clip_tips", args.clip_tips), ("remove_isolated", args.remove_isolated),
                                                      ("clean_rounds", args.clean_rounds), ("pop_bubbles", args.pop_bubbles),
                                                      ("bubble_ratio", args.bubble_ratio), ("min_component_kmers", args.min_component_kmers),
                                                      ("monochromatic_unitigs", args.monochromatic_unitigs or None)) if value is not None}
    meta = {"indexed": over, "colors": list(args.seq_in) if colors is not None else [], "min_abundance": args.min_abundance or 1,
            "cleaning": cleaning_flags}
    if _selects(args):  # (the flags as given, the filter files by their paths)
        meta["selection"] = {flag.lstrip("-").replace("-", "_"): value for flag, value in _SELECTION_FLAGS(args)
                             if value is not None and flag != "--selection-out"}
    with index:
        n_bytes = index.save(args.index_out, meta)
        print(f"Writing the index over the {over} to {args.index_out} took {time.perf_counter() - t0:.1f}s: {n_bytes} bytes; "
              f"{index.info.describe()}", file=sys.stderr)


def _read_seq_in(api, args, fastq, record_colors=None, paths=None, min_base_quality=None):
    """The `--seq-in` files (or `paths`, with their own quality threshold: the filter files of a selection) as one sequence set: the
    store of a single file as it is, else (data, offsets) of the files' stores one after the other, and the non-ACGT / low-quality
    runs cut. record_colors: a list that takes, per record, the number of its file."""
    import numpy as np

    stores = []
    for path in args.seq_in if paths is None else paths:
        if path in fastq:
            st, stats = api.read_fastq(path, (args.min_base_quality if paths is None else min_base_quality) or 0, args.device)
            print(f"Read {path}: {stats.describe()}", file=sys.stderr)
        else:
            st = api.read_sequences(path, split_non_acgt=True)
        stores.append(st)
    if record_colors is not None:  # every piece of a file has the file's colour
        record_colors.extend(np.repeat(np.arange(len(stores)), [len(st) for st in stores]).tolist())
    cut = sum(st.pieces_cut for st in stores)
    if len(stores) == 1:
        return stores[0], cut
    arrays = [st.arrays() for st in stores]
    base = np.cumsum([0] + [len(d) for d, _ in arrays]).astype(np.uint64)
    data = np.concatenate([d for d, _ in arrays])
    off = np.concatenate([o[:-1] + b for (_, o), b in zip(arrays, base)] + [base[-1:]])
    return (data, off), cut


def _run(api, args, fastq) -> int:
    t0 = time.perf_counter()
    cleaning = bubbles = abundance = selection = None
    component_filter = args.min_component_kmers is not None  # 
    if args.bcalm_in is not None:
        graph, store = api.read_bcalm2(args.bcalm_in, args.k)
    elif args.seq_in is not None:  # sequences -> unitigs (GPU compaction) -> graph (the --fa-in join on the same store)
        classed = bool(args.monochromatic_unitigs or args.color_classes_out or args.unitig_color_classes_out)  # 
        colored = bool(args.color_matrix_out or args.unitig_colors_out or args.query_colors_out or args.query_index_colors_out or classed
                       or args.pseudoalign_fa or args.index_colors or _selects_by_color(args)
                       or (args.bubbles_out is not None and len(args.seq_in) > 1))  # (the carriers of DESIGN.md 38)
        record_colors = [] if colored else None
        seqs, pieces_cut = _read_seq_in(api, args, fastq, record_colors)
        abundance = colors = cleaning = None
        selecting = _selects(args)  # 
        if selecting:
            subtract, intersect = (_read_seq_in(api, args, fastq, None, paths, args.filter_min_base_quality)[0] if paths else None
                                   for paths in (args.subtract_fa, args.intersect_fa))
            chosen = api.KmerSelection(args.require_mask, args.forbid_mask, args.min_colors or 0, MAX_COLORS if args.max_colors is None else args.max_colors,
                                       subtract, args.subtract_min_abundance or 1, intersect, args.intersect_min_abundance or 1)
        popping = args.pop_bubbles is not None  # 
        cleaned = args.clip_tips is not None or args.remove_isolated is not None or popping  # 
        per_kmer = bool(args.query_abundance_out or args.query_index_abundance_out or args.unitig_kmer_abundance_out
                        or args.index_weights)  # 
        counted = selecting or not (args.min_abundance is None and not (args.kmer_spectrum_out or args.unitig_abundance_out or per_kmer))
        if not counted and not colored and not cleaned:
            store, compaction = api.compact_unitigs(seqs, args.k, args.device)
        else:  # the counted compaction; an output flag alone counts without filtering
            min_abundance = args.min_abundance or 1
            if selecting:  # (the simplified call over the selected k-mers; what it does not clean or pop it reports as None, like the calls below)
                store, compaction, abundance, colors, classes, cleaning, bubbles, selection = api.compact_unitigs_selected(
                    seqs, args.k, chosen, args.pop_bubbles or 0, args.bubble_ratio or 1, args.clip_tips or 0, args.remove_isolated or 0,
                    args.clean_rounds or 1, min_abundance, record_colors if colored else None, len(args.seq_in) if colored else 0,
                    bool(args.monochromatic_unitigs), per_kmer, args.device)
                cleaning, bubbles = cleaning if cleaned else None, bubbles if popping else None
            elif popping:  # (the cleaned call whose rounds pop bubbles too)
                store, compaction, abundance, colors, classes, cleaning, bubbles = api.compact_unitigs_simplified(
                    seqs, args.k, args.pop_bubbles, args.bubble_ratio or 1, args.clip_tips or 0, args.remove_isolated or 0, args.clean_rounds or 1,
                    min_abundance, record_colors if colored else None, len(args.seq_in) if colored else 0, bool(args.monochromatic_unitigs),
                    per_kmer, args.device)
            elif cleaned:  # (whichever of the calls below it would have been, with the rounds in front of the final pass)
                store, compaction, abundance, colors, classes, cleaning = api.compact_unitigs_cleaned(
                    seqs, args.k, args.clip_tips or 0, args.remove_isolated or 0, args.clean_rounds or 1, min_abundance,
                    record_colors if colored else None, len(args.seq_in) if colored else 0, bool(args.monochromatic_unitigs), per_kmer, args.device)
            elif classed:  # (the coloured call plus the class dictionary, over unitigs cut at the colour changes if asked for)
                store, compaction, abundance, colors, classes = api.compact_unitigs_colored_classes(
                    seqs, args.k, record_colors, len(args.seq_in), min_abundance, args.monochromatic_unitigs, args.device)
            elif colored:  # (the counted call that hands out the counts, plus the colours)
                store, compaction, abundance, colors = api.compact_unitigs_colored(seqs, args.k, record_colors, len(args.seq_in), min_abundance,
                                                                                   args.device)
            elif per_kmer:
                store, compaction, abundance = api.compact_unitigs_counted(seqs, args.k, min_abundance, args.device, kmer_counts=True)
            else:
                store, compaction, abundance = api.compact_unitigs_counted(seqs, args.k, min_abundance, args.device)
            if args.kmer_spectrum_out:  # (also when nothing is kept: this is how a threshold that works is found)
                _write_spectrum(args, abundance)
            if selecting:  # (also when nothing is selected: the matrix and its occupancy row are how a carrier threshold is found)
                if args.selection_out:
                    _write_selection(args, abundance, colors, selection)
                if args.color_matrix_out:
                    _write_color_matrix(args, colors)
            if abundance.distinct_kept == 0:
                print(f"no k-mer reaches --min-abundance {min_abundance} ({abundance.describe()})", file=sys.stderr)
                return 1
            if selecting and selection.selected == 0:
                print(f"no k-mer is selected ({selection.describe()}; {abundance.describe()})", file=sys.stderr)
                return 1
            if len(store) == 0:
                print(f"nothing is left after cleaning ({cleaning.describe()}; {bubbles.describe() + '; ' if bubbles is not None else ''}"
                      f"{abundance.describe()})", file=sys.stderr)
                return 1
            if args.unitig_abundance_out and not component_filter:  # (with the component filter: after it, below)
                _write_unitig_abundance(args, store, abundance)
            if args.unitig_kmer_abundance_out and not component_filter:
                _write_unitig_kmer_abundance(args, store, abundance)
            if args.color_matrix_out and not selecting:
                _write_color_matrix(args, colors)
            if args.unitig_colors_out:
                _write_unitig_colors(args, store, colors)
            if classed:
                if args.color_classes_out:
                    _write_color_classes(args, classes)
                if args.unitig_color_classes_out:
                    _write_unitig_color_classes(args, store, classes)
                print(f"Colour classes: {classes.describe()}", file=sys.stderr)
        graph = api.Bigraph.from_sequences(store.arrays(), args.k, args.device)
    else:
        graph, store = api.read_fasta(args.fa_in, args.k, args.device)
    loaded = f"Loaded {len(store)} unitigs: {graph.node_count()} nodes, {graph.edge_count()} edges in {time.perf_counter() - t0:.1f}s"
    if args.seq_in is not None:
        loaded += f" (compacted from {compaction.describe()}; "
        loaded += f"cut into {compaction.unitigs} monochromatic unitigs; " if args.monochromatic_unitigs else ""
        loaded += f"{abundance.describe()}; " if abundance is not None and counted else ""
        loaded += f"{selection.describe()}; " if selection is not None else ""
        loaded += f"{cleaning.describe()}; " if cleaning is not None else ""
        loaded += f"{bubbles.describe()}; " if bubbles is not None else ""
        loaded += f"{pieces_cut} non-ACGT runs cut)"
    print(loaded, file=sys.stderr)
    component_kmers = 0  # the k-mers the component filter removed
    if component_filter:  # once, in front of everything that reads the unitigs; links exist only inside a component, so what stays is maximal
        import dataclasses

        import numpy as np

        given = store  # (what --fa-in's unitigs are verified against)
        store, keep, before = api.select_components(graph, given, args.k, args.min_component_kmers,
                                                    abundance.unitig_sums if abundance is not None else None, args.device)
        small = before.kmers < np.uint64(args.min_component_kmers)
        component_kmers = int(before.kmers[small].sum())
        print(f"Component filter: {int(small.sum())} of {len(before)} components have fewer than {args.min_component_kmers} k-mers: "
              f"{int(before.unitigs[small].sum())} unitigs, {component_kmers} k-mers removed, {len(store)} unitigs left "
              f"({before.describe()})", file=sys.stderr)
        if len(store) == 0:
            print(f"nothing is left after the component filter (--min-component-kmers {args.min_component_kmers}; {before.describe()})",
                  file=sys.stderr)
            return 1
        if abundance is not None:  # the abundances of the kept unitigs, for the outputs, KC and the weighted queries
            kmers = (np.diff(given.arrays()[1]) - np.uint64(args.k - 1)).astype(np.int64)
            abundance = dataclasses.replace(abundance, unitig_sums=abundance.unitig_sums[keep], kmer_counts=(
                None if abundance.kmer_counts is None else abundance.kmer_counts[np.repeat(keep, kmers)]))
        graph = api.Bigraph.from_sequences(store.arrays(), args.k, args.device)
        if args.unitig_abundance_out:
            _write_unitig_abundance(args, store, abundance)
        if args.unitig_kmer_abundance_out:
            _write_unitig_kmer_abundance(args, store, abundance)
    # what the tigs are verified against: the input as given -- on the --seq-in route the sequences, so that the check covers the compaction
    truth = seqs if args.seq_in is not None else store
    filtered = args.seq_in is not None and abundance is not None and min_abundance > 1
    deselected = selection.rejected if selection is not None else 0
    if filtered or cleaning is not None or component_filter or selection is not None:  # the tigs spell S_m less what the cleaning took, not the input's set: they are held to the
        truth = store                     # unitigs, and the unitigs to the input (below)
    cleaned_away = (cleaning.removed_kmers if cleaning is not None else 0) + (bubbles.arm_kmers if bubbles is not None else 0)

    def report(what: str, tigs, cmp) -> bool:
        """The verification line of one tig set; names the first missing and the first foreign k-mer when there is one."""
        line = f"Verifying {what}: {cmp.describe()}"
        if cmp.only_in_a:
            line += (f"; first missing k-mer: input record {cmp.first_only_in_a_record + 1} position {cmp.first_only_in_a_pos} "
                     f"{api.kmer_at(truth, cmp.first_only_in_a_record, cmp.first_only_in_a_pos, args.k)}")
        if cmp.only_in_b:
            line += (f"; first foreign k-mer: tig record {cmp.first_only_in_b_record + 1} position {cmp.first_only_in_b_pos} "
                     f"{api.kmer_at(tigs, cmp.first_only_in_b_record, cmp.first_only_in_b_pos, args.k)}")
        print(line, file=sys.stderr)
        return cmp.equal

    all_equal = True
    if (filtered or cleaning is not None or component_filter or selection is not None) and (args.verify or args.verify_fa):
        # by the k-mer set comparison, a kernel the compaction does not share: no foreign k-mer survived, and exactly the dropped, the
        # cleaned and those of the removed components are gone
        cmp = api.compare_kmer_sets(seqs if args.seq_in is not None else given, store, args.k, args.device)
        dropped = abundance.dropped if abundance is not None else 0
        ok = cmp.only_in_b == 0 and cmp.only_in_a == dropped + deselected + cleaned_away + component_kmers
        if selection is not None:
            print(f"Verifying selection: {cmp.distinct_b} of the input's {cmp.distinct_a} distinct k-mers are in the unitigs, "
                  f"{cmp.only_in_a} are not ({dropped} dropped by the abundance filter, {deselected} deselected, {cleaned_away} cleaned away, "
                  f"{component_kmers} in removed components), {cmp.only_in_b} foreign: {'as counted' if ok else 'MISMATCH'}", file=sys.stderr)
            # against the filter files themselves, by the comparison kernel: with A = 1 the unitigs share no k-mer with the subtract
            # files, with B = 1 every k-mer of the unitigs is in the intersect files
            if subtract is not None and chosen.subtract_min_abundance == 1:
                against = api.compare_kmer_sets(store, subtract, args.k, args.device)
                shared = against.distinct_b - against.only_in_b
                print(f"Verifying --subtract-fa: the unitigs share {shared} k-mers with the subtracted files: {'none' if shared == 0 else 'MISMATCH'}",
                      file=sys.stderr)
                ok = ok and shared == 0
            if intersect is not None and chosen.intersect_min_abundance == 1:
                against = api.compare_kmer_sets(intersect, store, args.k, args.device)
                print(f"Verifying --intersect-fa: {against.only_in_b} k-mers of the unitigs are not in the intersected files: "
                      f"{'none' if against.only_in_b == 0 else 'MISMATCH'}", file=sys.stderr)
                ok = ok and against.only_in_b == 0
        if filtered:
            print(f"Verifying abundance filter: {cmp.distinct_b} of the input's {cmp.distinct_a} distinct k-mers are in the unitigs, "
                  f"{cmp.only_in_a - deselected - cleaned_away - component_kmers} are not ({abundance.dropped} dropped by the filter), {cmp.only_in_b} foreign: "
                  f"{'as counted' if ok else 'MISMATCH'}", file=sys.stderr)
        if cleaning is not None:
            print(f"Verifying cleaning: {cmp.distinct_b} of the input's {cmp.distinct_a} distinct k-mers are in the unitigs, "
                  f"{cmp.only_in_a - component_kmers - deselected} are not ({abundance.dropped} dropped by the filter, {cleaning.tip_kmers} in tips, "
                  f"{cleaning.isolated_kmers} in isolated unitigs{f', {bubbles.arm_kmers} in bubble arms' if bubbles is not None else ''}), "
                  f"{cmp.only_in_b} foreign: {'as counted' if ok else 'MISMATCH'}", file=sys.stderr)
        if component_filter:
            print(f"Verifying component filter: {cmp.distinct_b} of the input's {cmp.distinct_a} distinct k-mers are in the unitigs, "
                  f"{cmp.only_in_a} are not ({dropped} dropped by the abundance filter, {cleaned_away} cleaned away, {component_kmers} in "
                  f"components of fewer than {args.min_component_kmers} k-mers), {cmp.only_in_b} foreign: "
                  f"{'as counted' if ok else 'MISMATCH'}", file=sys.stderr)
        all_equal &= ok
    for path in args.verify_fa or ():
        tigs = api.read_sequences(path)
        all_equal &= report(path, tigs, api.compare_kmer_sets(truth, tigs, args.k, args.device))
    if args.unitigs_fa_out:  # one walk per unitig through the tig writer (algorithm 1)
        r = api.compute_tigs_to_fasta_file(graph, store, 1, args.k, args.unitigs_fa_out, args.compression_level, args.device)
        graph.reset()
        print(f"Writing unitigs took {r['write_s']:.1f}s ({r['tigs']} unitigs, {r['fasta_bytes']} fasta bytes)", file=sys.stderr)
    if args.unitigs_bcalm_out or args.unitigs_gfa_out:  # the same unitigs with their links
        t1 = time.perf_counter()
        kc = abundance.unitig_sums if args.seq_in is not None and abundance is not None else None
        for path, gfa in ((args.unitigs_bcalm_out, False), (args.unitigs_gfa_out, True)):
            if path:
                r = api.write_unitig_graph(graph, store, args.k, path, gfa, kc, args.compression_level, args.device)
                print(f"Writing unitig graph took {time.perf_counter() - t1:.1f}s ({r['unitigs']} unitigs, {r['links']} links, "
                      f"{r['bytes']} bytes)", file=sys.stderr)
                t1 = time.perf_counter()
    if args.components_out or args.unitig_components_out:  # how the graph as written falls apart
        t1 = time.perf_counter()
        comps = api.unitig_components(graph, store, args.k, abundance.unitig_sums if args.seq_in is not None and abundance is not None else None,
                                      args.device)
        if args.components_out:
            _write_components(args, comps)
        if args.unitig_components_out:
            with _open_text(args, args.unitig_components_out) as f:
                f.write("".join(f"{c}\n" for c in comps.component_of.tolist()))
        print(f"Writing components took {time.perf_counter() - t1:.1f}s ({comps.describe()})", file=sys.stderr)
    if args.bubbles_out:  # what the variation is that the cleaning left
        import os

        import numpy as np

        t1 = time.perf_counter()
        masks = colors.kmer_colors if args.seq_in is not None and len(args.seq_in) > 1 else None
        if masks is not None and component_filter:  # (the masks of the kept unitigs' k-mers)
            masks = masks[np.repeat(keep, (np.diff(given.arrays()[1]) - np.uint64(args.k - 1)).astype(np.int64))]
        found = api.unitig_bubbles(graph, store, args.k, 2 * args.k if args.bubbles_max_kmers is None else args.bubbles_max_kmers,
                                   abundance.unitig_sums if args.seq_in is not None and abundance is not None else None, masks,
                                   len(args.seq_in) if masks is not None else 0, args.device)
        with _open_text(args, args.bubbles_out) as f:
            f.write(found.tsv(store, args.k, [os.path.basename(path) for path in args.seq_in] if masks is not None else None))
        print(f"Bubbles: {found.describe()} (found and written in {time.perf_counter() - t1:.1f}s)", file=sys.stderr)
    for name, alg, out, gfa, dup in (("matchtigs", 4, args.matchtigs_fa_out, args.matchtigs_gfa_out,
                                      args.matchtigs_duplication_bitvector_out),
                                     ("eulertigs", 3, args.eulertigs_fa_out, args.eulertigs_gfa_out, None),
                                     ("greedytigs", 5, args.greedytigs_fa_out, args.greedytigs_gfa_out,
                                      args.greedytigs_duplication_bitvector_out)):
        if not (out or gfa or dup):
            continue
        cfg = None
        if alg == 4:  # bin.rs:1141-1151: the matching files live next to the first matchtigs output; the matcher is looked up on PATH
            import shutil

            matcher = shutil.which(args.blossom5_command) or args.blossom5_command
            cfg = api.MatchtigAlgorithmConfiguration(args.threads, args.k, out or gfa, matcher, device_id=args.device)
        r = api.compute_tigs_to_fasta_file(graph, store, alg, args.k, out, args.compression_level, args.device, gfa_path=gfa,
                                           duplication_bitvector_path=dup, configuration=cfg, verify=args.verify, verify_against=truth)
        graph.reset()  # the reference clones the graph per algorithm (bin.rs:1069)
        print(f"Computing {name} took {r['compute_s']:.1f}s and writing took {r['write_s']:.1f}s "
              f"({r['tigs']} tigs, {r['fasta_bytes']} fasta bytes)", file=sys.stderr)
        if args.verify:
            all_equal &= report(f"{name} ({out or 'spelled in memory'})", r["verify_tigs"], r["verify"])
    if args.index_out:  # 
        _index_out(api, args, store, abundance.kmer_counts if args.index_weights else None, colors if args.index_colors else None, cleaning, bubbles)
    # the queries' index, left open, if it is the one the count asks for: the plain-enough table index over the unitig store, or
    #  the sparse index over the same sequences with the same minimizer length, then built locating
    shared_index = None
    count_sparse = args.count_index == "minimizer"
    share_sparse = bool(count_sparse and args.query_fa and args.query_index == "minimizer"
                        and (args.query_index_over or "input") == (args.count_index_over or "input")
                        and args.count_minimizer_length in (None, args.query_minimizer_length or api.default_minimizer_length(args.k)))
    # ... or the one the threading asks for: a LOCATING index over the unitig store -- the table if --query-locate-out
    # made it one, or the sparse index with the same minimizer length, unless a sparse count takes (and closes) that first
    thread_table = bool(args.thread_fa) and args.thread_index != "minimizer"
    thread_takes_table = thread_table and bool(args.query_fa and args.query_locate_out)
    thread_takes_sparse = bool(args.thread_fa and args.thread_index == "minimizer" and not count_sparse and args.query_fa
                               and args.query_index == "minimizer" and (args.query_index_over or "input") == "input"
                               and args.thread_minimizer_length in (None, args.query_minimizer_length or api.default_minimizer_length(args.k)))
    thread_index = None
    if args.query_fa:
        shared_index = _query(api, args, store, abundance.kmer_counts if args.query_abundance_out or args.query_index_abundance_out else None, fastq,
                              colors if args.query_colors_out or args.query_index_colors_out else None,
                              keep_index=(bool(args.count_fa) and not count_sparse) or bool(args.correct_fa and not args.count_fa)
                              or thread_takes_table,
                              keep_sparse=share_sparse or thread_takes_sparse)
        if thread_takes_sparse or (thread_takes_table and (count_sparse or not args.count_fa)):  # (no table count in between)
            thread_index, shared_index = shared_index, None
    if args.count_fa:  # (with --correct-fa or a threading on the table a table index it counted on stays open)
        shared_index = _count(api, args, store, fastq, shared_index, keep=bool(args.correct_fa) or (thread_takes_table and shared_index is not None))
    if args.thread_fa:
        if thread_takes_table and thread_index is None:
            thread_index, shared_index = shared_index, None
        # (a table index threaded on serves the correction too, unless the count left one for it already)
        kept = _thread(api, args, store, fastq, thread_index, keep=bool(args.correct_fa) and thread_table and shared_index is None)
        shared_index = kept if kept is not None else shared_index
    if args.pseudoalign_fa:
        status = _pseudoalign(api, args, store, colors, fastq)
        if status:
            return status
    if args.correct_fa:
        _correct(api, args, store, fastq, shared_index)
    return 0 if all_equal else 1


def _open_text(args, path):
    import gzip

    return gzip.open(path, "wt", compresslevel=args.compression_level) if path.endswith(".gz") else open(path, "w")


def _write_components(args, comps) -> None:
    """`--components-out`: one row per component, in order; mean = abundance / kmers with one decimal, rounded half up in integers,
    as the `km` of the unitig graph output."""
    with _open_text(args, args.components_out) as f:
        f.write("component\tfirst_unitig\tunitigs\tkmers\tbases\tabundance\tmean\tlinks\tdead_ends\tcircular\n")
        for c, (first, n, m, a, links, dead, irregular) in enumerate(zip(
                comps.first_unitig.tolist(), comps.unitigs.tolist(), comps.kmers.tolist(), comps.abundance.tolist(), comps.links.tolist(),
                comps.dead_ends.tolist(), comps.irregular.tolist())):
            t = (10 * a + m // 2) // m
            f.write(f"{c}\t{first}\t{n}\t{m}\t{m + (args.k - 1) * n}\t{a}\t{t // 10}.{t % 10}\t{links}\t{dead}\t{1 if irregular == 0 else 0}\n")


def _write_spectrum(args, abundance) -> None:
    """`--kmer-spectrum-out`: one row per non-empty bin, ascending; the last bin holds every abundance from 255 on."""
    last = len(abundance.spectrum) - 1
    with _open_text(args, args.kmer_spectrum_out) as f:
        f.write("abundance\tkmers\n")
        f.writelines(f"{c}{'+' if c == last else ''}\t{n}\n" for c, n in enumerate(abundance.spectrum.tolist()) if n)


def _write_unitig_abundance(args, store, abundance) -> None:
    """`--unitig-abundance-out`: row i describes record i of the unitig store (the order `--unitigs-fa-out` writes)."""
    import numpy as np

    kmers = (np.diff(store.arrays()[1]) - np.uint64(args.k - 1)).tolist()
    with _open_text(args, args.unitig_abundance_out) as f:
        f.write("unitig\tkmers\tabundance\tmean\n")
        f.writelines(f"{i}\t{n}\t{a}\t{a / n:.3f}\n" for i, (n, a) in enumerate(zip(kmers, abundance.unitig_sums.tolist())))


def _integer_lines(values, counts, dash=None) -> bytes:
    """The integers `values`, counts[i] of them on line i, space separated, each line followed by a newline; where `dash` is true the
    entry is `-`. One vectorised pass: the decimal digits are laid out in a byte matrix and the used ones picked."""
    import numpy as np

    values = np.asarray(values, np.uint64)
    counts = np.asarray(counts, np.int64)
    width = 1
    while values.size and int(values.max()) >= 10 ** width:
        width += 1
    digits = np.zeros((len(values), width + 1), np.uint8)  # right-aligned digits, then the separator
    rest = values.copy()
    for j in range(width - 1, -1, -1):
        digits[:, j] = ord("0") + (rest % np.uint64(10)).astype(np.uint8)
        rest //= np.uint64(10)
    used = np.zeros((len(values), width + 1), bool)
    lengths = np.ones(len(values), np.int64)
    for j in range(1, width):
        lengths += values >= np.uint64(10 ** j)
    used[:, :width] = np.arange(width)[None, :] >= (width - lengths)[:, None]
    if dash is not None:
        dash = np.asarray(dash, bool)
        digits[dash, width - 1] = ord("-")
        used[dash, :width - 1] = False
    used[:, width] = True
    digits[:, width] = ord(" ")
    ends = np.cumsum(counts)  # the last entry of a line ends it
    digits[ends[counts > 0] - 1, width] = ord("\n")
    body = digits[used]
    empty = np.flatnonzero(counts == 0)  # an empty line is a newline of its own: before the entry that follows it
    if len(empty) == 0:
        return body.tobytes()
    entry_start = np.concatenate([[0], np.cumsum(used.sum(axis=1))])
    at = entry_start[(ends - counts)[empty]]
    return np.insert(body, at, ord("\n")).tobytes()


def _write_unitig_kmer_abundance(args, store, abundance) -> None:
    """`--unitig-kmer-abundance-out`: line i holds the abundance of every k-mer of record i of the unitig store, left to right."""
    import gzip

    import numpy as np

    path = args.unitig_kmer_abundance_out
    kmers = (np.diff(store.arrays()[1]) - np.uint64(args.k - 1)).astype(np.int64)
    ends = np.cumsum(kmers)
    with (gzip.open(path, "wb", compresslevel=args.compression_level) if path.endswith(".gz") else open(path, "wb")) as f:
        at = 0
        while at < len(kmers):  # in slices of about 2^24 k-mers
            end = max(at + 1, int(np.searchsorted(ends, (int(ends[at - 1]) if at else 0) + (1 << 24), side="right")))
            lo, hi = (int(ends[at - 1]) if at else 0), int(ends[end - 1])
            f.write(_integer_lines(abundance.kmer_counts[lo:hi], kmers[at:end]))
            at = end


def _hex_runs(masks, counts) -> bytes:
    """Line i: the runs of equal masks among its counts[i] (>= 1) masks, left to right, as `length:hexmask`, space separated. One
    vectorised pass: the digits of both numbers are laid out in a byte matrix and the used ones picked."""
    import numpy as np

    masks = np.asarray(masks, np.uint64)
    ends = np.cumsum(np.asarray(counts, np.int64))
    first = np.ones(len(masks), bool)  # the first mask of a run: that of a line, or one that differs from the mask before it
    first[1:] = masks[1:] != masks[:-1]
    first[ends[:-1]] = True
    starts = np.flatnonzero(first)
    lengths = np.diff(np.append(starts, len(masks))).astype(np.uint64)
    run_masks = masks[starts]
    width = 1
    while lengths.size and int(lengths.max()) >= 10 ** width:
        width += 1
    cells = np.zeros((len(starts), width + 1 + 16 + 1), np.uint8)  # decimal digits, `:`, hex digits, the separator
    used = np.zeros(cells.shape, bool)
    rest, n_digits = lengths.copy(), np.ones(len(starts), np.int64)
    for j in range(width - 1, -1, -1):
        cells[:, j] = ord("0") + (rest % np.uint64(10)).astype(np.uint8)
        rest //= np.uint64(10)
    for j in range(1, width):
        n_digits += lengths >= np.uint64(10 ** j)
    used[:, :width] = np.arange(width)[None, :] >= (width - n_digits)[:, None]
    cells[:, width] = ord(":")
    hex_digits, n_hex = np.frombuffer(b"0123456789abcdef", np.uint8), np.ones(len(starts), np.int64)
    for j in range(16):
        cells[:, width + 1 + j] = hex_digits[((run_masks >> np.uint64(4 * (15 - j))) & np.uint64(15)).astype(np.int64)]
    for j in range(1, 16):
        n_hex += run_masks >= np.uint64(16 ** j)
    used[:, width + 1:width + 17] = np.arange(16)[None, :] >= (16 - n_hex)[:, None]
    used[:, width] = used[:, -1] = True
    cells[:, -1] = ord(" ")
    cells[np.searchsorted(starts, ends, side="left") - 1, -1] = ord("\n")  # the last run of a line ends it
    return cells[used].tobytes()


def _write_unitig_colors(args, store, colors) -> None:
    """`--unitig-colors-out`: line i describes the k-mers of record i of the unitig store, left to right, as runs of equal masks."""
    import gzip

    import numpy as np

    path = args.unitig_colors_out
    kmers = (np.diff(store.arrays()[1]) - np.uint64(args.k - 1)).astype(np.int64)
    ends = np.cumsum(kmers)
    with (gzip.open(path, "wb", compresslevel=args.compression_level) if path.endswith(".gz") else open(path, "wb")) as f:
        at = 0
        while at < len(kmers):  # in slices of about 2^24 k-mers
            end = max(at + 1, int(np.searchsorted(ends, (int(ends[at - 1]) if at else 0) + (1 << 24), side="right")))
            lo, hi = (int(ends[at - 1]) if at else 0), int(ends[end - 1])
            f.write(_hex_runs(colors.kmer_colors[lo:hi], kmers[at:end]))
            at = end


def _write_color_classes(args, classes) -> None:
    """`--color-classes-out`: one row per colour class, in the order the unitigs show them."""
    with _open_text(args, args.color_classes_out) as f:
        f.write("class\tmask\tcarriers\tkmers\truns\n")
        f.writelines(f"{c}\t{m:x}\t{bin(m).count('1')}\t{n}\t{r}\n" for c, (m, n, r) in enumerate(zip(
            classes.masks.tolist(), classes.kmers.tolist(), classes.runs.tolist())))


def _write_unitig_color_classes(args, store, classes) -> None:
    """`--unitig-color-classes-out`: line i describes the k-mers of record i of the unitig store, left to right, as runs of one class."""
    import numpy as np

    kmers = (np.diff(store.arrays()[1]) - np.uint64(args.k - 1)).astype(np.int64)
    cls = classes.kmer_class
    first = np.ones(len(cls), bool)  # the first k-mer of a run: that of a line, or one whose class differs from the one before it
    first[1:] = cls[1:] != cls[:-1]
    first[np.cumsum(kmers) - kmers] = True
    starts = np.flatnonzero(first)
    lengths = np.diff(np.append(starts, len(cls))).tolist()
    run_class = cls[starts].tolist()
    per_line = np.add.reduceat(first.astype(np.int64), np.cumsum(kmers) - kmers).tolist() if len(kmers) else []
    with _open_text(args, args.unitig_color_classes_out) as f:
        at = 0
        for n in per_line:
            f.write(" ".join(f"{l}:{c}" for l, c in zip(lengths[at:at + n], run_class[at:at + n])) + "\n")
            at += n


def _write_selection(args, abundance, colors, selection) -> None:
    """`--selection-out`: name<TAB>k-mers for the input, what the abundance threshold kept, what each rule rejected and
    what is selected; then per colour its file, its k-mers among those the threshold kept, and its selected k-mers."""
    rows = [("input", abundance.distinct_all), ("abundance_kept", selection.input_kmers), ("forbid", selection.rejected_forbid),
            ("require", selection.rejected_require), ("carriers", selection.rejected_carriers), ("subtract", selection.rejected_subtract),
            ("intersect", selection.rejected_intersect), ("selected", selection.selected)]
    with _open_text(args, args.selection_out) as f:
        f.writelines(f"{name}\t{int(n)}\n" for name, n in rows)
        if colors is not None:
            f.writelines(f"color\t{args.seq_in[c]}\t{int(colors.per_color[c])}\t{int(selection.per_color_selected[c])}\n" for c in range(colors.n_colors))


def _write_color_matrix(args, colors) -> None:
    """`--color-matrix-out`: row i = file i, its k-mers and those it shares with every file; the closing row: the k-mers carried by
    exactly 1 .. C files. One stderr line sums it up."""
    import numpy as np

    names, n = args.seq_in, colors.n_colors
    with _open_text(args, args.color_matrix_out) as f:
        f.write("\t".join(["color", "kmers"] + names) + "\n")
        f.writelines("\t".join([names[i], str(int(colors.per_color[i]))] + [str(x) for x in colors.shared[i].tolist()]) + "\n" for i in range(n))
        f.write("\t".join(["#occupancy"] + [str(x) for x in colors.occupancy[1:n + 1].tolist()]) + "\n")
    line = f"Colours: {int(colors.occupancy.sum())} k-mers kept in {n} colours, {colors.core} core, {colors.private} private"
    jac = colors.jaccard()
    pairs = [(jac[i, j], i, j) for i in range(n) for j in range(i + 1, n) if not np.isnan(jac[i, j])]
    if pairs:  # (ties: the first pair in the order of the files)
        hi, lo = max(pairs, key=lambda t: (t[0], -t[1], -t[2])), min(pairs)
        line += (f"; closest pair {names[hi[1]]} / {names[hi[2]]} (Jaccard {hi[0]:.4f}), most distant {names[lo[1]]} / {names[lo[2]]} "
                 f"(Jaccard {lo[0]:.4f})")
    print(line, file=sys.stderr)


def _tig_payloads(api, args, store, tigs, kmer_counts, colors, what):
    """The per-window weights and masks of a tig file: a k-mer's abundance and mask are functions of the k-mer, so a
    transient annotated table index over the unitig store is asked for every window of `tigs` (a UnitigStore), in slices of about
    2^24 bases, and the answers are cut to window order. The table is closed on return: the build peak of this route is the
    table's. Dies if a window of a tig is not a k-mer of the unitigs."""
    import numpy as np

    data, off = tigs.arrays()
    off = np.asarray(off).astype(np.int64)
    weights, masks = [], []
    with api.KmerIndex(store, args.k, args.device, weights=kmer_counts, colors=None if colors is None else colors.kmer_colors,
                       n_colors=None if colors is None else colors.n_colors) as table:
        at = 0
        while at < len(off) - 1:
            end = max(at + 1, int(np.searchsorted(off, int(off[at]) + (1 << 24), side="right")) - 1)
            piece = (np.ascontiguousarray(data[off[at]:off[end]]), (off[at:end + 1] - off[at]).astype(np.uint64))
            answers = ([table.abundance(piece, per_window=True)] if kmer_counts is not None else []) + (
                [table.color_hits(piece, per_window=True)] if colors is not None else [])
            r = answers[0]
            if not (np.array_equal(r.valid, r.kmers) and np.array_equal(r.found, r.kmers)):  # the tigs spell the unitigs' k-mers
                bad = int(np.flatnonzero((r.valid != r.kmers) | (r.found != r.kmers))[0])
                raise SystemExit(f"--query-index-over {what}: tig {at + bad} has {int(r.kmers[bad])} k-mers, of which the index over the "
                                 f"unitigs finds {int(r.found[bad])} ({int(r.valid[bad])} valid): the tigs do not spell the unitigs' k-mers")
            n = r.kmers.astype(np.int64)
            rec = np.repeat(np.arange(at, end), n)
            pos = (off[rec] - off[at]) + (np.arange(len(rec)) - np.repeat(np.cumsum(n) - n, n))  # the start of every window, in the piece
            for out, answer in zip(([weights] if kmer_counts is not None else []) + ([masks] if colors is not None else []), answers):
                out.append(answer.per_window[pos])
            at = end
    return (np.concatenate(weights) if weights else np.zeros(0, np.uint32) if kmer_counts is not None else None,
            np.concatenate(masks) if masks else np.zeros(0, np.uint64) if colors is not None else None)


def _describe_index(index, sparse) -> str:
    """What the `Indexing the ...` lines say of an index: the sparse one's own words, the table in the same terms."""
    i = index.info
    if sparse:
        return i.describe()
    return (f"table index: {i.characters} bases in {i.records} records, 0 anchors, 0 heavy buckets with 0 windows, {i.device_bytes} "
            f"device bytes, {i.device_bytes / i.occurrences if i.occurrences else 0.0:.2f} bytes per k-mer window")


def _query(api, args, store, kmer_counts=None, fastq=(), colors=None, keep_index=False, keep_sparse=False, loaded=None):
    """`--query-fa`: the input's k-mer set (the unitig store) indexed once; one TSV row and one presence line per query record, and
    with `--query-locate-out` (the sparse index: `--query-index-locate-out`) one row per run of located k-mers. kmer_counts (`--query-abundance-out`): the index is weighted with
    them, and one more TSV row, and with `--query-abundance-profile-out` one line of integers, per query record. colors
    (`--query-colors-out`): the index carries their masks, and one more TSV row per query record. keep_index: a table index over
    `store` is handed back open instead of closed (`--count-fa` counts on it); None if the queries asked another kind of index.
    keep_sparse (`--count-index minimizer` on what the queries index): the sparse index is built locating and handed back open.
    With the sparse index (`--query-index-abundance-out`, `--query-index-colors-out`) the same two payloads hang off the
    positions of whatever it indexes, and the same rows are written. loaded (`--index-in`): the sparse index of a file,
    asked as it is and left open; kmer_counts / colors then only say, by not being None, that its weights / colours are asked."""
    import contextlib
    import gzip

    import numpy as np

    def writer(path, mode):
        return gzip.open(path, "w" + mode, compresslevel=args.compression_level) if path.endswith(".gz") else open(path, "w" + mode)

    with contextlib.ExitStack() as stack:
        sparse = args.query_index == "minimizer"
        over = args.query_index_over or "input"
        kept = (keep_index and not sparse and over == "input") or (keep_sparse and sparse)
        hold = (lambda ix: ix) if kept else stack.enter_context  # (a kept index is closed by the caller)
        if loaded is not None:
            index = loaded
        elif sparse or over != "input":  # (the same k-mer set, asked of another index or spelled by the tigs)
            indexed = store if over == "input" else api.read_sequences(args.greedytigs_fa_out if over == "greedytigs" else args.eulertigs_fa_out)
            if sparse and (kmer_counts is not None or colors is not None):  # (payloads by position)
                weights, masks = (kmer_counts, None if colors is None else colors.kmer_colors) if over == "input" else _tig_payloads(
                    api, args, store, indexed, kmer_counts, colors, over)
                index = hold(api.TigIndex.annotated(indexed, args.k, args.query_minimizer_length, args.device, weights=weights,
                                                    colors=masks, n_colors=None if colors is None else colors.n_colors))
            elif sparse:
                index = hold(api.TigIndex(indexed, args.k, args.query_minimizer_length, args.device,
                                          locate=bool(args.query_index_locate_out) or keep_sparse))
            else:
                index = stack.enter_context(api.KmerIndex(indexed, args.k, args.device))
        elif colors is not None:  # (the masks, and the counts too when abundances are asked for)
            index = hold(api.KmerIndex(store, args.k, args.device, locate=bool(args.query_locate_out), weights=kmer_counts,
                                       colors=colors.kmer_colors, n_colors=colors.n_colors))
        elif kmer_counts is None:
            index = hold(api.KmerIndex(store, args.k, args.device, locate=bool(args.query_locate_out)))
        else:
            index = hold(api.KmerIndex(store, args.k, args.device, locate=bool(args.query_locate_out), weights=kmer_counts))
        if loaded is None and (args.query_index is not None or args.query_index_over is not None):
            print(f"Indexing the {over}: {_describe_index(index, sparse)}", file=sys.stderr)
            for what, p in (getattr(index, "payload_info", None) or {}).items():
                print(f"  {what} by position: {p['layout']}, {p['width']} B wide, {p['runs']} runs over {p['windows']} windows, "
                      f"{p['device_bytes']} device bytes", file=sys.stderr)
        tsv = stack.enter_context(writer(args.query_out, "t"))
        presence = stack.enter_context(writer(args.query_presence_out, "b")) if args.query_presence_out else None
        locate_out = args.query_locate_out or args.query_index_locate_out  # (never both: the first is refused with the sparse index)
        located = stack.enter_context(writer(locate_out, "t")) if locate_out else None
        # (the table's flag or the sparse index's, never both: the first is refused with the sparse index, the second without it)
        abundance_out = args.query_abundance_out or args.query_index_abundance_out
        profile_out = args.query_abundance_profile_out or args.query_index_abundance_profile_out
        colors_out = args.query_colors_out or args.query_index_colors_out
        weighed = stack.enter_context(writer(abundance_out, "t")) if kmer_counts is not None else None
        profile = stack.enter_context(writer(profile_out, "b")) if profile_out else None
        coloured = stack.enter_context(writer(colors_out, "t")) if colors is not None else None
        if coloured is not None:
            coloured.write("\t".join(["record", "kmers", "valid", "found"] + args.seq_in) + "\n")
        tsv.write("record\tlength\tkmers\tvalid\tfound\n")
        if weighed is not None:
            weighed.write("record\tkmers\tvalid\tfound\tsum\tmin\tmax\tmean\n")
        if located is not None:
            located.write("record\tqstart\tqend\tstrand\ttarget\ttstart\ttend\tkmers\n")
        for path in args.query_fa:
            t0 = time.perf_counter()
            if path in fastq:
                seqs, names, _ = api.read_fastq(path, args.query_min_base_quality or 0, args.device, named=True)
            else:
                seqs, names = api.read_sequences_named(path)
            if located is not None:  # the counts of the TSV come from the same call
                loc = index.locate(seqs)
                runs, span = loc.runs, loc.runs["kmers"] + np.uint64(args.k - 1)
                located.writelines(f"{names[q]}\t{qs}\t{qe}\t{'-' if s else '+'}\t{t}\t{ts}\t{te}\t{n}\n" for q, qs, qe, s, t, ts, te, n in zip(
                    runs["q_record"].tolist(), runs["q_start"].tolist(), (runs["q_start"] + span).tolist(), runs["strand"].tolist(),
                    runs["t_record"].tolist(), runs["t_start"].tolist(), (runs["t_start"] + span).tolist(), runs["kmers"].tolist()))
            r = index.query(seqs, bits=True) if presence is not None else loc if located is not None else index.query(seqs)
            lengths = np.diff(r.offsets)
            tsv.writelines(f"{name}\t{l}\t{n}\t{v}\t{f}\n"
                           for name, l, n, v, f in zip(names, lengths.tolist(), r.kmers.tolist(), r.valid.tolist(), r.found.tolist()))
            if presence is not None:  # in slices of about 2^24 bases, which bounds the unpacked bits held at once
                at = 0
                while at < len(names):
                    end = max(at + 1, int(np.searchsorted(r.offsets, int(r.offsets[at]) + (1 << 24), side="right")) - 1)
                    presence.write(r.presence_lines(at, end))
                    at = end
            if weighed is not None:
                _write_query_abundance(index, seqs, names, weighed, profile, getattr(r, "valid_bits", None))
            if coloured is not None:
                ch = index.color_hits(seqs)
                coloured.writelines("\t".join([name, str(n), str(v), str(f)] + [str(x) for x in row]) + "\n" for name, n, v, f, row in zip(
                    names, ch.kmers.tolist(), ch.valid.tolist(), ch.found.tolist(), ch.per_color.tolist()))
            valid, found = int(r.valid.sum()), int(r.found.sum())
            print(f"Querying {path}: {len(names)} records, {int(r.kmers.sum())} k-mers, {valid} valid, {found} found "
                  f"({100.0 * found / valid if valid else 0.0:.2f} %) in {time.perf_counter() - t0:.1f} s", file=sys.stderr)
        return index if kept else None


def _count(api, args, store, fastq=(), index=None, keep=False):
    """`--count-fa`: every file is a sample whose k-mers are counted on the k-mers of the unitig store. One table
    index over the store -- `index`, the one the queries left open, else a plain one built here -- and one tally serve all samples in
    turn: add the sample, read the coverage of the store's own records, keep two columns, reset. `--count-out`: one row per record
    of the store, per sample the k-mers it saw at all and the sum of their counts.
    With `--count-index minimizer` the index is a locating sparse one over what `--count-index-over` names -- the
    queries' own if they left it open -- and the tally one counter per window of that text; the coverage is still asked of the store.
    keep (`--correct-fa` follows): a table index is handed back open instead of closed; None if the count took the sparse one."""
    import contextlib

    import numpy as np

    with contextlib.ExitStack() as stack:
        sparse, over, built = args.count_index == "minimizer", args.count_index_over or "input", index is None
        if built and sparse:
            indexed = store if over == "input" else api.read_sequences(args.greedytigs_fa_out if over == "greedytigs" else args.eulertigs_fa_out)
            index = api.TigIndex(indexed, args.k, args.count_minimizer_length, args.device, locate=True)
        elif built:
            index = api.KmerIndex(store, args.k, args.device)
        if sparse or not keep:
            stack.enter_context(index)
        tally = stack.enter_context(api.TigTally(index) if sparse else api.KmerTally(index))
        if built and args.count_index is not None:
            print(f"Indexing the {over} for the count: {_describe_index(index, sparse)}; the tally: {tally.device_bytes} device bytes",
                  file=sys.stderr)
        columns, kmers = [], None
        for path in args.count_fa:
            t0 = time.perf_counter()
            if path in fastq:
                seqs, _, _ = api.read_fastq(path, args.count_min_base_quality or 0, args.device, named=True)  # (masked bases are N)
            else:
                seqs, _ = api.read_sequences_named(path)  # (any characters, as the queries)
            r = tally.add(seqs)
            cov = tally.coverage(store)
            tally.reset()
            if not (np.array_equal(cov.valid, cov.kmers) and np.array_equal(cov.found, cov.kmers)):  # the store is what is indexed
                bad = int(np.flatnonzero((cov.valid != cov.kmers) | (cov.found != cov.kmers))[0])
                raise SystemExit(f"--count-fa {path}: unitig {bad} has {int(cov.kmers[bad])} k-mers, of which the index finds "
                                 f"{int(cov.found[bad])} ({int(cov.valid[bad])} valid): the index does not hold the unitigs")
            kmers = cov.kmers
            columns += [cov.covered, cov.sum]
            valid, found, total = int(r.valid.sum()), int(r.found.sum()), int(kmers.sum())
            print(f"Counting {path}: {len(r.kmers)} records, {int(r.kmers.sum())} k-mers, {valid} valid, {found} found "
                  f"({100.0 * found / valid if valid else 0.0:.2f} %), {int(np.count_nonzero(cov.covered))} of {len(kmers)} unitigs covered, "
                  f"mean depth {int(cov.sum.sum()) / total if total else 0.0:.3f} in {time.perf_counter() - t0:.1f} s", file=sys.stderr)
        with _open_text(args, args.count_out) as f:
            f.write("\t".join(["unitig", "kmers"] + [f"{path}:{what}" for path in args.count_fa for what in ("covered", "sum")]) + "\n")
            rows = np.stack([np.arange(len(kmers), dtype=np.uint64), kmers] + columns, axis=1).tolist() if len(kmers) else []
            f.writelines("\t".join(map(str, row)) + "\n" for row in rows)
        return index if keep and not sparse else None


def _thread(api, args, store, fastq=(), index=None, keep=False):
    """`--thread-fa`: every file's records threaded through the unitig store. One LOCATING index over the store -- `index`,
    the one the queries or the count left open, if it is the kind `--thread-index` names, else one built here -- serves all files in
    turn; the segments of a path are the store's records by number, the `S` names of `--unitigs-gfa-out`. `--thread-gaf-out`: the
    lines of all files one after the other, formatted by the library; `--thread-report-out`: one row per read. With `--index-in`
    (store None) `index` is the file's sparse index and the segments are the records of whatever it indexed, by number; over tigs
    a k-mer that occurs twice is located once, which shortens walks and never makes one wrong. keep: a table index is handed back
    open instead of closed (`--correct-fa` follows), and the file's index always is."""
    import contextlib
    import gzip

    import numpy as np

    with contextlib.ExitStack() as stack:
        sparse = args.thread_index == "minimizer" or store is None
        if index is None:
            index = (api.TigIndex(store, args.k, args.thread_minimizer_length, args.device, locate=True) if sparse
                     else api.KmerIndex(store, args.k, args.device, locate=True))
            print(f"Indexing the input for the threading: {_describe_index(index, sparse)}", file=sys.stderr)
        elif not index.locating or not isinstance(index, api.TigIndex if sparse else api.KmerIndex):
            raise SystemExit("internal error: the index handed to the threading is not the locating index it asked for")
        keep = keep and (store is None or not sparse)
        if not keep:
            stack.enter_context(index)
        gaf = None
        if args.thread_gaf_out:
            out = args.thread_gaf_out
            gaf = stack.enter_context(gzip.open(out, "wb", compresslevel=args.compression_level) if out.endswith(".gz") else open(out, "wb"))
        report = stack.enter_context(_open_text(args, args.thread_report_out)) if args.thread_report_out else None
        if report is not None:
            report.write("file\trecord\tlength\tkmers\tvalid\tfound\twalks\tsteps\tlongest\n")
        for path in args.thread_fa:
            t0 = time.perf_counter()
            if path in fastq:
                seqs, names, _ = api.read_fastq(path, args.thread_min_base_quality or 0, args.device, named=True)
            else:
                seqs, names = api.read_sequences_named(path)
            r = index.thread(seqs, args.thread_min_kmers or 1)
            if gaf is not None:
                gaf.write(r.gaf(names))
            n, w = len(names), r.walks
            record = w["q_record"].astype(np.int64)
            walks, steps = np.bincount(record, minlength=n), np.bincount(record, weights=w["steps"].astype(np.float64), minlength=n).astype(np.int64)
            longest = np.zeros(n, np.uint64)
            np.maximum.at(longest, record, w["kmers"])
            if report is not None:
                columns = [x.tolist() for x in (np.diff(r.offsets), r.kmers, r.valid, r.found, walks, steps, longest)]
                report.writelines("\t".join([path, name] + [str(c[q]) for c in columns]) + "\n" for q, name in enumerate(names))
            whole = int(np.count_nonzero((walks == 1) & (longest == r.kmers) & (r.kmers > 0)))
            r.close()
            print(f"Threading {path}: {n} reads, {whole} threaded end to end, {len(w)} walks, {int(w['steps'].sum())} steps, "
                  f"{int(w['kmers'].sum())} k-mers threaded of {int(r.found.sum())} found in {time.perf_counter() - t0:.1f} s", file=sys.stderr)
        return index if keep and store is not None else None


def _pseudoalign(api, args, store, colors, fastq=(), loaded=None) -> int:
    """`--pseudoalign-fa`: every file is a sample whose reads are pseudoaligned to the colours of the unitig store's k-mers (DESIGN.md
    33). One coloured index over the store -- the table, or with `--pseudoalign-index minimizer` the sparse index with the masks by
    position -- and one aligner serve all samples in turn: align the sample (with its mates), keep the rows, the classes and the
    per-colour sums, reset. Returns 2 where a sample and its mates differ in their number of records. loaded (`--index-in`, DESIGN.md
    35): the coloured sparse index of a file, aligned on as it is and left open; the colours' names are args.seq_in."""
    import contextlib

    import numpy as np

    def read(path):
        if path in fastq:
            seqs, names, _ = api.read_fastq(path, args.pseudoalign_min_base_quality or 0, args.device, named=True)  # (masked bases are N)
            return seqs, names
        return api.read_sequences_named(path)  # (any characters, as the queries)

    with contextlib.ExitStack() as stack:
        sparse = args.pseudoalign_index == "minimizer"
        n_colors = loaded.n_colors if loaded is not None else colors.n_colors
        if loaded is not None:
            index = loaded
        elif sparse:
            index = api.TigIndex.annotated(store, args.k, args.pseudoalign_minimizer_length, args.device, colors=colors.kmer_colors,
                                           n_colors=colors.n_colors)
        else:
            index = api.KmerIndex(store, args.k, args.device, colors=colors.kmer_colors, n_colors=colors.n_colors)
        if loaded is None:
            stack.enter_context(index)
        aligner = stack.enter_context(api.Pseudoaligner(index, args.pseudoalign_permille, args.pseudoalign_over or "found",
                                                        args.pseudoalign_min_kmers or 1))
        if loaded is None:
            print(f"Indexing the input for the pseudoalignment: {_describe_index(index, sparse)}; {colors.n_colors} colours, threshold "
                  f"{args.pseudoalign_permille}/1000 of the {aligner.over} k-mers, at least {aligner.min_kmers}", file=sys.stderr)
        rows = stack.enter_context(_open_text(args, args.pseudoalign_out)) if args.pseudoalign_out else None
        classes_out = stack.enter_context(_open_text(args, args.pseudoalign_classes_out)) if args.pseudoalign_classes_out else None
        if rows is not None:
            rows.write("record\tkmers\tvalid\tfound\tcolors\n")
        if classes_out is not None:
            classes_out.write("sample\tclass\tmask\tcarriers\tfragments\n")
        columns, totals = [], []
        for i, path in enumerate(args.pseudoalign_fa):
            t0 = time.perf_counter()
            seqs, names = read(path)
            mates = None
            if args.pseudoalign_mate_fa:
                mates, mate_names = read(args.pseudoalign_mate_fa[i])
                if len(mate_names) != len(names):
                    print(f"--pseudoalign-fa {path} has {len(names)} records and --pseudoalign-mate-fa {args.pseudoalign_mate_fa[i]} has "
                          f"{len(mate_names)}: mates pair record by record", file=sys.stderr)
                    return 2
            r = aligner.align(seqs, mates)
            cl, tot = aligner.classes(), aligner.totals
            columns += list(aligner.color_reads)
            totals.append(tot)
            aligner.reset()
            if rows is not None:
                masks = r.masks.tolist()
                shown = {m: ",".join(str(c) for c in range(n_colors) if (m >> c) & 1) or "-" for m in set(masks)}
                rows.writelines(f"{name}\t{n}\t{v}\t{f}\t{shown[m]}\n" for name, n, v, f, m in zip(
                    names, r.kmers.tolist(), r.valid.tolist(), r.found.tolist(), masks))
            if classes_out is not None:
                classes_out.writelines(f"{path}\t{c}\t{m:x}\t{b}\t{n}\n" for c, (m, b, n) in enumerate(zip(
                    cl["mask"].tolist(), cl["carriers"].tolist(), cl["fragments"].tolist())))
            largest = int(np.argmax(cl["fragments"])) if len(cl["mask"]) else -1
            print(f"Pseudoaligning {path}{' with ' + args.pseudoalign_mate_fa[i] if mates is not None else ''}: {tot['fragments']} fragments, "
                  f"{tot['eligible']} eligible, {tot['assigned']} assigned, {tot['ambiguous']} ambiguous, {len(cl['mask'])} classes, the largest "
                  + (f"{int(cl['mask'][largest]):x} with {int(cl['fragments'][largest])} fragments" if largest >= 0 else "none")
                  + f" in {time.perf_counter() - t0:.1f} s", file=sys.stderr)
        if args.pseudoalign_summary_out:
            with _open_text(args, args.pseudoalign_summary_out) as f:
                f.write("\t".join(["color"] + [f"{path}:{what}" for path in args.pseudoalign_fa for what in ("assigned", "unique")]) + "\n")
                f.writelines("\t".join([args.seq_in[c]] + [str(int(col[c])) for col in columns]) + "\n" for c in range(n_colors))
                for what in ("fragments", "eligible", "assigned", "ambiguous"):  # (one value per sample: under its first column)
                    f.write("\t".join([f"#{what}"] + [x for tot in totals for x in (str(tot[what]), "-")]) + "\n")
    return 0


def _sequence_bytes(text, n_records, is_fastq):
    """Where the bases of a FASTA / FASTQ text lie: the byte offset of every base, in the order the readers concatenate them (numpy
    int64). FASTA: the content of every line that is neither empty nor a header, less the `\\r`s before its `\\n`. FASTQ: the content of
    line 4 r + 1 of each of the n_records records, less one `\\r`. The readers' line rules, not a parser: the caller
    holds the result against the reader's store."""
    import numpy as np

    a = np.frombuffer(text, np.uint8)
    ends = np.flatnonzero(a == 10)
    if len(a) and (not len(ends) or ends[-1] != len(a) - 1):
        ends = np.append(ends, len(a))  # (a last line without its line end)
    starts = np.concatenate(([0], ends[:-1] + 1)).astype(np.int64) if len(ends) else np.zeros(0, np.int64)
    ends = ends.astype(np.int64)
    if is_fastq:
        starts, ends = starts[1:4 * n_records:4], ends[1:4 * n_records:4].copy()
        cr = (ends > starts) & (a[np.maximum(ends - 1, 0)] == 13)
        ends[cr] -= 1
    else:
        ends = ends.copy()
        while True:
            cr = (ends > starts) & (a[np.maximum(ends - 1, 0)] == 13)
            if not cr.any():
                break
            ends[cr] -= 1
        body = (ends > starts) & (a[np.minimum(starts, max(len(a) - 1, 0))] != ord(">"))
        starts, ends = starts[body], ends[body]
    lengths = ends - starts
    total = int(lengths.sum())
    if not total:
        return np.zeros(0, np.int64)
    first = np.cumsum(lengths) - lengths  # the ordinal of each line's first base
    return np.arange(total, dtype=np.int64) + np.repeat(starts - first, lengths)


def _correct(api, args, store, fastq=(), index=None) -> None:
    """`--correct-fa`: every file's reads corrected against the k-mers of the unitig store. One table index over the
    store -- `index`, the one the queries or the count left open, else a plain one built here -- and one corrector serve all files in
    turn. `--correct-out`: the file's inflated text with exactly the substituted bytes replaced; the bases are found in the text by
    the readers' line rules and held against the reader's store before a byte is written. `--correct-report-out`: one row per read."""
    import contextlib
    import gzip

    import numpy as np

    with contextlib.ExitStack() as stack:
        if index is None:
            index = api.KmerIndex(store, args.k, args.device)
        stack.enter_context(index)
        corrector = stack.enter_context(api.ReadCorrector(index, args.correct_min_solid or 4, args.correct_rounds or 2))
        report = stack.enter_context(_open_text(args, args.correct_report_out)) if args.correct_report_out else None
        if report is not None:
            report.write("file\trecord\tlength\tkmers\tvalid\tfound\tfound_after\tcandidates\tambiguous\tcorrected\tcorrections\n")
        for i, path in enumerate(args.correct_fa):
            t0 = time.perf_counter()
            if path in fastq:
                seqs, names, _ = api.read_fastq(path, 0, args.device, named=True)
            else:
                seqs, names = api.read_sequences_named(path)
            r = corrector.correct(seqs)
            with open(path, "rb") as f:
                text = f.read()
            if text[:2] == b"\x1f\x8b":
                text = gzip.decompress(text)
            data = seqs.arrays()[0]
            where = _sequence_bytes(text, len(names), path in fastq)
            old = np.frombuffer(text, np.uint8)
            if len(where) != len(data) or not np.array_equal(old[where], data):
                raise SystemExit(f"--correct-fa {path}: the bases of the text are not the reader's ({len(where)} against {len(data)})")
            at = where[r.positions.astype(np.int64)]
            new = api.patched_bytes(old[at], r.bases)
            if args.correct_out:
                patched = old.copy()
                patched[at] = new
                out = args.correct_out[i]
                with (gzip.open(out, "wb", compresslevel=args.compression_level) if out.endswith(".gz") else open(out, "wb")) as f:
                    f.write(patched.tobytes())
            if report is not None:
                local = (r.positions - r.offsets[np.searchsorted(r.offsets, r.positions, side="right") - 1]).tolist()
                shown = [f"{p}:{chr(a)}>{chr(b)}" for p, a, b in zip(local, old[at].tolist(), new.tolist())]
                ends = np.cumsum(r.corrected.astype(np.int64)).tolist()
                lengths = np.diff(r.offsets).tolist()
                columns = [x.tolist() for x in (r.kmers, r.valid, r.found, r.found_after, r.candidates, r.ambiguous, r.corrected)]
                report.writelines("\t".join([path, name, str(lengths[q])] + [str(c[q]) for c in columns]
                                            + [",".join(shown[ends[q] - columns[6][q]:ends[q]]) or "-"]) + "\n" for q, name in enumerate(names))
            per_round = [int(x) for x in r.round_corrected[:corrector.rounds]]
            print(f"Correcting {path}: {len(names)} records, {int(r.candidates.sum())} candidates, {'+'.join(map(str, per_round))} = "
                  f"{len(r.positions)} substitutions in {corrector.rounds} rounds, {int(r.ambiguous.sum())} ambiguous, k-mers found "
                  f"{int(r.found.sum())} -> {int(r.found_after.sum())} of {int(r.valid.sum())} valid in {time.perf_counter() - t0:.1f} s",
                  file=sys.stderr)


def _write_query_abundance(index, seqs, names, weighed, profile, valid_bits) -> None:
    """One `--query-abundance-out` row per record of one query file and, if asked for, its `--query-abundance-profile-out` lines.
    valid_bits: those of the file's query if it made them, else None."""
    import numpy as np

    ab = index.abundance(seqs, per_window=profile is not None)
    weighed.writelines(f"{name}\t{n}\t{v}\t{f}\t{s}\t{lo}\t{hi}\t{f'{s / f:.3f}' if f else '-'}\n" for name, n, v, f, s, lo, hi in zip(
        names, ab.kmers.tolist(), ab.valid.tolist(), ab.found.tolist(), ab.sum.tolist(), ab.min.tolist(), ab.max.tolist()))
    if profile is None:
        return
    bits = valid_bits if valid_bits is not None else index.query(seqs, bits=True).valid_bits  # a clear bit: a character outside ACGT
    off, kmers = ab.offsets.astype(np.int64), ab.kmers.astype(np.int64)
    at = 0
    while at < len(names):  # in slices of about 2^24 bases, as the presence lines
        end = max(at + 1, int(np.searchsorted(off, int(off[at]) + (1 << 24), side="right")) - 1)
        n = kmers[at:end]
        rec = np.repeat(np.arange(at, end), n)
        pos = off[rec] + (np.arange(len(rec)) - np.repeat(np.cumsum(n) - n, n))  # the global start of every window of the slice
        invalid = ((bits[pos >> 6] >> (pos & 63).astype(np.uint64)) & np.uint64(1)) == 0
        profile.write(_integer_lines(ab.per_window[pos], n, invalid))
        at = end


if __name__ == "__main__":
    raise SystemExit(main())
