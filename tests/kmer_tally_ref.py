"""The k-mer tally's contract (kmer_query_device.hip) restated in plain Python on top of kmer_query_ref.py: string
windows, synth.canonical, a collections.Counter. Independent of the device code; slow (small inputs only). Not a test module.

tally(index_kmers, queries, k): Counter over the canonical k-mers of the valid windows of every record of every query set in
`queries` (a list of record lists: one per add), restricted to index_kmers (kmer_query_ref.index_set) -- repeats count, both strands
fold onto the canonical form, invalid and absent windows add nothing.
coverage(index_kmers, counts, seqs, k): per record of seqs kmers / valid / found (kmer_query_ref.query) and, over the found windows,
covered (those with a count > 0), sum and max of the counts -- all 0 where nothing is found; per_window over the global base
positions of seqs, 0 wherever no found window starts.
count_tsv(unitigs, samples, names, k): the bytes of `--count-out` for the unitigs as written and the samples' records (already
masked), one (covered, sum) column pair per sample."""
import collections

from matchtigs_amd import synth

import kmer_query_ref as Q


def valid_windows(s, k):
    """(start, canonical k-mer) of every window of s that holds ACGT of either case only."""
    for i in range(len(s) - k + 1):
        w = s[i:i + k]
        if all(c in Q.ACGT for c in w):
            yield i, synth.canonical(w.upper())


def tally(index_kmers, queries, k):
    counts = collections.Counter()
    for seqs in queries:
        for s in seqs:
            for _, x in valid_windows(s, k):
                if x in index_kmers:
                    counts[x] += 1
    return counts


def coverage(index_kmers, counts, seqs, k):
    out = Q.query(index_kmers, seqs, k)
    out = {f: out[f] for f in ("kmers", "valid", "found")}
    out.update(covered=[], sum=[], max=[], per_window=[0] * sum(len(s) for s in seqs))
    base = 0
    for r, s in enumerate(seqs):
        hits = []
        for i, x in valid_windows(s, k):
            if x in index_kmers:
                hits.append(counts.get(x, 0))
                out["per_window"][base + i] = hits[-1]
        assert len(hits) == out["found"][r]
        out["covered"].append(sum(1 for h in hits if h > 0))
        out["sum"].append(sum(hits))
        out["max"].append(max(hits, default=0))
        base += len(s)
    return out


def count_tsv(unitigs, samples, names, k):
    index_kmers = Q.index_set(unitigs, k)
    columns = []
    for reads in samples:
        cov = coverage(index_kmers, tally(index_kmers, [reads], k), unitigs, k)
        assert cov["found"] == cov["valid"] == cov["kmers"]
        columns += [cov["covered"], cov["sum"]]
    lines = ["\t".join(["unitig", "kmers"] + [f"{name}:{what}" for name in names for what in ("covered", "sum")])]
    for i, u in enumerate(unitigs):
        lines.append("\t".join(map(str, [i, len(u) - k + 1] + [c[i] for c in columns])))
    return ("\n".join(lines) + "\n").encode()
