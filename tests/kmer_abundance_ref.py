"""The weighted k-mer index's contract (kmer_query_device.hip) restated in plain Python on top of abundance_ref.py and
kmer_query_ref.py: string windows, synth.canonical, dictionaries. Independent of the device code; slow (small inputs only). Not a test
module.

window_counts(seqs, reads, k): per window of seqs, in window order, the abundance of its k-mer in reads -- what
compact_unitigs_counted(reads, k, m, kmer_counts=True) returns for its own store.
class_weights(index, weights, k): canonical k-mer -> the weight of its first window in window order (a record shorter than k has no
window, so it shifts nothing).
abundance(index, weights, query, k): per query record kmers / valid / found (kmer_query_ref.query) and sum / min / max over the found
windows, all 0 where nothing is found; per_window over the global base positions of the query, 0 wherever no found window starts."""
from matchtigs_amd import synth

import abundance_ref as A
import kmer_query_ref as Q


def windows(seqs, k):
    """The windows of the records in window order, upper-cased."""
    return [s[i:i + k].upper() for s in seqs for i in range(len(s) - k + 1)]


def window_counts(seqs, reads, k):
    count = A.abundances(reads, k)
    return [count.get(synth.canonical(w), 0) for w in windows(seqs, k)]


def class_weights(index, weights, k):
    ws = windows(index, k)
    if len(ws) != len(weights):
        raise ValueError(f"{len(weights)} weights for {len(ws)} windows")
    out = {}
    for w, x in zip(ws, weights):
        out.setdefault(synth.canonical(w), int(x))  # the first occurrence wins
    return out


def abundance(index, weights, query, k):
    weight = class_weights(index, weights, k)
    out = Q.query(set(weight), query, k)
    out = {f: out[f] for f in ("kmers", "valid", "found")}
    out.update(sum=[], min=[], max=[], per_window=[0] * sum(len(s) for s in query))
    base = 0
    for s in query:
        hits = []
        for i in range(len(s) - k + 1):
            w = s[i:i + k]
            if all(c in Q.ACGT for c in w) and synth.canonical(w.upper()) in weight:
                hits.append(weight[synth.canonical(w.upper())])
                out["per_window"][base + i] = hits[-1]
        out["sum"].append(sum(hits))
        out["min"].append(min(hits, default=0))
        out["max"].append(max(hits, default=0))
        assert len(hits) == out["found"][len(out["sum"]) - 1]
        base += len(s)
    return out


def profile_line(result, query, valid_bits, i, k):
    """The `--query-abundance-profile-out` line of record i: the weight per window, 0 absent, - invalid."""
    base = sum(len(s) for s in query[:i])
    return " ".join("-" if not (valid_bits[p >> 6] >> (p & 63)) & 1 else str(result["per_window"][p])
                    for p in range(base, base + result["kmers"][i]))


def reads_case():
    """The input the compaction tests share, that of test_abundance_cli.py -- a 600-base genome, 40 reads of 150 bases from either
    strand with about 1 % substitutions, lower case here and there -- plus one fully periodic record (period 9 < k = 21: every one
    of its k-mers repeats, and they close a walk) -> (genome, reads)."""
    import numpy as np

    rng = np.random.default_rng(3)
    genome = synth.random_genome(600, seed=77, haplotypes=1)[0]
    out = []
    for i in range(40):
        at = int(rng.integers(0, 600 - 150 + 1))
        r = list(genome[at:at + 150])
        for j in np.flatnonzero(rng.random(150) < 0.01):
            r[j] = "ACGT"[("ACGT".index(r[j]) + int(rng.integers(1, 4))) % 4]
        r = "".join(r)
        r = synth.revcomp(r) if rng.random() < 0.5 else r
        out.append(r.lower() if i % 7 == 0 else r)
    out.append("ACCGTTAGC" * 12)
    return genome, out
