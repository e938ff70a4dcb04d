"""The locate contract of the k-mer index (kmer_query_device.hip) restated in plain Python: string windows,
synth.canonical, a dict. It extends kmer_query_ref.py's notions of index, query, window, valid and canonical class.

loc(w): for a valid query window w whose class is in the index, the smallest global start position t, in the index's concatenated
bases, of an index window of that class (index windows lie inside one record). strand(w): + iff the upper-cased query window equals
the index window at t base by base, else -. Window p continues window p - 1 iff both start in the same query record, both are
valid and found, have the same strand, loc(p) = loc(p - 1) + 1 for + or loc(p - 1) - 1 for -, and both locations lie in the same
index record. A run starts at every found window that does not continue its predecessor.

locate(index_seqs, query_seqs, k) -> {"kmers", "valid", "found": lists per query record; "runs": list of RUN tuples
(q_record, q_start, kmers, strand, t_record, t_start) in ascending query position}; strand 0 = +, 1 = -; t_start = the offset in
t_record of the leftmost index base the run covers (for - the location of the run's last window)."""
import bisect

from matchtigs_amd import synth

ACGT = frozenset("ACGTacgt")
FIELDS = ("q_record", "q_start", "kmers", "strand", "t_record", "t_start")


def first_positions(index_seqs, k):
    """canonical k-mer -> the smallest global start position of a window of its class; and the record offsets."""
    first, off = {}, [0]
    for s in index_seqs:
        assert all(c in ACGT for c in s), "the index holds ACGT only"
        u = s.upper()
        for i in range(len(u) - k + 1):
            first.setdefault(synth.canonical(u[i:i + k]), off[-1] + i)  # (positions ascend: the first one seen is the smallest)
        off.append(off[-1] + len(s))
    return first, off


def locate(index_seqs, query_seqs, k):
    first, t_off = first_positions(index_seqs, k)
    text = "".join(index_seqs).upper()

    def record_of(t):  # the index record that holds base t (empty records hold none)
        return bisect.bisect_right(t_off, t) - 1

    kmers, valid, found, runs = [], [], [], []
    for qr, s in enumerate(query_seqs):
        n = max(0, len(s) - k + 1)
        v = f = 0
        prev = None  # (loc, strand) of the window before, if it was found
        for i in range(n):
            w = s[i:i + k]
            hit = None
            if all(c in ACGT for c in w):
                v += 1
                t = first.get(synth.canonical(w.upper()))
                if t is not None:
                    f += 1
                    hit = (t, 0 if w.upper() == text[t:t + k] else 1)
            if hit is not None:
                t, strand = hit
                cont = (prev is not None and prev[1] == strand and t == (prev[0] - 1 if strand else prev[0] + 1)
                        and record_of(t) == record_of(prev[0]))
                if cont:
                    run = runs[-1]
                    run[2] += 1
                    if strand:
                        run[5] -= 1  # the leftmost base moves with the last window
                else:
                    tr = record_of(t)
                    runs.append([qr, i, 1, strand, tr, t - t_off[tr]])
            prev = hit
        kmers.append(n)
        valid.append(v)
        found.append(f)
    return {"kmers": kmers, "valid": valid, "found": found, "runs": [tuple(r) for r in runs]}


def spells(index_seqs, query_seqs, run, k):
    """What a run means: the query bases it covers equal the index bases it covers (case-insensitive; - : the reverse complement)."""
    qr, qs, n, strand, tr, ts = run
    span = n + k - 1
    q = query_seqs[qr][qs:qs + span].upper()
    t = index_seqs[tr][ts:ts + span].upper()
    return len(q) == len(t) == span and q == (synth.revcomp(t) if strand else t)
