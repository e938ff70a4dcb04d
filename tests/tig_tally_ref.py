"""Tallies by position on the sparse minimizer index (tig_tally_device.hpp) restated in plain Python on top of
tig_locate_ref.TigLocateRef and tig_payload_ref.window_offsets / ordinal. Not a test module.

TigTallyRef(ref) holds the counters as a list of W integers, W the windows of the indexed text. add(query): for every valid found
window, +1 at the ordinal of ref.where(window). coverage(seqs): the counter read at that ordinal, shaped like
kmer_tally_ref.coverage, which stays the arbiter: it knows nothing about positions. counters(): the list.

tally_pair(rng, k) is the generator the GPU test draws its random cases from, and seen_flags() says which of the hazards a case
shows; test_tig_tally_ref.py checks without a GPU that the generator shows all of them at every k the GPU test uses."""
import tig_index_cases as cases
import tig_index_ref as T
import tig_payload_ref as TP
from matchtigs_amd import synth

RUN = 64  # query positions per thread of the add and the gather (kw::RUN)


class TigTallyRef:
    def __init__(self, ref):
        self.ref = ref
        self.win_off = TP.window_offsets(ref.off, ref.k)
        self.windows = self.win_off[-1]
        self.count = [0] * self.windows

    def _walk(self, query, each):
        """kmers / valid / found per query record; each(record, global position, ordinal) per found window."""
        ref, k = self.ref, self.ref.k
        out = {"kmers": [], "valid": [], "found": []}
        base = 0
        for r, s in enumerate(query):
            n = max(0, len(s) - k + 1)
            v = f = 0
            for i in range(n):
                w = s[i:i + k]
                if all(c in T.ACGT for c in w):
                    v += 1
                    t = ref.where(w.upper())
                    if t is not None:
                        f += 1
                        each(r, base + i, TP.ordinal(ref.off, k, t, self.win_off))
            out["kmers"].append(n)
            out["valid"].append(v)
            out["found"].append(f)
            base += len(s)
        return out

    def add(self, query):
        def each(r, p, o):
            self.count[o] += 1

        return self._walk(query, each)

    def coverage(self, seqs):
        hits = [[] for _ in seqs]
        per_window = [0] * sum(len(s) for s in seqs)

        def each(r, p, o):
            hits[r].append(self.count[o])
            per_window[p] = self.count[o]

        out = self._walk(seqs, each)
        out.update(covered=[sum(1 for h in hs if h > 0) for hs in hits], sum=[sum(hs) for hs in hits], max=[max(hs, default=0) for hs in hits],
                   per_window=per_window)
        return out

    def counters(self):
        return list(self.count)

    def reset(self):
        self.count = [0] * self.windows


def first_windows(index, k):
    """(text, off, {canonical k-mer: (ordinal, start) of its first window}, windows) from dictionaries alone (no minimizers)."""
    text, off = "".join(index).upper(), [0]
    for s in index:
        off.append(off[-1] + len(s))
    first, o = {}, 0
    for r in range(len(index)):
        for t in range(off[r], off[r + 1] - k + 1):
            first.setdefault(synth.canonical(text[t:t + k]), (o, t))
            o += 1
    return text, off, first, o


def counters_by_dictionary(index, queries, k):
    """What counters() must hold after adding every record list of `queries`: the count of a class at the ordinal of its first window."""
    _, _, first, windows = first_windows(index, k)
    out = [0] * windows
    for seqs in queries:
        for s in seqs:
            for i in range(len(s) - k + 1):
                w = s[i:i + k]
                if all(c in T.ACGT for c in w) and synth.canonical(w.upper()) in first:
                    out[first[synth.canonical(w.upper())][0]] += 1
    return out


def tally_pair(rng, k):
    """About 40 index records -- ten of tig_index_cases.random_pair's indexes, a poly-A record and a record that repeats an earlier
    one (a class with a later occurrence) -- and the ten queries plus: poly-A and poly-T (a thread merges its hits into one atomic,
    both strands), two one-window records of one class side by side (for k < RUN they share a thread: the run goes on across the
    change of record), the index's own text reverse-complemented (`-` hits) and a record of more than 2 RUN positions."""
    index, query = [], []
    for _ in range(10):
        i, q = cases.random_pair(rng, k)
        index += i
        query += q
    first = cases.dna(rng, k + rng.randint(2, 9))  # (never without a window)
    index = [first] + index + ["A" * (k + 3), first]
    own = "".join(index).upper()
    query += ["A" * (k + 5), "T" * (k + 2)]
    query += ["N" * (-sum(len(s) for s in query) % RUN)]  # (the next record starts a thread's positions)
    query += ["A" * k, "a" * k, synth.revcomp(own[:3 * k + 5]), (own * (2 * RUN // len(own) + 2))[:2 * RUN + k + 7], ""]
    return index, query


SEEN = ("a - hit", "repeated class", "merged hits", "run across records")


def seen_flags(index, query, k):
    """Which hazards of SEEN the case shows, from dictionaries alone: a found window that reads the other strand of its first
    occurrence; a found class with a later occurrence in the index (whose counter must stay 0); two found windows in one thread's
    RUN positions, next to each other among the thread's hits, on one ordinal; ... of which the second lies in another query record."""
    text, off, first, _ = first_windows(index, k)
    later = set()
    seen_first = set()
    for r in range(len(index)):
        for t in range(off[r], off[r + 1] - k + 1):
            x = synth.canonical(text[t:t + k])
            (later if x in seen_first else seen_first).add(x)
    seen = dict.fromkeys(SEEN, False)
    base, last = 0, None  # last: (thread, ordinal, record) of the found window before
    for r, s in enumerate(query):
        for i in range(len(s) - k + 1):
            w = s[i:i + k]
            if not all(c in T.ACGT for c in w):
                continue
            x = synth.canonical(w.upper())
            if x not in first:
                continue
            o, t = first[x]
            seen["a - hit"] |= w.upper() != text[t:t + k]
            seen["repeated class"] |= x in later
            here = ((base + i) // RUN, o, r)
            if last is not None and last[:2] == here[:2]:
                seen["merged hits"] = True
                seen["run across records"] |= last[2] != r
            last = here
        base += len(s)
    return seen


def needed(k):
    """The hazards a case can show at k: two windows of different records lie at least k positions apart, so for k >= RUN no thread
    sees both."""
    return tuple(f for f in SEEN if f != "run across records" or k < RUN)
