"""The thread contract (include/mtg_engine.h) restated in plain Python from strings alone: a dict from every canonical
k-mer of the indexed records to its place, and one step per query window. It knows nothing of runs, scans or how an index is organised.

place(w): for a valid query window w whose class is in the index, (u, i, s): the record u and the offset i in it of the window of that
class at the smallest global position, and s = 0 iff the upper-cased query window equals that index window base by base, else 1.
With W(u) = len(u) - k + 1, a placed window is AT THE TAIL of u iff i == W(u) - 1 (s = 0) or i == 0 (s = 1), and AT THE HEAD iff
i == 0 (s = 0) or i == W(u) - 1 (s = 1). The placed window p of a record goes on the walk of window p - 1 iff that one is placed too and
either it is the next window of the same step -- same u, same s, i one further in the strand's direction -- or the window before is
at the tail of its record and this one at the head of its own, which opens the walk's next step. Every other placed window starts a
walk.

thread(index_seqs, query_seqs, k, min_kmers=1) -> {"kmers", "valid", "found": lists per query record; "walks": list of WALK tuples in
ascending query position; "steps": the flat list of (u << 1) | s}. gaf(...) formats the lines. check(...) holds any such result --
the reference's or the library's -- to what a walk means, from the strings alone."""
from matchtigs_amd import synth

ACGT = frozenset("ACGTacgt")
FIELDS = ("q_record", "q_start", "q_end", "kmers", "steps", "first_step", "path_len", "path_start", "path_end")


def places(index_seqs, k):
    """canonical k-mer -> (record, offset) of the window of its class at the smallest global position"""
    place = {}
    for u, s in enumerate(index_seqs):
        assert all(c in ACGT for c in s), "the index holds ACGT only"
        up = s.upper()
        for i in range(len(up) - k + 1):
            place.setdefault(synth.canonical(up[i:i + k]), (u, i))
    return place


def thread(index_seqs, query_seqs, k, min_kmers=1):
    place = places(index_seqs, k)
    W = [len(s) - k + 1 for s in index_seqs]
    kmers, valid, found, walks, steps = [], [], [], [], []

    def close(walk):
        if walk is not None and walk["kmers"] >= min_kmers:
            span = walk["kmers"] + k - 1
            walks.append((walk["q_record"], walk["q_start"], walk["q_start"] + span, walk["kmers"], len(walk["steps"]), len(steps),
                          sum(W[x >> 1] for x in walk["steps"]) + k - 1, walk["path_start"], walk["path_start"] + span))
            steps.extend(walk["steps"])

    for qr, q in enumerate(query_seqs):
        n = max(0, len(q) - k + 1)
        v = f = 0
        prev = walk = None
        for p in range(n):
            w = q[p:p + k]
            hit = None
            if all(c in ACGT for c in w):
                v += 1
                at = place.get(synth.canonical(w.upper()))
                if at is not None:
                    f += 1
                    u, i = at
                    hit = (u, i, 0 if w.upper() == index_seqs[u][i:i + k].upper() else 1)
            if hit is not None:
                u, i, s = hit
                same_step = prev is not None and prev[0] == u and prev[2] == s and i == (prev[1] - 1 if s else prev[1] + 1)
                next_step = (prev is not None and not same_step and prev[1] == (0 if prev[2] else W[prev[0]] - 1)
                             and i == (W[u] - 1 if s else 0))
                if same_step or next_step:
                    walk["kmers"] += 1
                    if next_step:
                        walk["steps"].append(u << 1 | s)
                else:
                    close(walk)
                    walk = {"q_record": qr, "q_start": p, "kmers": 1, "steps": [u << 1 | s], "path_start": W[u] - 1 - i if s else i}
            else:
                close(walk)
                walk = None
            prev = hit
        close(walk)
        kmers.append(n)
        valid.append(v)
        found.append(f)
    return {"kmers": kmers, "valid": valid, "found": found, "walks": walks, "steps": steps}


def gaf(result, query_names, query_lengths, segment_names=None):
    """The GAF lines of a result, as bytes."""
    lines = []
    for qr, qs, qe, n, n_steps, first, path_len, ps, pe in result["walks"]:
        path = "".join(("<" if x & 1 else ">") + (str(x >> 1) if segment_names is None else segment_names[x >> 1])
                       for x in result["steps"][first:first + n_steps])
        lines.append(f"{query_names[qr]}\t{query_lengths[qr]}\t{qs}\t{qe}\t+\t{path}\t{path_len}\t{ps}\t{pe}\t{qe - qs}\t{qe - qs}\t255\t"
                     f"cg:Z:{qe - qs}=\tkm:i:{n}\n")
    return "".join(lines).encode()


def found_stretches(index_seqs, query, k):
    """The maximal stretches of found windows of one query record, from a set of canonical k-mers alone."""
    have = {synth.canonical(s[i:i + k].upper()) for s in index_seqs for i in range(len(s) - k + 1)}
    n, inside = 0, False
    for p in range(max(0, len(query) - k + 1)):
        w = query[p:p + k]
        hit = all(c in ACGT for c in w) and synth.canonical(w.upper()) in have
        n += hit and not inside
        inside = hit
    return n


def check(index_seqs, query_seqs, k, result, min_kmers=1, unitigs=False):
    """What a result must satisfy whoever made it: (1) every walk's path, cut at [path_start, path_end), spells the query bases
    [q_start, q_end); (2) consecutive steps overlap in k - 1 bases; (3) per record the walks are disjoint and ascend, their steps
    follow each other in the step array, and at min_kmers <= 1 their k-mers sum to `found`; (4) no two query-adjacent walks could
    have been one; (5) unitigs=True: a record has as many walks as maximal stretches of found windows."""
    walks, steps = result["walks"], result["steps"]
    next_step, per_record = 0, {}
    for w in walks:
        qr, qs, qe, n, n_steps, first, path_len, ps, pe = w
        assert n >= max(1, min_kmers) and n_steps >= 1 and qe == qs + n + k - 1 and pe == ps + (qe - qs) and first == next_step, w
        next_step += n_steps
        path = ""
        for x in steps[first:first + n_steps]:
            s = index_seqs[x >> 1].upper()
            s = synth.revcomp(s) if x & 1 else s
            assert len(s) >= k, w
            if path:
                assert path[-(k - 1):] == s[:k - 1] if k > 1 else True, (w, "steps do not overlap")
                path += s[k - 1:]
            else:
                path = s
        assert len(path) == path_len and pe <= path_len, (w, len(path))
        assert path[ps:pe] == query_seqs[qr][qs:qe].upper(), (w, "the path does not spell the query")
        per_record.setdefault(qr, []).append(w)
    assert next_step == len(steps)
    assert [w[0] for w in walks] == sorted(w[0] for w in walks)
    for qr, ws in per_record.items():
        for a, b in zip(ws, ws[1:]):
            assert a[1] + a[3] <= b[1], (a, b, "walks overlap or descend")
            if a[1] + a[3] == b[1]:  # query-adjacent: a ends at its path's end and b starts at its path's start -> they continue
                assert not (a[8] == a[6] and b[7] == 0), (a, b, "two walks that continue each other")
    if min_kmers <= 1:
        for qr in range(len(query_seqs)):
            assert sum(w[3] for w in per_record.get(qr, [])) == result["found"][qr], qr
        if unitigs:
            for qr, q in enumerate(query_seqs):
                assert len(per_record.get(qr, [])) == found_stretches(index_seqs, q, k), (qr, "a walk broke inside a stretch of found windows")
