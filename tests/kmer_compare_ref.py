"""The k-mer set comparison restated in a few lines of Python over sets and Counters of canonical strings: what the
GPU result (mtg_kmer_comparison) is held to, field by field, the witnesses included."""
from collections import Counter

from matchtigs_amd.synth import canonical, revcomp

NONE = 2 ** 64 - 1


def windows(seqs, k):
    """(record, position, canonical k-mer) of every window of length k inside one record, in (record, position) order."""
    return [(r, p, canonical(s.upper()[p:p + k])) for r, s in enumerate(seqs) for p in range(len(s) - k + 1)]


def compare(a, b, k) -> dict:
    wa, wb = windows(a, k), windows(b, k)
    ca, cb = Counter(x for _, _, x in wa), Counter(x for _, _, x in wb)
    fa = next(((r, p) for r, p, x in wa if x not in cb), (NONE, NONE))
    fb = next(((r, p) for r, p, x in wb if x not in ca), (NONE, NONE))
    return {
        "records_a": len(a), "records_b": len(b),
        "characters_a": sum(map(len, a)), "characters_b": sum(map(len, b)),
        "occurrences_a": len(wa), "occurrences_b": len(wb),
        "distinct_a": len(ca), "distinct_b": len(cb),
        "common": len(ca.keys() & cb.keys()), "only_in_a": len(ca.keys() - cb.keys()), "only_in_b": len(cb.keys() - ca.keys()),
        "first_only_in_a_record": fa[0], "first_only_in_a_pos": fa[1],
        "first_only_in_b_record": fb[0], "first_only_in_b_pos": fb[1],
    }


def kinds(seqs, k) -> dict:
    """What a case exercises: a k-mer that occurs twice in the same orientation, one that occurs in both orientations, a palindrome."""
    seen, out = {}, {"repeat": False, "rc_repeat": False, "palindrome": False}
    for _, _, x in [(r, p, s.upper()[p:p + k]) for r, s in enumerate(seqs) for p in range(len(s) - k + 1)]:
        if x == revcomp(x):
            out["palindrome"] = True
            continue
        c = canonical(x)
        if c in seen:
            out["repeat" if (x == c) in seen[c] else "rc_repeat"] = True
        seen.setdefault(c, set()).add(x == c)
    return out
