"""Independent restatement of the unitig bubble contract, with dicts and strings, on top of unitig_links_ref.py and
compact_ref.py, for the tests of api.unitig_bubbles and `--bubbles-out`. Slow (small inputs only). Not a test module.

Oriented unitig 2u is record u as written, 2u + 1 its reverse complement; tail(o) / head(o) are the first / last k - 1 bases of
seq(o), n(u) = len - k + 1. Unitig u is a CANDIDATE ARM iff n(u) < L and, with x = tail(2u) and y = head(2u), none of x = rc(x),
y = rc(y), x = y, x = rc(y) holds. Its key is the smaller of (x, y) and (rc(y), rc(x)); the candidates of one key are a bundle, a
bundle of two or more a BUBBLE. Arm a is better than b iff kc[a] n(b) > kc[b] n(a), on equality the smaller unitig; the best arm r
is the reference arm. Arm a has strand 0 (+) iff (tail(2a), head(2a)) == (tail(2r), head(2r)), else 1 (-), and is read as the
oriented unitig 2a + strand. Bubbles are numbered by their smallest unitig; inside one, r is arm 0 and the others ascend by unitig.
Against R = seq(2r) the arm A has suffix s = the longest common suffix (at most min(|R|, |A|)), prefix p = the longest common
prefix (at most min(|R|, |A|) - s), ref = R[p : |R| - s], alt = A[p : |A| - s], pos = p, differences = the differing positions of
ref and alt where their lengths agree, else 0. carried[arm][c] = the arm's k-mers whose mask has bit c.
"""
from __future__ import annotations

import compact_ref as R
import unitig_links_ref as LR

U32_FIELDS = ("arm_unitig", "arm_kmers", "prefix", "suffix", "differences")
FIELDS = ("arm_off", "arm_unitig", "arm_strand", "arm_kmers", "arm_abundance", "prefix", "suffix", "differences")


def ends(seqs, k, o):
    s = LR.oriented(seqs, o)
    return s[:k - 1], s[len(s) - (k - 1):]


def candidate(seqs, k, u, L):
    x, y = ends(seqs, k, 2 * u)
    if len(seqs[u]) - k + 1 >= L:
        return False
    return not (x == R.revcomp(x) or y == R.revcomp(y) or x == y or x == R.revcomp(y))


def allele(ref_seq, arm_seq):
    """-> (prefix, suffix, differences): the suffix first, so that an indel inside a run is left-aligned."""
    short = min(len(ref_seq), len(arm_seq))
    s = 0
    while s < short and ref_seq[len(ref_seq) - 1 - s] == arm_seq[len(arm_seq) - 1 - s]:
        s += 1
    p = 0
    while p < short - s and ref_seq[p] == arm_seq[p]:
        p += 1
    ref, alt = ref_seq[p:len(ref_seq) - s], arm_seq[p:len(arm_seq) - s]
    return p, s, sum(a != b for a, b in zip(ref, alt)) if len(ref) == len(alt) else 0


def kind_of(ref, alt):
    if not ref and not alt:
        return "identical"
    if not alt:
        return "del"
    if not ref:
        return "ins"
    if len(ref) == len(alt):
        return "snp" if len(ref) == 1 else "mnp"
    return "complex"


def bubbles_of_sequences(seqs, k, L, kc=None, kmer_colors=None, n_colors=0):
    """-> {field: list for every field of FIELDS, "carried": [[per colour] per arm] or None, "kinds": [...], "alleles": [(ref, alt)]}.
    kinds has "ref" and alleles (".", ".") for arm 0 of a bubble."""
    seqs = [s.upper() for s in seqs]
    n = [len(s) - k + 1 for s in seqs]
    weight = n if kc is None else [int(x) for x in kc]
    bundles = {}
    for u in range(len(seqs)):
        if candidate(seqs, k, u, L):
            x, y = ends(seqs, k, 2 * u)
            bundles.setdefault(min((x, y), (R.revcomp(y), R.revcomp(x))), []).append(u)  # (u ascends: every list is sorted)
    first_kmer = [0]
    for m in n:
        first_kmer.append(first_kmer[-1] + m)
    out = {f: [] for f in FIELDS}
    out["arm_off"].append(0)
    out["carried"] = None if kmer_colors is None else []
    out["kinds"], out["alleles"] = [], []
    for members in sorted((m for m in bundles.values() if len(m) >= 2), key=lambda m: m[0]):
        r = members[0]
        for a in members[1:]:
            if weight[a] * n[r] > weight[r] * n[a]:  # (exact: Python integers; a tie keeps the smaller unitig)
                r = a
        ref_seq = seqs[r]
        for a in [r] + [m for m in members if m != r]:
            strand = 0 if ends(seqs, k, 2 * a) == ends(seqs, k, 2 * r) else 1
            assert ends(seqs, k, 2 * a + strand) == ends(seqs, k, 2 * r)
            arm_seq = LR.oriented(seqs, 2 * a + strand)
            p, s, d = (0, 0, 0) if a == r else allele(ref_seq, arm_seq)
            ref, alt = ref_seq[p:len(ref_seq) - s], arm_seq[p:len(arm_seq) - s]
            for f, v in zip(FIELDS[1:], (a, strand, n[a], weight[a], p, s, d)):
                out[f].append(v)
            out["kinds"].append("ref" if a == r else kind_of(ref, alt))
            out["alleles"].append((".", ".") if a == r else (ref, alt))
            if kmer_colors is not None:
                masks = [int(x) for x in kmer_colors[first_kmer[a]:first_kmer[a + 1]]]
                out["carried"].append([sum(1 for x in masks if x >> c & 1) for c in range(n_colors)])
        out["arm_off"].append(len(out["arm_unitig"]))
    return out


def popped_arms(b):
    """What one round of DESIGN.md 25 at ratio 1 pops of these bubbles: every arm but the best."""
    return len(b["arm_unitig"]) - (len(b["arm_off"]) - 1)


def calls(b, seqs):
    """The calls free of numbering and strand: a sorted list of (kind, ref, alt, the reference arm's record), every call read in
    the canonical orientation of the reference arm's record (the smaller of the record and its reverse complement)."""
    out = []
    for i in range(len(b["arm_off"]) - 1):
        lo, hi = b["arm_off"][i], b["arm_off"][i + 1]
        rec = seqs[b["arm_unitig"][lo]].upper()
        for a in range(lo + 1, hi):
            ref, alt = b["alleles"][a]
            if R.revcomp(rec) < rec:
                out.append((b["kinds"][a], R.revcomp(ref), R.revcomp(alt), R.revcomp(rec)))
            else:
                out.append((b["kinds"][a], ref, alt, rec))
    return sorted(out)


def bubbles_tsv(b, names=None) -> str:
    """`--bubbles-out`: one row per arm; mean = abundance / kmers with one decimal, rounded half up in integers; arm 0 has
    `ref . . . 0`; an empty allele is `-`; one column per colour with the carried k-mers."""
    n_colors = 0 if b["carried"] is None else (len(b["carried"][0]) if b["carried"] else len(names or ()))
    head = "bubble\tarm\tunitig\tstrand\tkmers\tabundance\tmean\ttype\tpos\tref\talt\tdifferences"
    head += "".join("\t" + x for x in (names if names is not None else [f"c{c}" for c in range(n_colors)]))
    rows = [head + "\n"]
    for i in range(len(b["arm_off"]) - 1):
        for j, a in enumerate(range(b["arm_off"][i], b["arm_off"][i + 1])):
            ref, alt = b["alleles"][a]
            row = f"{i}\t{j}\t{b['arm_unitig'][a]}\t{'-' if b['arm_strand'][a] else '+'}\t{b['arm_kmers'][a]}\t{b['arm_abundance'][a]}\t"
            row += f"{LR.km_text(b['arm_abundance'][a], b['arm_kmers'][a])}\t{b['kinds'][a]}\t{'.' if j == 0 else b['prefix'][a]}\t"
            row += f"{ref or '-'}\t{alt or '-'}\t{b['differences'][a]}"
            if b["carried"] is not None:
                row += "".join(f"\t{x}" for x in b["carried"][a])
            rows.append(row + "\n")
    return "".join(rows)


def describe(b) -> str:
    kinds = b["kinds"]
    sizes = [y - x for x, y in zip(b["arm_off"], b["arm_off"][1:])]
    return (f"{len(sizes)} bubbles, {len(kinds)} arms: {kinds.count('snp')} snp, {kinds.count('mnp')} mnp, {kinds.count('ins')} ins, "
            f"{kinds.count('del')} del, {kinds.count('complex')} complex; the largest has {max(sizes, default=0)} arms")
