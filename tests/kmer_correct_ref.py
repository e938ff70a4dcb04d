"""Read correction against a solid k-mer set (kmer_correct_device.hpp) restated in plain Python: a set of canonical
k-mers, string windows, Python integers. Independent of the device code; slow (small inputs only). Not a test module.

The rule (include/mtg_engine.h states it too). The SOLID SET is a set of canonical k-mers. A record x[0..n) has the windows
i = 0 .. n - k. A base is GOOD iff it is one of ACGTacgt. A window is VALID iff all its k bases are good and PRESENT iff it is valid and
its canonical form (case folded) is in the set. cover(p) = the valid windows i with max(0, p - k + 1) <= i <= min(p, n - k).
One round, every decision against the round's input text, all substitutions applied together afterwards:
  1. p is a CANDIDATE iff x[p] is good, cover(p) is not empty and no window of cover(p) is present;
  2. for a candidate and each of the three bases b != x[p] (as upper case), S(p, b) = the windows of cover(p) that are in the set when
     x[p] alone is replaced by b;
  3. best = max S(p, b), need = min(W, |cover(p)|): best < need -> nothing; two or more b with S = best -> AMBIGUOUS, nothing;
     else x[p] becomes that b (in the case of the letter it replaces).
Round r + 1 runs on round r's output; R rounds in all (a round without a substitution ends them: the later ones would be identical).
Note. A substituted position is covered by a present window from then on, and is never a candidate again, PROVIDED no other
substitution of the same round lies within k - 1 of it: two such substitutions are each scored against the other's old base, and the
windows that hold both may be solid with neither pair. Then a position can be substituted again. The substitutions reported are the
positions whose final base differs from the input's, with that base; round_corrected counts every substitution made.

solid_set(index, k): the canonical k-mers of the sequences.
correct(solid, k, reads, min_solid=4, rounds=2): what api.ReadCorrector.correct answers, as a dict of lists (memo: see in_set).
report_lines(path, names, reads, result): the rows of --correct-report-out."""
from matchtigs_amd import synth

GOOD = frozenset("ACGTacgt")


def solid_set(index, k):
    return {synth.canonical(s.upper()[p:p + k]) for s in index for p in range(len(s) - k + 1)}


def in_set(solid, w, memo=None):
    """The window w (good bases only) is in the set. memo: a dict of the caller's that remembers the answers for ONE solid set."""
    if memo is None:
        return synth.canonical(w.upper()) in solid
    hit = memo.get(w)
    if hit is None:
        hit = memo[w] = synth.canonical(w.upper()) in solid
    return hit


def windows(solid, k, x, memo=None):
    """(valid, present): one bool per window of x."""
    valid = [all(c in GOOD for c in x[i:i + k]) for i in range(len(x) - k + 1)]
    present = [v and in_set(solid, x[i:i + k], memo) for i, v in enumerate(valid)]
    return valid, present


def one_round(solid, k, x, min_solid, memo=None):
    """One round on the record x -> (candidates, ambiguous, substitutions): positions, positions, {position: upper-case base}."""
    n = len(x)
    valid, present = windows(solid, k, x, memo)
    candidates, ambiguous, subs = [], [], {}
    for p in range(n):
        cover = [i for i in range(max(0, p - k + 1), min(p, n - k) + 1) if valid[i]]
        if x[p] not in GOOD or not cover or any(present[i] for i in cover):
            continue
        candidates.append(p)
        score = {}
        for b in "ACGT":
            if b == x[p].upper():
                continue
            y = x[:p] + b + x[p + 1:]
            score[b] = sum(in_set(solid, y[i:i + k], memo) for i in cover)
        best = max(score.values())
        if best < min(min_solid, len(cover)):
            continue
        winners = [b for b in "ACGT" if score.get(b) == best]
        if len(winners) > 1:
            ambiguous.append(p)
        else:
            subs[p] = winners[0]
    return candidates, ambiguous, subs


def patched(x, subs):
    """x with the substitutions {position: upper-case base} applied; a replacement takes the case of the letter it replaces."""
    s = list(x)
    for p, b in subs.items():
        s[p] = b.lower() if s[p].islower() else b
    return "".join(s)


def correct(solid, k, reads, min_solid=4, rounds=2, memo=None):
    if min_solid < 1 or not 1 <= rounds <= 8:
        raise ValueError("a bad parameter")
    out = {f: [] for f in ("kmers", "valid", "found", "found_after", "candidates", "ambiguous", "corrected")}
    out.update(positions=[], bases=[], round_corrected=[0] * 8, texts=[], substitutions=[])
    start = 0
    for x in reads:
        valid, present = windows(solid, k, x, memo)
        text, all_subs, first_candidates, last_ambiguous = x, {}, 0, 0
        for r in range(rounds):
            candidates, ambiguous, subs = one_round(solid, k, text, min_solid, memo)
            if r == 0:
                first_candidates = len(candidates)
            last_ambiguous = len(ambiguous)
            out["round_corrected"][r] += len(subs)
            if not subs:
                break  # (every later round would be this one again)
            all_subs.update(subs)  # (a position substituted again -- see the note below -- keeps its last base)
            text = patched(text, subs)
        all_subs = {p: b for p, b in all_subs.items() if b != x[p].upper()}  # (... and may have got its first one back)
        for f, v in (("kmers", len(valid)), ("valid", sum(valid)), ("found", sum(present)), ("found_after", sum(windows(solid, k, text, memo)[1])),
                     ("candidates", first_candidates), ("ambiguous", last_ambiguous), ("corrected", len(all_subs))):
            out[f].append(v)
        for p in sorted(all_subs):
            out["positions"].append(start + p)
            out["bases"].append(all_subs[p])
        out["substitutions"].append([(p, x[p], text[p]) for p in sorted(all_subs)])
        out["texts"].append(text)
        start += len(x)
    return out


def report_lines(path, names, reads, result):
    lines = ["file\trecord\tlength\tkmers\tvalid\tfound\tfound_after\tcandidates\tambiguous\tcorrected\tcorrections"]
    for r, (name, x) in enumerate(zip(names, reads)):
        subs = ",".join(f"{p}:{a}>{b}" for p, a, b in result["substitutions"][r]) or "-"
        lines.append("\t".join([path, name, str(len(x))] + [str(result[f][r]) for f in (
            "kmers", "valid", "found", "found_after", "candidates", "ambiguous", "corrected")] + [subs]))
    return lines


# ---- the worked example of DESIGN.md 34 ----
EXAMPLE_K = 4
EXAMPLE_INDEX = ["ACGTTGCATGGACCTA"]
# (read, valid, found, candidates, then per W in (4, 2, 1): (substitutions as "pos:X>Y", found_after)); R = 1
EXAMPLE_ROWS = [
    ("ACGTTGCATGG", 8, 8, 0, {4: ([], 8), 2: ([], 8), 1: ([], 8)}),
    ("ACGTAGCATGG", 8, 4, 1, {4: (["4:A>T"], 8), 2: (["4:A>T"], 8), 1: (["4:A>T"], 8)}),
    ("TCGTTGCATGG", 8, 7, 1, {4: (["0:T>A"], 8), 2: (["0:T>A"], 8), 1: (["0:T>A"], 8)}),
    ("CCATGCTACGT", 8, 4, 1, {4: (["6:T>A"], 8), 2: (["6:T>A"], 8), 1: (["6:T>A"], 8)}),
    ("ACGTAGCTTGGACC", 11, 4, 4, {4: ([], 4), 2: (["4:A>T", "6:C>G", "7:T>A"], 8), 1: (["4:A>T", "5:G>C", "6:C>G", "7:T>A"], 6)}),
    ("ACGTAGCANGGACC", 7, 3, 4, {4: (["4:A>T"], 7), 1: (["4:A>T", "6:C>G"], 6)}),
    ("GGGGGGG", 4, 0, 7, {4: ([], 0), 2: ([], 0), 1: ([], 0)}),
    ("ACG", 0, 0, 0, {4: ([], 0), 2: ([], 0), 1: ([], 0)}),
    ("", 0, 0, 0, {4: ([], 0), 2: ([], 0), 1: ([], 0)}),
]
