"""The unitig bubble contract on the CPU: the restatement (unitig_bubbles_ref.py) against expectations derived by
hand from bubble_ref.hand_cases' parts at k = 11, against bubble_ref's popping on the 300 fuzz inputs, what those inputs hold, the
TSV byte for byte, api.UnitigBubbles on given arrays, the flag rules of the CLI (argparse, before any GPU call) and the declarations."""
import random
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import bubble_ref as B
import compact_ref as R
import unitig_bubbles_ref as UB

ROOT = Path(__file__).resolve().parent.parent
K = 11


def _dna(rng):
    return lambda n: "".join(rng.choice("ACGT") for _ in range(n))


@pytest.fixture(scope="module")
def cases():
    rng = random.Random(25)
    return B.hand_cases(rng, _dna(rng), K)


def _unitigs(records, k=K):
    """The unitigs of the records as the compaction writes them, with their abundance sums."""
    out = B.compact_simplified(records, k)
    return out[0], out[3]["unitig_sums"]


def _bubbles(records, L, k=K):
    seqs, kc = _unitigs(records, k)
    return seqs, UB.bubbles_of_sequences(seqs, k, L, kc)


def _calls(b):
    """(kind, pos, ref, alt, differences) of every non-reference arm, in order."""
    return [(b["kinds"][a], b["prefix"][a], *b["alleles"][a], b["differences"][a]) for a in range(len(b["kinds"])) if b["kinds"][a] != "ref"]


def _either_strand(x, y):
    """{(ref, alt)} as the pair reads on the two strands."""
    return {(x, y), (R.revcomp(x), R.revcomp(y))}


def test_a_snp_seen_once(cases):
    p = cases["_parts"]
    seqs, b = _bubbles(cases["snp_tie"][0], K + 1)
    assert len(seqs) == 4 and b["arm_off"] == [0, 2] and b["arm_kmers"] == [K, K] and b["arm_abundance"] == [K, K]
    assert b["arm_unitig"][0] < b["arm_unitig"][1]  # means 1 : 1, the smaller unitig is the reference
    (kind, pos, ref, alt, d), = _calls(b)
    assert (kind, pos, d) == ("snp", K - 1, 1)
    assert {ref, alt} in ({p["g"][p["p"]], p["snp"][K - 1]}, {R.revcomp(p["g"][p["p"]]), R.revcomp(p["snp"][K - 1])})
    assert b["suffix"][1] == K - 1  # an arm has 2 k - 1 bases: k - 1, the site, k - 1
    assert _bubbles(cases["snp_tie"][0], K)[1]["arm_off"] == [0]  # n = k is not below L = k


def test_a_deletion_both_ways(cases):
    p = cases["_parts"]
    base = p["g"][p["dp"]]
    seqs, b = _bubbles(cases["deletion_goes"][0], K + 1)  # means 2 against 1: g's arm is the reference
    assert b["arm_off"] == [0, 2] and b["arm_kmers"] == [K, K - 1] and b["arm_abundance"] == [2 * K, K - 1]
    (kind, pos, ref, alt, d), = _calls(b)
    assert (kind, pos, alt, d) == ("del", K - 1, "", 0) and ref in (base, R.revcomp(base))
    seqs, b = _bubbles(cases["deletion_wins"][0], K + 1)  # means 1 against 2: the deletion is the reference
    assert b["arm_off"] == [0, 2] and b["arm_kmers"] == [K - 1, K] and b["arm_abundance"] == [2 * (K - 1), K]
    (kind, pos, ref, alt, d), = _calls(b)
    assert (kind, pos, ref, d) == ("ins", K - 1, "", 0) and alt in (base, R.revcomp(base))


def test_three_alleles_hairpin_and_ring(cases):
    p = cases["_parts"]
    seqs, b = _bubbles(cases["three_alleles"][0], K + 1)
    assert b["arm_off"] == [0, 3] and b["kinds"] == ["ref", "snp", "snp"] and b["arm_unitig"][1] < b["arm_unitig"][2]
    assert [c[1] for c in _calls(b)] == [K - 1] * 2 and len({c[2] for c in _calls(b)}) == 1 and len({c[3] for c in _calls(b)}) == 2
    bases = {p["g"][p["p"]], p["snp"][K - 1], p["snp2"][K - 1]}
    got = {_calls(b)[0][2], _calls(b)[0][3], _calls(b)[1][3]}
    assert got in (bases, {R.revcomp(x) for x in bases})
    seqs, b = _bubbles(cases["hairpin"][0], 4 * K)
    assert b["arm_off"] == [0] and b["arm_unitig"] == [] and len(seqs) > 1
    seqs, b = _bubbles(cases["ring_snp"][0], K + 1)
    assert b["arm_off"] == [0, 2] and [c[0] for c in _calls(b)] == ["snp"]


def test_two_changed_bases_are_one_mnp(cases):
    p = cases["_parts"]
    seqs, b = _bubbles([p["g"], p["wide"]], 4 * K)
    assert b["arm_off"] == [0, 2] and b["arm_kmers"] == [2 * K - 1] * 2
    (kind, pos, ref, alt, d), = _calls(b)
    assert (kind, pos, d) == ("mnp", K - 1, 2) and len(ref) == len(alt) == K  # the two bases lie k - 1 apart: k bases from one to the other
    assert (ref, alt) in _either_strand(p["wide"][K - 1:2 * K - 1], p["g"][p["p"] - 5 * K:p["p"] - 4 * K]) | _either_strand(
        p["g"][p["p"] - 5 * K:p["p"] - 4 * K], p["wide"][K - 1:2 * K - 1])
    assert _bubbles([p["g"], p["wide"]], 2 * K - 1)[1]["arm_off"] == [0]  # 2 k - 1 k-mers are not below 2 k - 1


def test_a_long_arm_beside_two_short_ones(cases):
    records = cases["long_arm"][0]
    seqs, b = _bubbles(records, 4 * K)
    assert b["arm_off"] == [0, 3] and sorted(b["arm_kmers"]) == [K, K, K + 7]
    assert sorted(c[0] for c in _calls(b)) == ["complex", "snp"]
    cx = next(c for c in _calls(b) if c[0] == "complex")
    assert (len(cx[2]), len(cx[3]), cx[1], cx[4]) == (1, 8, K - 1, 0)
    seqs, b = _bubbles(records, K + 1)  # the long arm is no candidate: the two short ones are a bubble of their own
    assert b["arm_off"] == [0, 2] and [c[0] for c in _calls(b)] == ["snp"]


def test_a_deletion_inside_a_run_is_left_aligned(cases):
    g = cases["_parts"]["g"]
    at = next(i for i in range(len(g) // 2, len(g)) if "A" not in g[i - 1:i + 1])
    g2 = g[:at] + "AAAA" + g[at:]
    shorter = g[:at] + "AAA" + g[at:]
    seqs, b = _bubbles([g2, g2, shorter[at - 2 * K:at + 2 * K]], 2 * K)
    assert b["arm_off"] == [0, 2], b
    (kind, pos, ref, alt, d), = _calls(b)
    rec = seqs[b["arm_unitig"][0]]
    assert kind == "del" and alt == "" and d == 0 and ref == rec[pos] and rec[pos:pos + 4] == 4 * ref and rec[pos - 1] != ref and rec[pos + 4] != ref
    assert b["arm_kmers"][0] - b["arm_kmers"][1] == 1


def test_the_other_strand_and_the_other_order_give_the_same_calls(cases):
    rng = random.Random(3)
    g = cases["_parts"]["g"]
    snps, _ = B.plant_snps(rng, g, K, 5)
    seqs, kc = _unitigs([g, g] + snps[1:] + [cases["_parts"]["deletion"]])  # 2 : 1 everywhere: no tie
    want = UB.bubbles_of_sequences(seqs, K, 2 * K, kc)
    assert len(want["arm_off"]) - 1 == 6 and sorted(want["kinds"]) == ["del"] + ["ref"] * 6 + ["snp"] * 5
    order = list(range(len(seqs)))
    rng.shuffle(order)
    turned = [R.revcomp(seqs[i]) for i in order]
    got = UB.bubbles_of_sequences(turned, K, 2 * K, [kc[i] for i in order])
    assert UB.calls(got, turned) == UB.calls(want, seqs)
    assert sorted(got["arm_strand"]) == sorted(want["arm_strand"])  # both arms of a bubble are turned: what was + against its reference still is
    assert [order[u] for u in got["arm_unitig"]] != want["arm_unitig"]  # the numbering did change
    assert sorted(order[u] for u in got["arm_unitig"]) == sorted(want["arm_unitig"])


def test_ties_and_a_large_abundance(cases):
    seqs, kc = _unitigs(cases["snp_tie"][0])
    b = UB.bubbles_of_sequences(seqs, K, K + 1, kc)
    u0, u1 = b["arm_unitig"]
    back = UB.bubbles_of_sequences(seqs[::-1], K, K + 1, kc[::-1])  # the ids run the other way: the other arm is the smaller one
    assert back["arm_unitig"] == [len(seqs) - 1 - u1, len(seqs) - 1 - u0]
    big = list(kc)
    big[u1] = (1 << 33) + 6
    b = UB.bubbles_of_sequences(seqs, K, K + 1, big)
    assert b["arm_unitig"] == [u1, u0] and b["arm_abundance"] == [(1 << 33) + 6, K]
    # a product above 2^64 decides: (2^63 + 1) * 10 against 2^63 * 10, which agree in their low 64 bits up to the carry
    two = ["AACC" + "T" + "GGAT", "AACC" + "G" + "GGAT"]
    assert UB.bubbles_of_sequences(two, 5, 9, [1 << 63, (1 << 63) + 1])["arm_unitig"] == [1, 0]
    assert UB.bubbles_of_sequences(two, 5, 9, [(1 << 63) + 1, 1 << 63])["arm_unitig"] == [0, 1]
    assert UB.bubbles_of_sequences(two, 5, 9)["arm_abundance"] == [5, 5]  # nothing counted: one per k-mer


def test_one_fork_two_merges():
    rng = random.Random(8)
    dna = _dna(rng)
    x, y1, y2 = dna(K - 1), dna(K - 1), dna(K - 1)
    seqs = [x + "AC" + y1, x + "CA" + y2, x + "GT" + y1, x + "TG" + y2, x + dna(3 * K) + y2]
    b = UB.bubbles_of_sequences(seqs, K, 2 * K)
    assert b["arm_off"] == [0, 2, 4] and b["arm_unitig"] == [0, 2, 1, 3] and b["kinds"] == ["ref", "mnp", "ref", "mnp"]
    assert b["alleles"][1] == ("AC", "GT") and b["alleles"][3] == ("CA", "TG") and b["differences"] == [0, 2, 0, 2]
    assert b["prefix"] == [0, K - 1, 0, K - 1] and b["arm_strand"] == [0] * 4  # (the long walk between x and y2 is in no bundle)


def test_nothing_to_find():
    for seqs, L in (([], 9), (["AACCTGGAT", "AACCGGGAT"], 1), (["AACCTGGAT", "AACCGGGAT"], 0), (["AACCTGGAT", "AACCGGGAT"], 5), (["AACCTGGAT"], 9)):
        b = UB.bubbles_of_sequences(seqs, 5, L)
        assert b["arm_off"] == [0] and all(b[f] == [] for f in UB.FIELDS[1:]) and UB.describe(b) == "0 bubbles, 0 arms: 0 snp, 0 mnp, 0 ins, 0 del, 0 complex; the largest has 0 arms"
    assert UB.bubbles_of_sequences(["AACCTGGAT", "AACCGGGAT"], 5, 6)["arm_off"] == [0, 2]
    # never an arm: a self-mirror end (ACGT), a loop at one node, a hairpin
    for pair in (["ACGTAGGAT", "ACGTCGGAT"], ["AACCTAACC", "AACCGAACC"], ["AACCTGGTT", "AACCGGGTT"]):
        assert UB.bubbles_of_sequences(pair, 5, 9)["arm_off"] == [0], pair
    same = UB.bubbles_of_sequences(["AACCTGGAT", "ATCCAGGTT"], 5, 9)  # a record and its reverse complement: one key, no difference
    assert same["kinds"] == ["ref", "identical"] and same["arm_strand"] == [0, 1] and same["alleles"][1] == ("", "")


# ---- against bubble_ref, and what the fuzz inputs hold ----
@pytest.fixture(scope="module")
def fuzz():
    """[(the unitigs, k, L, their bubbles, what one round of bubble_ref pops at L)] of the 300 fuzz inputs."""
    out = []
    for records, k, kw in B.fuzz_cases():
        L = kw["pop_bubbles"]
        seqs, kc = _unitigs(records, k)
        out.append((seqs, k, L, UB.bubbles_of_sequences(seqs, k, L, kc), B.compact_simplified(records, k, pop_bubbles=L, rounds=1)[7]["arms"]))
    return out


def test_every_other_arm_is_what_one_round_pops(fuzz):
    assert len(fuzz) == 300
    for i, (seqs, k, L, b, popped) in enumerate(fuzz):
        assert UB.popped_arms(b) == popped, (i, seqs, k, L)


def test_what_the_fuzz_inputs_hold(fuzz):
    sizes = [y - x for _, _, _, b, _ in fuzz for x, y in zip(b["arm_off"], b["arm_off"][1:])]
    kinds = [x for _, _, _, b, _ in fuzz for x in b["kinds"]]
    minus = sum(sum(b["arm_strand"]) for _, _, _, b, _ in fuzz)
    print(len(sizes), sum(1 for s in sizes if s >= 3), minus, {x: kinds.count(x) for x in set(kinds)})
    assert len(sizes) >= 100 and sum(1 for s in sizes if s >= 3) >= 10 and minus >= 50
    assert kinds.count("ins") >= 20 and kinds.count("del") >= 20


# ---- the interface ----
HAND_SEQS = ["AACCTGGAT", "AACCGGGAT", "ATCCGGTT"]  # k = 5: two records from AACC to GGAT and one, shorter, from ATCC to GGTT -- its mirror
HAND_KC = [10, 5, 9]  # means 2, 1 and 2.25: record 2 is the reference, R = ATCCGGTT
HAND_MASKS = [1, 1, 1, 1, 1, 2, 2, 3, 2, 2, 3, 3, 3, 1]
# record 0 reversed is ATCCAGGTT: suffix GGTT, prefix ATCC, an A inserted at 4. Record 1 reversed is ATCCCGGTT: the suffix takes
# CCGGTT, the prefix AT: a C inserted at 2, the first base of R's run CC. Means: 9 / 4 = 2.25 -> 2.3, 10 / 5, 5 / 5.
HAND_TSV = ("bubble\tarm\tunitig\tstrand\tkmers\tabundance\tmean\ttype\tpos\tref\talt\tdifferences\ta.fq\tb.fq\n"
            "0\t0\t2\t+\t4\t9\t2.3\tref\t.\t.\t.\t0\t4\t3\n"
            "0\t1\t0\t-\t5\t10\t2.0\tins\t4\t-\tA\t0\t5\t0\n"
            "0\t2\t1\t-\t5\t5\t1.0\tins\t2\t-\tC\t0\t1\t5\n")


def _as_api(b, k):
    from matchtigs_amd import api

    arrays = {f: np.array(b[f], np.uint32) for f in UB.U32_FIELDS}
    carried = None if b["carried"] is None else np.array(b["carried"], np.uint32).reshape(len(b["arm_unitig"]), -1)
    return api.UnitigBubbles(arm_off=np.array(b["arm_off"], np.uint64), arm_strand=np.array(b["arm_strand"], np.uint8),
                             arm_abundance=np.array(b["arm_abundance"], np.uint64), k=k, carried=carried, **arrays)


def test_the_tsv_byte_for_byte():
    b = UB.bubbles_of_sequences(HAND_SEQS, 5, 6, HAND_KC, HAND_MASKS, 2)
    assert b["arm_unitig"] == [2, 0, 1] and b["arm_strand"] == [0, 1, 1] and b["prefix"] == [0, 4, 2] and b["suffix"] == [0, 4, 6]
    assert b["carried"] == [[4, 3], [5, 0], [1, 5]]
    assert UB.bubbles_tsv(b, ["a.fq", "b.fq"]) == HAND_TSV
    plain = UB.bubbles_of_sequences(HAND_SEQS, 5, 6, HAND_KC)
    assert UB.bubbles_tsv(plain) == "".join(l.rsplit("\t", 2)[0] + "\n" for l in HAND_TSV.splitlines())
    assert UB.describe(b) == "1 bubbles, 3 arms: 0 snp, 0 mnp, 2 ins, 0 del, 0 complex; the largest has 3 arms"


def test_the_dataclass_on_given_arrays(cases):
    from matchtigs_amd import api

    b = UB.bubbles_of_sequences(HAND_SEQS, 5, 6, HAND_KC, HAND_MASKS, 2)
    got = _as_api(b, 5)
    assert len(got) == 1 and got.kinds() == b["kinds"] == ["ref", "ins", "ins"] and got.alleles(HAND_SEQS) == b["alleles"]
    assert got.tsv(HAND_SEQS, 5, ["a.fq", "b.fq"]) == HAND_TSV and got.describe() == UB.describe(b)
    data = np.frombuffer("".join(HAND_SEQS).encode(), np.uint8)
    assert got.tsv((data, np.array([0, 9, 18, 26], np.uint64)), 5, ["a.fq", "b.fq"]) == HAND_TSV
    assert got.tsv(HAND_SEQS, 5).splitlines()[0].endswith("differences\tc0\tc1")
    with pytest.raises(ValueError):
        got.tsv(HAND_SEQS, 6)
    with pytest.raises(ValueError):
        got.tsv(HAND_SEQS, 5, ["a.fq"])
    with pytest.raises(Exception):
        got.prefix = None  # frozen
    # every kind, from the hand cases' worlds
    p = cases["_parts"]
    seqs, kc = _unitigs([p["g"], p["g"], p["snp"], p["insertion"], p["wide"], p["deletion"]])
    b = UB.bubbles_of_sequences(seqs, K, 4 * K, kc)
    assert sorted(set(b["kinds"])) == ["complex", "del", "mnp", "ref", "snp"]
    got = _as_api(b, K)
    assert got.kinds() == b["kinds"] and got.alleles(seqs) == b["alleles"] and got.tsv(seqs, K) == UB.bubbles_tsv(b) and got.describe() == UB.describe(b)
    n_ref, n_alt = got.allele_lengths()
    assert n_ref.tolist() == [0 if x == "." else len(x) for x, _ in b["alleles"]] and n_alt.tolist() == [0 if y == "." else len(y) for _, y in b["alleles"]]
    none = _as_api(UB.bubbles_of_sequences([], 5, 9), 5)
    assert len(none) == 0 and none.kinds() == [] and none.tsv([], 5).count("\n") == 1
    assert none.describe() == "0 bubbles, 0 arms: 0 snp, 0 mnp, 0 ins, 0 del, 0 complex; the largest has 0 arms"


def _cli(*a):
    return subprocess.run([sys.executable, "-m", "matchtigs_amd", *a], capture_output=True, text=True, cwd=str(ROOT), timeout=120)


def test_help_names_the_flags(capsys):
    from matchtigs_amd.__main__ import main

    with pytest.raises(SystemExit) as e:
        main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert "--bubbles-out" in out and "--bubbles-max-kmers" in out


def test_the_flag_rules(tmp_path):
    out = ["--bubbles-out", str(tmp_path / "b.tsv")]
    r = _cli("--fa-in", str(tmp_path / "missing.fa"), "-k", "5", *out, "--bubbles-max-kmers", "1")
    assert r.returncode == 2 and "--bubbles-max-kmers must be >= 2" in r.stderr
    r = _cli("--fa-in", str(tmp_path / "missing.fa"), "-k", "5", "--unitigs-fa-out", str(tmp_path / "u.fa"), "--bubbles-max-kmers", "9")
    assert r.returncode == 2 and "--bubbles-max-kmers needs --bubbles-out" in r.stderr
    r = _cli("--bcalm-in", str(tmp_path / "missing.fa"), "-k", "5", *out)
    assert r.returncode == 2 and "--bubbles-out needs --seq-in or --fa-in" in r.stderr
    r = _cli("--index-in", str(tmp_path / "missing.idx"), *out)
    assert r.returncode == 2 and "--bubbles-out" in r.stderr
    r = _cli("--seq-in", str(tmp_path / "missing.fa"), "-k", "5", *out, "--monochromatic-unitigs")
    assert r.returncode == 2 and "--bubbles-out cannot be combined with --monochromatic-unitigs" in r.stderr


def test_nothing_to_do_counts_the_new_output(product_lib, tmp_path):
    r = _cli("--fa-in", str(tmp_path / "missing.fa"), "-k", "5")
    assert r.returncode == 2 and "nothing to do" in r.stderr
    r = _cli("--fa-in", str(tmp_path / "missing.fa"), "-k", "5", "--bubbles-out", str(tmp_path / "b.tsv"))
    assert r.returncode != 0 and "nothing to do" not in r.stderr and "missing.fa" in r.stderr, r.stderr[-2000:]


def test_headers_compile_as_c_with_the_new_declarations(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "mtg_engine.h"\n'
                   "uint64_t (*a)(const mtg_graph *, const char *, const uint64_t *, uint64_t, uint64_t, uint64_t, const uint64_t *, const uint64_t *,"
                   " uint32_t, int, mtg_unitig_bubble_arrays *) = mtg_unitig_bubbles;\n"
                   "void (*b)(double *) = mtg_last_unitig_bubbles_times;\n"
                   "int main(void){mtg_unitig_bubble_arrays s; uint64_t *o = 0; uint32_t *w = 0; uint8_t *c = 0;"
                   " s.arm_off = o; s.arm_unitig = w; s.arm_strand = c; s.arm_kmers = w; s.arm_abundance = o; s.prefix = w; s.suffix = w;"
                   " s.differences = w; s.carried = w;"
                   " return a && b && sizeof s == 9 * sizeof(void *) && offsetof(mtg_unitig_bubble_arrays, arm_off) == 0"
                   " && offsetof(mtg_unitig_bubble_arrays, arm_strand) == 2 * sizeof(void *)"
                   " && offsetof(mtg_unitig_bubble_arrays, carried) == 8 * sizeof(void *) && !s.carried ? 0 : 1;}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-c", "-o", str(tmp_path / "t.o")], check=True)


def test_the_new_symbols_are_declared():
    import ctypes as C

    from matchtigs_amd import _lib, api

    names = _lib.declared_symbols()
    assert "mtg_unitig_bubbles" in names and "mtg_last_unitig_bubbles_times" in names
    assert C.sizeof(_lib.MtgUnitigBubbleArrays) == 9 * C.sizeof(C.c_void_p)
    assert [f for f, _ in _lib.MtgUnitigBubbleArrays._fields_] == list(UB.FIELDS) + ["carried"]
    for n in ("UnitigBubbles", "unitig_bubbles", "last_unitig_bubbles_times"):
        assert hasattr(api, n), n
    for n in ("Bubbles", "last_bubble_times"):  # DESIGN.md 25's keep their names
        assert hasattr(api, n), n
