"""The unitig component contract on the CPU: the restatement (unitig_components_ref.py) against values derived by
hand from the oriented strings, the filter and its renumbering, the link totals against unitig_links_ref, rings, the flag rules of
the CLI (argparse, before any GPU call) and the declarations."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import ring_cases as RC
import unitig_components_ref as R
import unitig_links_ref as LR
from matchtigs_amd import synth

ROOT = Path(__file__).resolve().parent.parent
K = 5

# name -> (component_of, [(unitigs, kmers, links, dead_ends, irregular) per component]); k = 5, a record of n bases has n - 4 k-mers.
# The links are those worked out in unitig_links_ref.HAND; below, per case, the number of links of every orientation.
HAND_WANT = {
    # 0+ -> 1+, 2+, 3+ (3 links); 1-, 2-, 3- -> 0- (1 each); 0-, 1+, 2+, 3+ end in nothing (0 each). One component of 4 records of 8
    # bases: 16 k-mers, 3 + 1 + 1 + 1 = 6 links, dead ends 0-, 1+, 2+, 3+ = 4, irregular = those four and 0+ (3 links) = 5.
    "fork": ([0, 0, 0, 0], [(4, 16, 6, 4, 5)]),
    # 0+ -> 2+, 1+ -> 2+ (1 each), 2- -> 0-, 1- (2); 0-, 1-, 2+ end in nothing. Bases 7, 7, 6: 3 + 3 + 2 = 8 k-mers, 1 + 1 + 2 = 4
    # links, dead ends 0-, 1-, 2+ = 3, irregular = those and 2- = 4.
    "merge": ([0, 0, 0], [(3, 8, 4, 3, 4)]),
    # 0+ -> 0+ and 0- -> 0-: 9 bases, 5 k-mers, 2 links, both orientations have exactly one: a ring.
    "closed": ([0], [(1, 5, 2, 0, 0)]),
    # 0+ -> 0- once, 0- ends in GACC where nothing starts: 8 bases, 4 k-mers, 1 link, 1 dead end, 1 irregular.
    "hairpin": ([0], [(1, 4, 1, 1, 1)]),
    # 0+ and 1- end in ACGT, where 0- and 1+ start: 2 links each; 0- and 1+ end in nothing. Bases 7 and 6: 3 + 2 = 5 k-mers, 4
    # links, dead ends 0-, 1+ = 2, irregular = all four orientations (2, 0, 0, 2 links).
    "palindrome": ([0, 0], [(2, 5, 4, 2, 4)]),
    # no link at all: 9 bases, 5 k-mers, both orientations are dead ends and irregular.
    "isolated": ([0], [(1, 5, 0, 2, 2)]),
    # ACCGTTA and ACCGAGC both START with ACCG; 0+ ends in GTTA, 1+ in GAGC, 0- = TAACGGT and 1- = GCTCGGT both END in CGGT, and
    # the starts are ACCG, ACCG, TAAC, GCTC: no end equals a start. They share a node and have no link: two components of 3 k-mers.
    "siblings": ([0, 1], [(1, 3, 0, 2, 2), (1, 3, 0, 2, 2)]),
    # records 0..2 are fork without its last record: 0+ -> 1+, 2+ (2), 1-, 2- -> 0- (1 each), 0-, 1+, 2+ dead: 3 records of 8
    # bases = 12 k-mers, 4 links, 3 dead ends, irregular = those and 0+ = 4.
    # record 3 = GGACC / GGTCC: one k-mer; ends GACC, GTCC, starts GGAC, GGTC, nothing else starts or ends so: alone, 2 dead ends.
    # record 4 = ACCGTACCG (the ring of `closed`), record 5 = ACCGTTAGC (`isolated`) starts with ACCG too: 4+ -> 4+, 5+ (2 links);
    # 5+ ends in TAGC: nothing. 4- = CGGTACGGT ends in CGGT, 4- starts with it: 4- -> 4- (1); 5- = GCTAACGGT ends in CGGT: 5- -> 4-
    # (1). 5 + 5 = 10 k-mers, 2 + 1 + 0 + 1 = 4 links, dead end 5+ = 1, irregular = 5+ and 4+ = 2.
    "mixed": ([0, 0, 0, 1, 2, 2], [(3, 12, 4, 3, 4), (1, 1, 0, 2, 2), (2, 10, 4, 1, 2)]),
}


def _tuples(c):
    return list(zip(c["unitigs"], c["kmers"], c["links"], c["dead_ends"], c["irregular"]))


@pytest.mark.parametrize("name", sorted(HAND_WANT))
def test_restatement_equals_the_hand_values(name):
    c = R.components_of_sequences(R.HAND[name], K)
    want_of, want = HAND_WANT[name]
    assert c["component_of"] == want_of and _tuples(c) == want
    assert c["abundance"] == c["kmers"]  # nothing counted: one per k-mer
    assert c["first_unitig"] == [want_of.index(i) for i in range(len(want))]
    assert R.circular(c) == [name == "closed"] * len(want)


def test_the_table_is_complete():
    assert sorted(HAND_WANT) == sorted(R.HAND) and len(HAND_WANT) == 8
    assert R.HAND["siblings"] == ["ACCGTTA", "ACCGAGC"]
    assert R.HAND["mixed"] == ["TTGACGCA", "CGCAATTC", "CGCACTTG", "GGACC", "ACCGTACCG", "ACCGTTAGC"]


def test_abundance_sums_the_callers_values():
    kc = [10, 20, 30, (1 << 40) + 1, 7, 8]
    c = R.components_of_sequences(R.HAND["mixed"], K, kc)
    assert c["abundance"] == [60, (1 << 40) + 1, 15] and c["kmers"] == [12, 1, 10]


@pytest.mark.parametrize("n, kept, renumbered", [
    (2, [0, 1, 2, 4, 5], [0, 0, 0, 1, 1]),   # GGACC (1 k-mer) goes; the ring with its tail becomes component 1
    (10, [0, 1, 2, 4, 5], [0, 0, 0, 1, 1]),  # 10 k-mers is not below 10
    (11, [0, 1, 2], [0, 0, 0]),              # 10 < 11 <= 12
    (12, [0, 1, 2], [0, 0, 0]),
    (13, [], []),                            # nothing is left
    (1, [0, 1, 2, 3, 4, 5], [0, 0, 0, 1, 2, 2]),
])
def test_filter_on_mixed(n, kept, renumbered):
    seqs = R.HAND["mixed"]
    got, keep = R.filtered_sequences(seqs, K, n)
    assert got == [seqs[i] for i in kept] and keep == [i in kept for i in range(6)]
    after = R.components_of_sequences(got, K)
    assert after["component_of"] == renumbered
    # none merge, none split: the kept components' records are those of before, in order
    before = R.components_of_sequences(seqs, K)
    kept_before = [c for c in range(3) if before["kmers"][c] >= n]
    assert _tuples(after) == [_tuples(before)[c] for c in kept_before]
    assert after["first_unitig"] == [kept.index(before["first_unitig"][c]) for c in kept_before]


def test_numbering_follows_the_smallest_unitig():
    """Any order of the records: component_of[0] == 0, first_unitig ascends strictly, and a component's number is its rank by its
    smallest unitig."""
    rng = np.random.default_rng(4)
    base = R.HAND["mixed"] + R.HAND["siblings"] + R.HAND["merge"]
    for _ in range(20):
        seqs = [base[i] for i in rng.permutation(len(base))]
        c = R.components_of_sequences(seqs, K)
        of, first = c["component_of"], c["first_unitig"]
        assert of[0] == 0 and all(a < b for a, b in zip(first, first[1:]))
        assert first == [of.index(i) for i in range(len(first))]
        assert sorted(_tuples(c)) == sorted(_tuples(R.components_of_sequences(base, K)))


@pytest.mark.parametrize("k", [5, 31])
def test_link_totals_and_g_seq(k):
    ug = synth.g_seq(400 if k == 5 else 12000, seed=3, k=k)
    off, to = LR.links_of_sequences(ug.unitigs, k)
    c = R.components_of_sequences(ug.unitigs, k)
    assert sum(c["links"]) == len(to) and sum(c["unitigs"]) == len(ug.unitigs)
    assert sum(c["kmers"]) == sum(len(s) - k + 1 for s in ug.unitigs)
    assert sum(c["dead_ends"]) == sum(1 for a, b in zip(off, off[1:]) if a == b)
    for o in range(2 * len(ug.unitigs)):  # no link leaves a component
        assert all(c["component_of"][t >> 1] == c["component_of"][o >> 1] for t in to[off[o]:off[o + 1]])
    if k == 31:
        assert c["unitigs"] == [len(ug.unitigs)] and len(ug.unitigs) > 1000  # one G-seq is one component


def test_fifty_rings_are_fifty_circular_components():
    seqs = [RC.ring_record(c, 21) for c in RC.plasmids(50, seed=9)]
    c = R.components_of_sequences(seqs, 21)
    assert c["component_of"] == list(range(50)) and R.circular(c) == [True] * 50 and c["links"] == [2] * 50


def test_empty_graph():
    c = R.components_of_sequences([], K)
    assert c["component_of"] == [] and all(c[f] == [] for f in R.FIELDS)
    assert R.components_tsv(c, K).count("\n") == 1


def test_tsv_of_mixed():
    c = R.components_of_sequences(R.HAND["mixed"], K, [25, 12, 12, 3, 5, 8])
    # bases = kmers + 4 unitigs; mean: 49 / 12 = 4.08 -> 4.1; 3 / 1 = 3.0; 13 / 10 = 1.3
    assert R.components_tsv(c, K) == ("component\tfirst_unitig\tunitigs\tkmers\tbases\tabundance\tmean\tlinks\tdead_ends\tcircular\n"
                                      "0\t0\t3\t12\t24\t49\t4.1\t4\t3\t0\n1\t3\t1\t1\t5\t3\t3.0\t0\t2\t0\n2\t4\t2\t10\t18\t13\t1.3\t4\t1\t0\n")
    ring = R.components_of_sequences(R.HAND["closed"], K)
    assert R.components_tsv(ring, K).splitlines()[1] == "0\t0\t1\t5\t9\t5\t1.0\t2\t0\t1"


# ---- the CLI's flag rules: all of these end in argparse, before the library is asked for anything ----

def _cli(*a):
    return subprocess.run([sys.executable, "-m", "matchtigs_amd", *a], capture_output=True, text=True, cwd=str(ROOT), timeout=120)


def test_help_names_the_flags(capsys):
    from matchtigs_amd.__main__ import main

    with pytest.raises(SystemExit) as e:
        main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert "--components-out" in out and "--unitig-components-out" in out and "--min-component-kmers" in out


@pytest.mark.parametrize("n", ["0", "-3"])
def test_the_threshold_must_be_positive(tmp_path, n):
    r = _cli("--fa-in", str(tmp_path / "missing.fa"), "-k", "5", "--components-out", str(tmp_path / "c.tsv"), "--min-component-kmers", n)
    assert r.returncode == 2 and "--min-component-kmers must be >= 1" in r.stderr


def test_the_filter_is_refused_with_bcalm_in(tmp_path):
    r = _cli("--bcalm-in", str(tmp_path / "missing.fa"), "-k", "5", "--components-out", str(tmp_path / "c.tsv"), "--min-component-kmers", "3")
    assert r.returncode == 2 and "--min-component-kmers needs --seq-in or --fa-in" in r.stderr


@pytest.mark.parametrize("flag", ["--color-matrix-out", "--unitig-colors-out", "--query-colors-out", "--monochromatic-unitigs",
                                  "--color-classes-out", "--unitig-color-classes-out"])
def test_the_filter_is_refused_with_a_colour_flag(tmp_path, flag):
    extra = [flag] if flag == "--monochromatic-unitigs" else [flag, str(tmp_path / "x")]
    if flag == "--query-colors-out":
        extra += ["--query-fa", str(tmp_path / "q.fa"), "--query-out", str(tmp_path / "q.tsv")]
    r = _cli("--seq-in", str(tmp_path / "missing.fa"), "-k", "5", "--unitigs-fa-out", str(tmp_path / "u.fa"), "--min-component-kmers", "3", *extra)
    assert r.returncode == 2 and f"--min-component-kmers cannot be combined with {flag}" in r.stderr, r.stderr[-2000:]


@pytest.mark.parametrize("flag", ["--components-out", "--unitig-components-out"])
def test_nothing_to_do_counts_the_new_outputs(product_lib, tmp_path, flag):
    """Each output flag alone gets the run past the "nothing to do" check, to the input file that does not exist; the filter alone
    is no output."""
    def cli(*a):
        return _cli("--bcalm-in", str(tmp_path / "missing.fa"), "-k", "5", *a)

    r = cli()
    assert r.returncode == 2 and "nothing to do" in r.stderr
    r = _cli("--fa-in", str(tmp_path / "missing.fa"), "-k", "5", "--min-component-kmers", "3")
    assert r.returncode == 2 and "nothing to do" in r.stderr
    r = cli(flag, str(tmp_path / "out"))
    assert r.returncode != 0 and "nothing to do" not in r.stderr and "missing.fa" in r.stderr, r.stderr[-2000:]


def test_headers_compile_as_c_with_the_new_declarations(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "mtg_engine.h"\n'
                   "uint64_t (*a)(const mtg_graph *, const uint64_t *, const uint64_t *, int, uint32_t **, mtg_component_arrays *)"
                   " = mtg_unitig_components;\n"
                   "void (*b)(double *) = mtg_last_unitig_components_times;\n"
                   "void (*c)(const mtg_unitigs *, const uint8_t *, mtg_unitigs **) = mtg_unitigs_select;\n"
                   "void (*d)(int) = mtg_set_unitig_components_aggregation;\n"
                   "int main(void){mtg_component_arrays s; s.first_unitig = 0; s.unitigs = 0; s.kmers = 0; s.abundance = 0; s.links = 0;"
                   " s.dead_ends = 0; s.irregular = 0; return a && b && c && d && sizeof s == 7 * sizeof(void *) && !s.kmers ? 0 : 1;}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-c", str(src), "-o", str(tmp_path / "t.o")], check=True)


def test_the_new_symbols_are_declared():
    import ctypes as C

    from matchtigs_amd import _lib, api

    names = _lib.declared_symbols()
    for n in ("mtg_unitig_components", "mtg_last_unitig_components_times", "mtg_unitigs_select", "mtg_set_unitig_components_aggregation"):
        assert n in names
    assert C.sizeof(_lib.MtgComponentArrays) == 7 * C.sizeof(C.c_void_p)
    assert [f for f, _ in _lib.MtgComponentArrays._fields_] == list(R.FIELDS)
    for n in ("Components", "unitig_components", "select_components", "last_unitig_components_times"):
        assert hasattr(api, n), n


def test_describe_and_circular():
    from matchtigs_amd import api

    c = R.components_of_sequences(R.HAND["mixed"] + ["TTGCATTGC"], K)  # a ring of its own: first 4 = last 4 = TTGC, mirror GCAA
    comps = api.Components(component_of=np.array(c["component_of"], np.uint32), **{
        f: np.array(c[f], np.uint64 if f in ("kmers", "abundance", "links") else np.uint32) for f in R.FIELDS})
    assert comps.circular.tolist() == [False, False, False, True] and len(comps) == 4
    # 12 + 1 + 10 + 5 = 28 k-mers; the largest has 12: 42.9 %
    assert comps.describe() == "4 components, largest 3 unitigs / 12 k-mers (42.9 % of the k-mers), 2 of one unitig, 1 circular"
    with pytest.raises(Exception):
        comps.kmers = None  # frozen
