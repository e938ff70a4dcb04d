"""The engineered spelling cases (spell_cases.py) on the CPU: the host speller (spell.cpp through api.write_walks_fasta / _gfa) equals
the restatement spell_ref.py byte for byte on every case, in FASTA, GFA and GFA with a header of the caller's; pyref.fasta agrees where
the walks hold no dummy edge; the censuses say that the cases reach what they were built for; and the four inputs on which the
reference panics (an empty walk, a dummy first edge, a dummy heavier than k - 1, an overlap longer than the unitig) end the host
speller with a message -- in a child process, through the HOST entry point only: the device entry point runs the same function
(check_walks_spellable) before its first GPU call, and no test hands it such input.

Out of scope here and in test_gpu_spell_cases.py: texts beyond 4 GB, more than 2^32 - 2 walks, characters outside ACGT."""
import subprocess
import sys
from pathlib import Path

import pytest

import pyref
import spell_cases as SC
import spell_ref
from matchtigs_amd import api

ROOT = Path(__file__).resolve().parents[1]


@pytest.mark.parametrize("name", SC.NAMES)
def test_host_speller_equals_the_restatement(name, product_lib):
    c = SC.case(name)
    G = SC.graph_of(c)
    seqs = c.seqs
    fasta = api.write_walks_fasta(G, c.walks, seqs, c.k)
    assert fasta == SC.expected(name, "fasta")
    assert api.write_walks_gfa(G, c.walks, seqs, c.k) == SC.expected(name, "gfa")
    assert api.write_walks_gfa(G, c.walks, seqs, c.k, header=SC.FORMATS["gfa-header"]["header"]) == SC.expected(name, "gfa-header")
    # the three texts differ in what they should: the header line and the record frame
    assert SC.expected(name, "gfa").startswith(f"H\tKL:Z:{c.k}\nS\t1\t".encode()) and SC.expected(name, "gfa-header").startswith(b"H\tVN:Z:1.0\tKL:Z:77\nS\t1\t")
    assert SC.expected(name, "gfa").split(b"\n", 1)[1] == SC.expected(name, "gfa-header").split(b"\n", 1)[1]
    assert fasta.startswith(b">1\n") and fasta.count(b">") == len(c.walk_lists())
    walks = c.walk_lists()
    if all(e < c.n_orig for w in walks for e in w):  # no dummy edge: the graph as built is all the restatement of the algorithms needs
        pg = pyref.from_unitig_links([len(s) - c.k + 1 for s in seqs], [])
        assert pyref.fasta(pg, walks, seqs, c.k).encode() == fasta


def test_which_cases_hold_no_dummy_edge():
    """... so that the comparison with pyref.fasta above is known to happen: k = 1 has no dummy weights, many-walks no dummy edges."""
    none = [n for n in SC.NAMES if all(e < SC.case(n).n_orig for w in SC.case(n).walk_lists() for e in w)]
    assert none == ["overlaps-1", "many-walks"]


@pytest.mark.parametrize("k", SC.OVERLAP_KS)
def test_census_of_overlaps(k):
    c = SC.case(f"overlaps-{k}")
    s = c.census
    assert c.k == k and len(c.seqs) == 40 and len(c.walks) == 300 and max(map(len, c.walks)) == 13 and min(map(len, c.walks)) == 1
    assert sorted(set(c.dummy_weights)) == list(range(1, k))
    assert s["transitions"] == {(p, f) for p in ["o"] + list(range(1, k)) for f in (True, False)}
    assert s["lengths"] == SC.overlap_lengths(k) and min(s["lengths"]) == max(k - 1, 1) and s["start_residues"] == list(range(16))
    assert {n % 16 for n in s["lengths"]} >= {0, 1} and s["backwards_first"] > 0
    if k >= 2:
        assert min(s["dummy_runs"], s["ends_in_dummy"], s["zero_character_edges"], s["offset_zero_after_dummy"]) >= 1
    assert s == SC.census_of(c.k, c.seqs, c.pairs, c.walks)


def test_census_of_the_block_cases():
    assert (SC.SP_BLOCK, SC.SCAN_BLOCK, SC.BLOCK_K) == (256, 1024, 5)
    totals = {n: SC.case(n).census for n in SC.BLOCK_CASES if n.startswith("total-")}
    assert [s["positions"] for s in totals.values()] == list(SC.BLOCK_TOTALS) == [SC.case(n).n_positions() for n in totals]
    assert [n for n, s in totals.items() if s["sentinel_alone_in_workgroup"]] == ["total-256", "total-512", "total-1024"]
    assert [n for n, s in totals.items() if s["sentinel_last_in_workgroup"]] == ["total-255", "total-511", "total-1023"]
    assert [n for n, s in totals.items() if s["sentinel_alone_in_scan_block"]] == ["total-1024"]
    assert [n for n, s in totals.items() if s["sentinel_last_in_scan_block"]] == ["total-1023"]
    assert SC.case("walk-starts").census["walk_starts_on_block_edges"] == [0, 256, 512, 768, 1024, 1280]
    silent = SC.case("silent-block")
    assert silent.census["silent_blocks"] == [1, 2] and (255, 256) in silent.census["zero_extent_block_edges"] and (767, 768) in silent.census["zero_extent_block_edges"]
    run = max(silent.walks, key=len)
    assert sum(e >= silent.n_orig for e in run) == 600 and all(e >= silent.n_orig for e in run[10:610])
    assert SC.case("zero-extents").census["zero_extent_block_edges"] == [(255, 256), (511, 512), (767, 768), (1023, 1024)]


def test_census_of_many_walks():
    c = SC.case("many-walks")
    lim, ed = c.walks
    assert len(lim) == 1_050_000 == c.n_positions() and len(c.seqs) == 64 and c.k == 5 and int(ed.max()) == 127 and int(ed.min()) == 0
    assert c.n_positions() + 1 > SC.SCAN_BLOCK * SC.SCAN_BLOCK and c.census["scan_blocks"] > SC.SCAN_BLOCK
    text = SC.expected("many-walks", "fasta")
    for n in (9, 99, 999, 9999, 99_999, 999_999):  # every digit boundary lies inside the text
        assert f"\n>{n}\n".encode() in text and f"\n>{n + 1}\n".encode() in text
    assert text.index(b"\n>1000000\n") < len(text) - 400_000 and len(text) > 16_000_000


def test_mixed_case_input(product_lib):
    """Lower-case and mixed-case unitigs: the reference's 2-bit store gives upper-case text, and so does the restatement (the GPU
    speller is held to that in test_gpu_spell_cases.py). The host speller copies characters as they are: its text is the expected one
    up to case."""
    c = SC.case("overlaps-9")
    G = SC.graph_of(c)
    lower, mixed = SC.mixed_case(c.seqs)
    assert lower != c.seqs and mixed != c.seqs and mixed != lower and [s.upper() for s in mixed] == c.seqs
    assert set("".join(mixed)) == set("ACGTacgt")
    for seqs in (lower, mixed):
        assert spell_ref.spell_ref(c.k, seqs, c.n_orig, c.dummy_weights, c.walks) == SC.expected("overlaps-9", "fasta")
        host = api.write_walks_fasta(G, c.walks, seqs, c.k)
        assert host != SC.expected("overlaps-9", "fasta") and host.upper() == SC.expected("overlaps-9", "fasta")


# ---- the inputs on which the reference panics ----
# k = 9, unitigs of 9, 8, 7 and 20 bases, dummy biedges of weight 8 (= k - 1: fine) and 9 (too heavy): edges 8, 9 and 10, 11
_CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import spell_cases as SC
from matchtigs_amd import api
c = SC.Case(9, ["ACGTACGTA", "CCCCGGGG", "ACGTTGC", "ACGTACGTAACCGGTTACGT"], [(0, 3, 8), (0, 3, 9)], None)
G = api.Bigraph.from_unitig_links([1, 0, 0, 12], [])
ex = G.export()
rows = np.zeros(2, api.PAIR_DTYPE)
for i, (a, b, w) in enumerate(c.pairs):
    rows[i] = (ex["edge_to"][2 * a], ex["edge_from"][2 * b], w)
G.insert_pair_edges(rows)
assert G.edge_count() == 12
good = api.write_walks_fasta(G, [[0, 8, 6], [0, 2, 3]], c.seqs, 9)
assert good == b">1\\nACGTACGTAACGTACGTAACCGGTTACGT\\n>2\\nACGTACGTA\\n", good
print("GOOD", flush=True)
walks = {walks}
writer = api.write_walks_gfa if {gfa} else api.write_walks_fasta
writer(G, walks, c.seqs, 9)
print("RETURNED", flush=True)
"""
IMPOSSIBLE = {
    "empty-walk": ("(np.array([2, 2, 3], np.uint64), np.array([0, 6, 2], np.uint32))", "libmatchtigs: empty walk 1\n"),
    "dummy-first": ("[[0], [6, 0], [8, 6]]", "libmatchtigs: walk 2 starts with a dummy edge (bin.rs:489)\n"),
    "dummy-heavier-than-k-1": ("[[0, 8, 6], [0, 11, 6]]", "libmatchtigs: dummy edge 11 of weight 9: longer than k - 1 = 8 (bin.rs:536)\n"),
    "overlap-longer-than-unitig": ("[[0, 2], [6, 5]]", "libmatchtigs: overlap 8 longer than unitig 2\n"),
}


@pytest.mark.parametrize("gfa", [False, True])
@pytest.mark.parametrize("name", IMPOSSIBLE)
def test_host_speller_dies_with_a_message_where_the_reference_panics(name, gfa, product_lib):
    walks, message = IMPOSSIBLE[name]
    code = _CHILD.format(root=str(ROOT), tests=str(ROOT / "tests"), walks=walks, gfa=gfa)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(ROOT), timeout=120)
    assert r.stdout == "GOOD\n", r.stdout + r.stderr[-1500:]  # the graph is right, legal walks are spelled, the call did not return
    assert r.returncode == -6, (r.returncode, r.stderr[-1500:])  # SIGABRT
    assert r.stderr.endswith(message), r.stderr[-1500:]


@pytest.mark.parametrize("name", IMPOSSIBLE)
def test_the_restatement_refuses_the_same_inputs(name):
    import numpy as np  # noqa: F401  (the walks of IMPOSSIBLE are written as the child process reads them)

    walks = eval(IMPOSSIBLE[name][0])
    if isinstance(walks, tuple):
        walks = spell_ref.walks_of(*walks)
    seqs = ["ACGTACGTA", "CCCCGGGG", "ACGTTGC", "ACGTACGTAACCGGTTACGT"]
    assert spell_ref.spell_ref(9, seqs, 8, [8, 9], [[0, 8, 6], [0, 2, 3]]) == b">1\nACGTACGTAACGTACGTAACCGGTTACGT\n>2\nACGTACGTA\n"
    with pytest.raises(AssertionError):
        spell_ref.spell_ref(9, seqs, 8, [8, 9], walks)
