"""The restatement of the unitig graph output (unitig_links_ref.py) held to cases worked out by hand, to the links
synth.g_seq lists by its own rule, and the host-side surface of the feature: the CLI's flags and the C declarations. No GPU."""
import subprocess
from pathlib import Path

import pytest

import unitig_links_ref as R
from matchtigs_amd import synth

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("name", sorted(R.HAND))
def test_hand_cases(name):
    seqs, off, to = R.HAND[name]
    assert R.links_of_sequences(seqs, R.K_HAND) == (off, to)
    if name in R.HAND_BCALM:
        assert R.bcalm_text(seqs, R.K_HAND, off, to) == R.HAND_BCALM[name]
    if name in R.HAND_GFA:
        assert R.gfa_text(seqs, R.K_HAND, off, to) == R.HAND_GFA[name]


def test_what_the_hand_cases_show():
    t = {name: R.link_tuples(off, to) for name, (_, off, to) in R.HAND.items()}
    assert t["fork"][:3] == [(0, True, 1, True), (0, True, 2, True), (0, True, 3, True)]          # three successors
    assert t["merge"] == [(0, True, 2, True), (1, True, 2, True), (2, False, 0, False), (2, False, 1, False)]
    assert t["closed"] == [(0, True, 0, True), (0, False, 0, False)]                              # both self links
    assert t["hairpin"] == [(0, True, 0, False)]                                                  # its own mirror: once
    assert t["isolated"] == []
    for links in t.values():  # a link and its mirror (v, not b) -> (u, not a) are both listed
        assert sorted(links) == sorted((v, not b, u, not a) for u, a, v, b in links)


def test_the_graph_rule_agrees_on_the_hand_cases():
    """fasta_in_ref's graph of the same records (nodes = (k-1)-mers) gives the same lists by from == to."""
    import fasta_in_ref as F

    for seqs, off, to in R.HAND.values():
        g = F.graph_dict(seqs, R.K_HAND)
        assert R.links_of_graph(g["edge_from"], g["edge_to"], 2 * len(seqs)) == (off, to)


def test_km_rule():
    assert R.km_text(5, 4) == "1.3" and f"{5 / 4:.1f}" == "1.2"  # round half up in integers, not "%.1f"
    assert R.km_text(4, 4) == "1.0" and R.km_text(1, 3) == "0.3" and R.km_text(2, 3) == "0.7" and R.km_text(199, 100) == "2.0"
    big = (1 << 32) + 6
    assert R.km_text(big, 4) == "1073741825.5"
    text = R.bcalm_text(["ACCGTTAG"], 5, [0, 0, 0], [], kc=[big])
    assert text == f">0 LN:i:8 KC:i:{big} km:f:1073741825.5\nACCGTTAG\n"
    assert R.gfa_text(["ACCGTTAG"], 5, [0, 0, 0], [], kc=[5]) == "H\tVN:Z:1.0\tKL:Z:5\nS\t0\tACCGTTAG\tLN:i:8\tKC:i:5\tkm:f:1.3\n"


def test_empty_store():
    assert R.links_of_sequences([], 5) == ([0], [])
    assert R.bcalm_text([], 5, [0], []) == "" and R.gfa_text([], 5, [0], []) == "H\tVN:Z:1.0\tKL:Z:5\n"


@pytest.mark.parametrize("k", [5, 12, 21, 31, 32])
def test_links_equal_g_seq(k):
    ug = synth.g_seq(400 if k == 5 else 3000, seed=5, k=k)
    off, to = R.links_of_sequences(ug.unitigs, k)
    links = R.link_tuples(off, to)
    assert len(links) == len(set(links)) and set(links) == set(ug.links) and len(links) > 0
    recs = R.parse_bcalm(R.bcalm_text(ug.unitigs, k, off, to))
    assert [l for r in recs for l in r["links"]] == links and [r["seq"] for r in recs] == ug.unitigs


def test_help_names_both_flags(capsys):
    from matchtigs_amd.__main__ import main

    with pytest.raises(SystemExit) as e:
        main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert "--unitigs-bcalm-out" in out and "--unitigs-gfa-out" in out


@pytest.mark.parametrize("flag", ["--unitigs-bcalm-out", "--unitigs-gfa-out"])
def test_nothing_to_do_counts_both_flags(product_lib, tmp_path, flag):
    """Each flag alone is an output: the run gets past the "nothing to do" check and stops at the input file that does not exist."""
    import sys

    def cli(*a):
        return subprocess.run([sys.executable, "-m", "matchtigs_amd", "--bcalm-in", str(tmp_path / "missing.fa"), "-k", "5", *a],
                              capture_output=True, text=True, cwd=str(ROOT), timeout=120)

    r = cli()
    assert r.returncode == 2 and "nothing to do" in r.stderr
    r = cli(flag, str(tmp_path / "out"))
    assert r.returncode != 0 and "nothing to do" not in r.stderr and "missing.fa" in r.stderr, r.stderr[-2000:]


def test_headers_compile_as_c_with_the_new_declarations(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "mtg_engine.h"\n'
                   "uint64_t (*a)(const mtg_graph *, int, uint64_t **, uint32_t **) = mtg_unitig_links;\n"
                   "uint64_t (*b)(const mtg_graph *, const char *, const uint64_t *, uint64_t, uint64_t, const uint64_t *, int, int, char **)"
                   " = mtg_write_unitig_graph_text;\n"
                   "uint64_t (*c)(const mtg_graph *, const char *, const uint64_t *, uint64_t, uint64_t, const uint64_t *, int, int,"
                   " const char *, int) = mtg_write_unitig_graph_file;\n"
                   "void (*d)(double *) = mtg_last_unitig_graph_times;\n"
                   "int main(void){return a && b && c && d ? 0 : 1;}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-c", str(src), "-o", str(tmp_path / "t.o")], check=True)


def test_the_new_symbols_are_declared():
    from matchtigs_amd import _lib

    names = _lib.declared_symbols()
    for n in ("mtg_unitig_links", "mtg_write_unitig_graph_text", "mtg_write_unitig_graph_file", "mtg_last_unitig_graph_times"):
        assert n in names
