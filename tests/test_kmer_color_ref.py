"""The restatement of the coloured k-mer set's contract (kmer_color_ref.py) on cases derived by hand."""
import pytest

import kmer_color_ref as R
from matchtigs_amd import synth


def test_both_strands_count():
    """AACCG in colour 0, its reverse complement CGGTT in colour 2: one k-mer, mask 0b101."""
    masks = R.kmer_masks(["AACCG", "T", "CGGTT"], [0, 1, 2], 5)
    assert masks == {"AACCG": 0b101}
    assert R.kmer_masks(["aaccg", "CGGTT"], [1, 1], 5) == {"AACCG": 0b10}  # either case; a repeat in one colour adds nothing


def test_a_palindrome_at_even_k():
    """ACGT is its own reverse complement: one class whichever strand is read, and a colour is counted once."""
    assert synth.revcomp("ACGT") == "ACGT"
    assert R.kmer_masks(["ACGT", "ACGT"], [3, 0], 4) == {"ACGT": 0b1001}
    _, _, _, ab, col = R.compact_colored(["ACGT", "ACGT"], [3, 0], 4, 4)
    assert ab["distinct_kept"] == 1 and col["kmer_colors"] == [0b1001] and col["per_color"] == [1, 0, 0, 1]
    assert col["occupancy"][2] == 1 and sum(col["occupancy"]) == 1


def test_a_repeat_inside_one_record_adds_nothing_to_the_mask_but_counts_as_abundance():
    rec = "ACCGTACCGT"  # ACCGT twice; k = 5
    masks = R.kmer_masks([rec], [1], 5)
    assert masks[synth.canonical("ACCGT")] == 0b10
    unitigs, _, _, ab, col = R.compact_colored([rec, "ACCGT"], [1, 0], 2, 5, m=3)
    assert unitigs == ["ACCGT"] and ab["distinct_kept"] == 1  # abundance 3 over all windows, not per colour
    assert col["kmer_colors"] == [0b11] and col["per_color"] == [1, 1] and col["shared"] == [[1, 1], [1, 1]]


def test_a_three_record_toy_by_hand():
    """k = 3. Record a = AAAC (colour 0): AAA, AAC. Record b = AACG (colour 1): AAC, ACG. Record c = GTT (colour 2): GTT = rc(AAC).
    Canonical: AAA {0}, AAC {0, 1, 2}, ACG {1} (rc CGT > ACG)."""
    recs, cols = ["AAAC", "AACG", "GTT"], [0, 1, 2]
    assert R.kmer_masks(recs, cols, 3) == {"AAA": 0b001, "AAC": 0b111, "ACG": 0b010}
    unitigs, stats, _, ab, col = R.compact_colored(recs, cols, 4, 3)  # colour 3 is unused
    assert ab["distinct_kept"] == 3 and sorted(col["kmer_colors"]) == [0b001, 0b010, 0b111]
    assert col["per_color"] == [2, 2, 1, 0]
    assert col["shared"] == [[2, 1, 1, 0], [1, 2, 1, 0], [1, 1, 1, 0], [0, 0, 0, 0]]
    assert col["occupancy"][:5] == [0, 2, 0, 1, 0] and sum(col["occupancy"]) == 3
    # the masks follow the unitigs' windows
    at = 0
    for u in unitigs:
        for i in range(len(u) - 2):
            assert col["kmer_colors"][at] == R.kmer_masks(recs, cols, 3)[synth.canonical(u[i:i + 3])]
            at += 1
    # m = 2 keeps AAC alone (abundance 3 over all colours)
    unitigs, _, _, ab, col = R.compact_colored(recs, cols, 3, 3, m=2)
    assert unitigs in (["AAC"], ["GTT"]) and col["kmer_colors"] == [0b111] and col["occupancy"][3] == 1 and col["per_color"] == [1, 1, 1]
    assert R.jaccard(col["per_color"], col["shared"])[0][2] == 1.0
    assert R.jaccard([0, 1], [[0, 0], [0, 1]]) == [[None, 0.0], [0.0, 1.0]]


def test_colour_rules():
    with pytest.raises(ValueError):
        R.compact_colored(["ACGTA"], [1], 1, 3)  # a colour >= n_colors
    for n in (0, 65):
        with pytest.raises(ValueError):
            R.compact_colored(["ACGTA"], [0], n, 3)
    with pytest.raises(ValueError):
        R.compact_colored(["ACGTA", "ACGTA"], [0], 1, 3)
    # a colour whose records are all shorter than k gives a zero row
    _, _, _, _, col = R.compact_colored(["ACGTAC", "AC", "A"], [0, 1, 1], 2, 3)
    assert col["per_color"][1] == 0 and col["shared"][1] == [0, 0] and col["per_color"][0] > 0
    assert col["occupancy"][2] == 0 and col["occupancy"][1] == col["per_color"][0]
    # 64 colours: bit 63 is a bit like any other
    _, _, _, _, col = R.compact_colored(["ACGTAC", "ACGTAC"], [0, 63], 64, 6)
    assert col["kmer_colors"] == [(1 << 63) | 1] and col["shared"][0][63] == col["shared"][63][0] == 1


def test_the_index_takes_the_mask_of_the_first_occurrence():
    """k = 3, index AACAAC + GTT: AAC at windows 0 and 3 and, as its reverse complement, in record 1; the first mask given wins."""
    index, colors = ["AACAAC", "GT", "GTT"], [0b01, 0b10, 0b10, 0b11, 0b100]  # windows: AAC ACA CAA AAC | - | GTT
    assert R.class_colors(index, colors, 3) == {"AAC": 0b01, "ACA": 0b10, "CAA": 0b10}
    with pytest.raises(ValueError):
        R.class_colors(index, colors[:-1], 3)
    got = R.color_hits(index, colors, 3, ["GTTG", "ACAN", "", "TTG"], 3)
    assert got["kmers"] == [2, 2, 0, 1] and got["valid"] == [2, 1, 0, 1] and got["found"] == [2, 1, 0, 1]
    assert got["per_color"] == [[1, 1, 0], [0, 1, 0], [0, 0, 0], [0, 1, 0]]  # GTT -> AAC {0}, TTG -> CAA {1}; ACA {1}; TTG {1}
    assert got["per_window"] == [0b01, 0b10, 0, 0] + [0b10, 0, 0, 0] + [0b10, 0, 0]
    with pytest.raises(ValueError):
        R.color_hits(index, colors, 2, [], 3)  # 0b100 is colour 2


def test_a_zero_mask_is_found_and_touches_no_column():
    got = R.color_hits(["ACGGA"], [0, 0b1, 0], 2, ["ACGGAT"], 3)  # ACG {}, CGG = rc(CCG) {0}, GGA {}; GAT absent
    assert got["found"] == [3] and got["valid"] == [4] and got["per_color"] == [[1, 0]] and got["per_window"] == [0, 1, 0, 0, 0, 0]


def test_the_files_lines():
    col = {"n_colors": 2, "per_color": [3, 2], "shared": [[3, 1], [1, 2]], "occupancy": [0, 3, 1] + [0] * 62}
    assert R.matrix_lines(["a.fa", "b.fq"], col) == ["color\tkmers\ta.fa\tb.fq", "a.fa\t3\t3\t1", "b.fq\t2\t1\t2", "#occupancy\t3\t1"]
    assert R.unitig_color_lines(["ACGTA", "ACG"], [1, 1, 3, 1 << 63], 3) == ["2:1 1:3", "1:8000000000000000"]
