"""The FASTQ contract's restatement (fastq_ref.py) against hand-written cases with the expected values written out,
its Q = 0 result against the existing host FASTA reader on the twin file, the host half of the reader (fastq_text.hpp) as a
stand-alone program under -fsanitize=address,undefined, and the new entry points. No GPU."""
import ctypes as C
import gzip
import subprocess
from pathlib import Path

import numpy as np
import pytest

import fastq_ref as F
from matchtigs_amd import _lib

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = ("mtg_read_fastq_split", "mtg_read_fastq_named", "mtg_sequence_file_format", "mtg_last_fastq_times")

# name -> (text, Q, pieces, pieces_cut, (records, bases, non_acgt, masked), names); pieces of the split mode, written out by hand
HAND = {
    "quality_line_starting_with_at": (b"@r1\nACGT\n+\n@III\n@r2\nGG\n+\nII\n", 0, [b"ACGT", b"GG"], 0, (2, 6, 0, 0), ["r1", "r2"]),
    "quality_line_starting_with_plus": (b"@r1\nACGT\n+\n+III\n@r2\nGG\n+\n+I\n", 0, [b"ACGT", b"GG"], 0, (2, 6, 0, 0), ["r1", "r2"]),
    "separator_with_name": (b"@r1 first read\nACGT\n+r1 first read\nIIII\n", 0, [b"ACGT"], 0, (1, 4, 0, 0), ["r1"]),
    "crlf": (b"@r1\r\nACGT\r\n+\r\nIIII\r\n@r2\tx\r\nTT\r\n+\r\nII\r\n", 0, [b"ACGT", b"TT"], 0, (2, 6, 0, 0), ["r1", "r2"]),
    "no_final_newline": (b"@r1\nACGT\n+\nIIII", 0, [b"ACGT"], 0, (1, 4, 0, 0), ["r1"]),
    "trailing_blank_lines": (b"@r1\nACGT\n+\nIIII\n\n\r\n\n", 0, [b"ACGT"], 0, (1, 4, 0, 0), ["r1"]),
    "trailing_blank_lines_after_a_read_of_length_0": (b"@r1\nAC\n+\nII\n@e\n\n+\n\n\r\n\n", 0, [b"AC"], 0, (2, 2, 0, 0), ["r1", "e"]),
    "read_of_length_0": (b"@e\n\n+\n\n@r\nAC\n+\nII\n@e2\n\n+\n\n", 0, [b"AC"], 0, (3, 2, 0, 0), ["e", "r", "e2"]),
    "read_of_length_0_without_final_newline": (b"@r\nAC\n+\nII\n@e\n\n+\n", 0, [b"AC"], 0, (2, 2, 0, 0), ["r", "e"]),
    "lower_case": (b"@r\nacgTn\n+\nIIIII\n", 0, [b"ACGT"], 1, (1, 5, 1, 0), ["r"]),
    "n_at_both_ends_and_inside": (b"@r\nNACNNGTN\n+\nIIIIIIII\n", 0, [b"AC", b"GT"], 3, (1, 8, 4, 0), ["r"]),
    # qualities 5 ('&'), 20 ('5'), 21 ('6'), 40 ('I')
    "q_exactly_at_a_base": (b"@r\nACGT\n+\n&56I\n", 20, [b"CGT"], 1, (1, 4, 0, 1), ["r"]),
    "q_one_above_a_base": (b"@r\nACGT\n+\n&56I\n", 21, [b"GT"], 1, (1, 4, 0, 2), ["r"]),
    "every_base_masked": (b"@r\nACGT\n+\n&56I\n@s\nAC\n+\n!!\n", 41, [], 2, (2, 6, 0, 6), ["r", "s"]),
    "mask_inside_and_n": (b"@r\nACNTACG\n+\nII!I!II\n", 10, [b"AC", b"T", b"CG"], 2, (1, 7, 1, 1), ["r"]),
    "empty_file": (b"", 0, [], 0, (0, 0, 0, 0), []),
    "only_blank_lines": (b"\n\r\n\n", 0, [], 0, (0, 0, 0, 0), []),
}

# name -> (text, record, line, reason)
MALFORMED = {
    "three_lines": (b"@r\nACGT\n+\n", 0, 4, F.BAD_LENGTH),  # (the end of the text is read as an empty quality line)
    "three_lines_and_blank_lines": (b"@r\nACGT\n+\n\n\n", 0, 4, F.BAD_LENGTH),
    "two_lines_and_blank_lines": (b"@r\nACGT\n\n\n", 0, 2, F.TRUNCATED),
    "five_lines": (b"@r\nAC\n+\nII\n@s\n", 1, 5, F.TRUNCATED),
    "header_without_at": (b"@r\nAC\n+\nII\nr2\nAC\n+\nII\n", 1, 5, F.BAD_HEADER),
    "fasta": (b">r\nACGT\n>s\nAC\n", 0, 1, F.BAD_HEADER),
    "separator_without_plus": (b"@r\nAC\n-\nII\n", 0, 3, F.BAD_SEPARATOR),
    "quality_shorter": (b"@r\nACGT\n+\nIII\n", 0, 4, F.BAD_LENGTH),
    "quality_longer": (b"@r\nAC\n+\nII\n@s\nAC\n+\nIII\n", 1, 8, F.BAD_LENGTH),
    "multi_line_record": (b"@r\nACGT\nACGT\n+\nIIII\nIIII\n", 0, 3, F.BAD_SEPARATOR),
    "quality_below_bang": (b"@r\nACGT\n+\nII I\n", 0, 4, F.BAD_QUALITY),
    "quality_above_tilde": (b"@r\nAC\n+\nII\n@s\nACGT\n+\nII\x7fI\n", 1, 8, F.BAD_QUALITY),
    "blank_line_inside": (b"@r\nAC\n+\nII\n\n@s\nAC\n+\nII\n", 1, 5, F.BAD_HEADER),
    "earlier_record_wins": (b"@r\nAC\n+\nI\n@s\nAC\n-\nII\n", 0, 4, F.BAD_LENGTH),
    "first_rule_wins_in_a_record": (b"r\nAC\n-\nI\n", 0, 1, F.BAD_HEADER),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_cases(name):
    text, q, pieces, cut, (records, bases, other, masked), names = HAND[name]
    assert F.first_error(text) is None
    data, off, st = F.split(text, q)
    assert [data[off[i]:off[i + 1]] for i in range(len(off) - 1)] == pieces and off[0] == 0
    assert st == dict(records=records, bases=bases, non_acgt_bases=other, masked_bases=masked, pieces=len(pieces),
                      bases_kept=sum(map(len, pieces)), pieces_cut=cut)
    seqs, got_names, nst = F.named(text, q)
    assert got_names == names and len(seqs) == records
    assert nst["pieces"] == records and nst["bases_kept"] == bases


def test_named_mode_masks_with_n_and_keeps_characters():
    seqs, names, _ = F.named(b"@r x\nacNTk\n+\nI!I!I\n", 10)
    assert seqs == [b"aNNNk"] and names == ["r"]
    assert F.named(b"@r x\nacNTk\n+\nI!I!I\n", 0)[0] == [b"acNTk"]


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_malformed_cases(name):
    text, record, line, reason = MALFORMED[name]
    assert F.first_error(text) == (record, line, reason)
    assert F.error_message("x.fq", record, line, reason) == f"x.fq: record {record} (line {line}): {F.REASON_TEXT[reason]}"


def _random_reads(rng, n):
    reads = []
    for i in range(n):
        length = int(rng.choice([0, 1, 6, 7, 8, 151]))
        bases = rng.choice(np.frombuffer(b"ACGTacgtNnRY", np.uint8), length, p=[.2, .2, .2, .2, .03, .03, .03, .03, .03, .02, .02, .01])
        reads.append((f"r{i}".encode(), bases.tobytes(), rng.integers(33, 127, length, dtype=np.uint8).tobytes()))
    return reads


def test_q0_equals_the_host_fasta_reader_on_the_twin(product_lib, tmp_path):
    """api.read_sequences(twin.fa, split_non_acgt=True) is host code: store and pieces_cut, byte for byte."""
    from matchtigs_amd import api

    rng = np.random.default_rng(11)
    texts = [t for t, q, *_ in HAND.values() if q == 0] + [F.fastq_text(_random_reads(rng, 60)) for _ in range(5)]
    for i, text in enumerate(texts):
        twin = tmp_path / f"twin{i}.fa"
        twin.write_bytes(F.fasta_twin(text))
        store = api.read_sequences(str(twin), split_non_acgt=True)
        data, off, st = F.split(text, 0)
        d, o = store.arrays()
        assert d.tobytes() == data and o.tolist() == off and store.pieces_cut == st["pieces_cut"]


def test_entry_points_declared_and_exported(product_lib):
    names = _lib.declared_symbols()
    for n in ENTRY_POINTS:
        assert n in names and hasattr(product_lib, n), n
    assert C.sizeof(_lib.MtgFastqStats) == 8 * 8
    assert [f for f, _ in _lib.MtgFastqStats._fields_] == ["records", "bases", "non_acgt_bases", "masked_bases", "pieces", "bases_kept",
                                                           "pieces_cut", "tile_bytes"]


def test_format_detection(product_lib, tmp_path):
    from matchtigs_amd import api

    for i, (text, want) in enumerate(((b"@r\nAC\n+\nII\n", 2), (b">r\nAC\n", 1), (b"", 0), (b"\n\r\n", 0), (b"\n\n@r\n", 2), (b"\r\n>r\n", 1),
                                      (b"ACGT\n", -1), (b"\n" * 5000 + b"@r\n", 2))):
        p = tmp_path / f"f{i}.fa"  # (the name plays no part)
        p.write_bytes(text)
        assert api.sequence_file_format(str(p)) == want
        with gzip.open(str(p) + ".gz", "wb") as f:
            f.write(text)
        assert api.sequence_file_format(str(p) + ".gz") == want


def test_cli_flags(capsys):
    from matchtigs_amd.__main__ import main

    with pytest.raises(SystemExit):
        main(["--help"])
    out = capsys.readouterr().out
    assert all(f in out for f in ("--min-base-quality", "--query-min-base-quality"))
    for bad in ("-1", "94"):
        with pytest.raises(SystemExit) as e:
            main(["--seq-in", "x.fq", "-k", "5", "--unitigs-fa-out", "u.fa", "--min-base-quality", bad])
        assert e.value.code == 2


def test_host_half_under_sanitizers(tmp_path):
    """fastq_text.hpp (file buffer, trims, detection, name slicing, error message) in a stand-alone program built with
    -fsanitize=address,undefined: what it prints equals the restatement, and no sanitizer report ends the run."""
    exe = tmp_path / "fastq_text_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(ROOT / "tests" / "tools" / "fastq_text_check.cpp"), "-o", str(exe), "-lz", "-pthread"], check=True)
    cases = [t for t, *_ in HAND.values()] + [t for t, *_ in MALFORMED.values()] + [b"@", b"@r", b"\r\n", b"\n", b"@a b\r", b"@r\nAC\r\r\n"]
    cases.append(F.fastq_text(_random_reads(np.random.default_rng(5), 3000)))  # (inflated: larger than the reader's first buffer)
    files = []  # (path, text)
    for i, text in enumerate(cases):
        p = tmp_path / f"c{i}.fq"
        p.write_bytes(text)
        files.append((p, text))
        if i % 2 == 0 or len(text) > 100000:
            with gzip.open(str(p) + ".gz", "wb") as f:
                f.write(text)
            files.append((Path(str(p) + ".gz"), text))
    r = subprocess.run([str(exe), *(str(p) for p, _ in files)], capture_output=True, text=True, encoding="latin-1")
    assert r.returncode == 0, r.stderr[-3000:]
    out = r.stdout.splitlines()
    at = 0
    for p, text in files:
        lines = F.lines_of(text, restore=False)
        first = text.lstrip(b"\r\n")[:1]
        fmt = 0 if not first else 1 if first == b">" else 2 if first == b"@" else -1
        raw = (text if text.endswith(b"\n") or not text else text + b"\n").split(b"\n")[:-1]
        kept = sum(len(l) + 1 for l in raw[:len(lines)])  # the bytes up to the end of the last line that is not empty
        more = kept + 1 if kept else 0  # ... and an empty line behind it
        assert out[at].split() == ["file", str(fmt), str(fmt), str(kept), str(more), str(len(lines)), str(len(lines) // 4)], (p, out[at])
        at += 1
        for rec in range(len(lines) // 4):
            head = lines[4 * rec]
            end = 1
            while end < len(head) and head[end] not in F.WHITE:
                end += 1
            assert out[at] == "name " + head[1:end].decode("latin-1"), (p, rec)
            at += 1
        assert out[at] == "error 23 " + F.error_message(p, 0, 4, F.BAD_QUALITY), out[at]
        at += 1
    assert at == len(out)
