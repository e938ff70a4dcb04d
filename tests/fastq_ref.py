"""The FASTQ reader's contract restated in plain Python over bytes: what `api.read_fastq` must return for a text.

The text is a sequence of lines ended by "\\n"; one "\\r" before the "\\n" belongs to the line end; a missing final "\\n" is tolerated;
empty lines are tolerated only behind the last record, and when three lines remain of the last record, the end of the text is its
quality line, of length 0. Record r is lines 4r .. 4r+3: line 4r begins with `@`, line 4r+2 with `+` (the rest of it is ignored), lines 4r+1 and 4r+3 have the same length (0 included), every quality byte lies in '!' .. '~'. The kind of a
line is its index mod 4 and nothing else. The first error is that of the smallest record which breaks a rule and, inside it, the first
rule in the order header, separator, length, quality; a line count that is no multiple of 4 belongs to the incomplete last record.

Base j of a record is good when it is one of ACGTacgt and qual[j] - 33 >= Q. Split mode: the maximal runs of good bases, upper-cased,
in file order; pieces_cut = the runs of bases that are not good. Named mode: the records whole, a base with qual[j] - 33 < Q as `N`.
"""
from __future__ import annotations

TRUNCATED, BAD_HEADER, BAD_SEPARATOR, BAD_LENGTH, BAD_QUALITY = "truncated", "header", "separator", "length", "quality"
REASON_TEXT = {
    TRUNCATED: "the file ends inside the record (its line count is not a multiple of 4)",
    BAD_HEADER: "the header line does not begin with '@'",
    BAD_SEPARATOR: "the separator line does not begin with '+'",
    BAD_LENGTH: "the sequence and the quality line differ in length",
    BAD_QUALITY: "a quality character is outside '!' .. '~'",
}
ACGT = frozenset(b"ACGTacgt")
WHITE = frozenset(b" \t\n\v\f\r")


def lines_of(text: bytes, restore: bool = True) -> list[bytes]:
    """The lines without their ends; the empty ones behind the last line that is not empty are dropped. restore: when three lines
    remain of the last record, the end of the text is its quality line, of length 0 (written with or without its line end)."""
    if text and not text.endswith(b"\n"):
        text += b"\n"
    out = []
    start = 0
    for i, c in enumerate(text):
        if c == 0x0A:
            end = i - 1 if i > start and text[i - 1] == 0x0D else i
            out.append(text[start:end])
            start = i + 1
    while out and not out[-1]:
        out.pop()
    if restore and len(out) % 4 == 3:
        out.append(b"")
    return out


def first_error(text: bytes):
    """None, or (0-based record, 1-based line, reason) of the first offending record."""
    lines = lines_of(text)
    for r in range((len(lines) + 3) // 4):
        rec = lines[4 * r:4 * r + 4]
        if len(rec) < 4:
            return r, len(lines), TRUNCATED
        if not rec[0].startswith(b"@"):
            return r, 4 * r + 1, BAD_HEADER
        if not rec[2].startswith(b"+"):
            return r, 4 * r + 3, BAD_SEPARATOR
        if len(rec[1]) != len(rec[3]):
            return r, 4 * r + 4, BAD_LENGTH
        if any(q < 33 or q > 126 for q in rec[3]):
            return r, 4 * r + 4, BAD_QUALITY
    return None


def error_message(path, record: int, line: int, reason: str) -> str:
    return f"{path}: record {record} (line {line}): {REASON_TEXT[reason]}"


def records_of(text: bytes):
    """[(name, bases, qualities)] of a well-formed text."""
    assert first_error(text) is None
    lines = lines_of(text)
    out = []
    for r in range(len(lines) // 4):
        head = lines[4 * r]
        end = 1
        while end < len(head) and head[end] not in WHITE:
            end += 1
        out.append((head[1:end].decode("latin-1"), lines[4 * r + 1], lines[4 * r + 3]))
    return out


def good_flags(bases: bytes, quals: bytes, q_min: int) -> list[bool]:
    return [b in ACGT and q - 33 >= q_min for b, q in zip(bases, quals)]


def split(text: bytes, q_min: int = 0):
    """(data, offsets, stats) of the split mode; stats holds the seven counters of mtg_fastq_stats."""
    data = bytearray()
    off = [0]
    st = dict(records=0, bases=0, non_acgt_bases=0, masked_bases=0, pieces=0, bases_kept=0, pieces_cut=0)
    for _, bases, quals in records_of(text):
        st["records"] += 1
        st["bases"] += len(bases)
        prev = None
        for b, g in zip(bases, good_flags(bases, quals, q_min)):
            if b not in ACGT:
                st["non_acgt_bases"] += 1
            elif not g:
                st["masked_bases"] += 1
            if g:
                data.append(b & 0xDF)
            else:
                if prev is None or prev:
                    st["pieces_cut"] += 1
                if len(data) > off[-1]:
                    off.append(len(data))
            prev = g
        if len(data) > off[-1]:
            off.append(len(data))
    st["pieces"] = len(off) - 1
    st["bases_kept"] = len(data)
    return bytes(data), off, st


def named(text: bytes, q_min: int = 0):
    """(sequences, names, stats) of the named mode: pieces = records, bases_kept = bases."""
    recs = records_of(text)
    seqs = [bytes(0x4E if q - 33 < q_min else b for b, q in zip(bases, quals)) for _, bases, quals in recs]
    st = split(text, q_min)[2]
    st["pieces"], st["bases_kept"] = st["records"], st["bases"]
    return seqs, [n for n, _, _ in recs], st


def fasta_twin(text: bytes, q_min: int = 0, names: bool = False) -> bytes:
    """The same reads as one-line FASTA records; with q_min > 0 every base below the threshold is written as `N`."""
    seqs, nm, _ = named(text, q_min)
    return b"".join(b">" + (nm[i].encode("latin-1") if names else str(i).encode()) + b"\n" + s + b"\n" for i, s in enumerate(seqs))


def fastq_text(reads, eol: bytes = b"\n", final_newline: bool = True) -> bytes:
    """reads: [(name, bases, qualities)] -> four-line FASTQ."""
    text = b"".join(b"@" + n + eol + s + eol + b"+" + eol + q + eol for n, s, q in reads)
    return text if final_newline or not text else text[:-len(eol)]
