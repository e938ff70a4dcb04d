"""Reference reader and writer of the index file format, version 1, in numpy -- written from the document, sharing
nothing with the library. A file is

    header (784 bytes) | u64 meta_len | meta bytes | zeros to a multiple of 4096 | the 13 sections, each starting at a multiple
    of 4096, zeros between them and up to the file's length, itself a multiple of 4096

all integers little-endian. The header, as 64-bit words unless said otherwise:

    0    char[8] magic "MTGTIGIX"
    8    u32 version (1), u32 byte-order mark (0x01020304)
    16   header length (784)        24  file length         32  meta length         40  meta digest
    48   k, m, records, characters, occurrences, anchors, buckets, bucket_limit, heavy_buckets, heavy_windows, table_slots
    136  shift, locating, n_colors
    160  weights: layout, width, windows, runs, device_bytes        200  colors: the same five
    240  win_offset_bytes           248 sections (13)
    256  13 x (id, element size, count, offset, digest)
    776  the digest of the 776 bytes before

The digest of a byte string: its little-endian 64-bit words w_0 .. w_(n-1), the tail zero-padded;
n XOR sum_i mix(w_i XOR (i + 1) * 0x9E3779B97F4A7C15) mod 2^64, mix = splitmix64's finaliser.
"""
from __future__ import annotations

import json
import struct

import numpy as np

MAGIC = b"MTGTIGIX"
VERSION = 1
BYTE_ORDER_MARK = 0x01020304
HEADER_BYTES = 784
ALIGN = 4096
INFO_FIELDS = ("k", "m", "records", "characters", "occurrences", "anchors", "buckets", "bucket_limit", "heavy_buckets", "heavy_windows",
               "table_slots")
PAYLOAD_FIELDS = ("layout", "width", "windows", "runs", "device_bytes")
SECTIONS = ("packed", "off", "dir", "entries", "table", "heavy_where", "win_off", "weights.dense", "weights.start", "weights.value",
            "colors.dense", "colors.start", "colors.value")
M64 = (1 << 64) - 1


def mix(x: int) -> int:
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9 & M64
    x = (x ^ (x >> 27)) * 0x94D049BB133111EB & M64
    return x ^ (x >> 31)


def digest(data: bytes) -> int:
    """The digest of a byte string (vectorised; digest_slow is the definition word by word)."""
    data = bytes(data)
    n = (len(data) + 7) // 8
    if n == 0:
        return 0
    w = np.frombuffer(data + b"\0" * (8 * n - len(data)), dtype="<u8").copy()
    with np.errstate(over="ignore"):
        x = w ^ (np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
        total = int(np.add.reduce(x, dtype=np.uint64))
    return n ^ total


def digest_slow(data: bytes) -> int:
    n = (len(data) + 7) // 8
    padded = bytes(data) + b"\0" * (8 * n - len(data))
    total = 0
    for i in range(n):
        w = int.from_bytes(padded[8 * i:8 * i + 8], "little")
        total = (total + mix(w ^ ((i + 1) * 0x9E3779B97F4A7C15 & M64))) & M64
    return n ^ total


def _align(x: int) -> int:
    return (x + ALIGN - 1) // ALIGN * ALIGN


def _payload(p) -> dict:
    return {f: int((p or {}).get(f, 0)) for f in PAYLOAD_FIELDS}


def meta_bytes(meta) -> bytes:
    if isinstance(meta, (bytes, bytearray)):
        return bytes(meta)
    return json.dumps(meta if meta is not None else {}, ensure_ascii=False, sort_keys=True, separators=(",", ":")).encode("utf-8")


def pack_header(fields: dict, section_table: list, file_len: int, meta: bytes) -> bytes:
    """The 784 header bytes. fields: the INFO_FIELDS, shift, locating, n_colors, weights, colors (dicts of PAYLOAD_FIELDS or None),
    win_offset_bytes; also version, byte_order, header_len, n_sections, meta_len, meta_digest to write something else than the truth.
    section_table: 13 x (id, elem_size, count, offset, digest)."""
    words = [fields.get("header_len", HEADER_BYTES), file_len, fields.get("meta_len", len(meta)), fields.get("meta_digest", digest(meta))]
    words += [int(fields[f]) for f in INFO_FIELDS]
    words += [int(fields["shift"]), int(fields["locating"]), int(fields["n_colors"])]
    for key in ("weights", "colors"):
        words += [_payload(fields.get(key))[f] for f in PAYLOAD_FIELDS]
    words += [int(fields["win_offset_bytes"]), fields.get("n_sections", len(SECTIONS))]
    for row in section_table:
        words += [int(x) for x in row]
    head = fields.get("magic", MAGIC) + struct.pack("<II", fields.get("version", VERSION), fields.get("byte_order", BYTE_ORDER_MARK))
    head += struct.pack(f"<{len(words)}Q", *[w & M64 for w in words])
    assert len(head) == HEADER_BYTES - 8, len(head)
    return head + struct.pack("<Q", digest(head))


def write(path, fields: dict, arrays: dict, meta=None, counts: dict | None = None, offsets: dict | None = None, file_len: int | None = None) -> bytes:
    """Writes a file from the header fields and the sections' arrays (name -> numpy array or bytes; a missing one is empty) and
    returns its bytes. Element sizes follow the format: packed 4, weights.dense / colors.dense the payload's width, weights.value 4,
    everything else 8. counts / offsets / file_len: what the section table and the header SAY, where a test wants them to lie."""
    blob = meta_bytes(meta)
    elem = {name: 8 for name in SECTIONS}
    elem["packed"] = 4
    elem["weights.value"] = 4
    for key in ("weights", "colors"):
        p = _payload(fields.get(key))
        elem[key + ".dense"] = p["width"] if p["layout"] == 1 else 1
    raw = {}
    for name in SECTIONS:
        a = arrays.get(name, b"")
        raw[name] = bytes(a) if isinstance(a, (bytes, bytearray)) else np.ascontiguousarray(a).tobytes()
    at = _align(HEADER_BYTES + 8 + len(blob))
    table, body = [], {}
    for i, name in enumerate(SECTIONS):
        n = len(raw[name])
        assert n % elem[name] == 0, name
        body[name] = at
        table.append([i + 1, elem[name], (counts or {}).get(name, n // elem[name]), (offsets or {}).get(name, at), digest(raw[name])])
        at = _align(at + n)
    total = at
    head = pack_header(fields, table, total if file_len is None else file_len, blob)
    out = bytearray(total)
    out[:HEADER_BYTES] = head
    out[HEADER_BYTES:HEADER_BYTES + 8] = struct.pack("<Q", fields.get("meta_len", len(blob)))
    out[HEADER_BYTES + 8:HEADER_BYTES + 8 + len(blob)] = blob
    for name in SECTIONS:
        out[body[name]:body[name] + len(raw[name])] = raw[name]
    if path is not None:
        with open(path, "wb") as f:
            f.write(out)
    return bytes(out)


_DTYPES = {1: "u1", 2: "<u2", 4: "<u4", 8: "<u8"}


def read(path_or_bytes, check: bool = True) -> dict:
    """Parses a file: {"fields": the header's fields (as pack_header takes them), "meta": dict, "meta_bytes", "sections": name ->
    {"elem_size", "count", "offset", "digest", "data": numpy array, "bytes"}, "file_len", "header_digest"}. check: every digest,
    the magic, the version and the zero padding are asserted."""
    data = path_or_bytes if isinstance(path_or_bytes, (bytes, bytearray)) else open(path_or_bytes, "rb").read()
    data = bytes(data)
    assert len(data) >= HEADER_BYTES
    version, bom = struct.unpack_from("<II", data, 8)
    words = struct.unpack_from(f"<{(HEADER_BYTES - 16) // 8}Q", data, 16)
    it = iter(words)
    fields = {"magic": data[:8], "version": version, "byte_order": bom, "header_len": next(it)}
    file_len = next(it)
    fields["meta_len"], fields["meta_digest"] = next(it), next(it)
    for f in INFO_FIELDS:
        fields[f] = next(it)
    for f in ("shift", "locating", "n_colors"):
        fields[f] = next(it)
    for key in ("weights", "colors"):
        fields[key] = {f: next(it) for f in PAYLOAD_FIELDS}
    fields["win_offset_bytes"], fields["n_sections"] = next(it), next(it)
    rows = [[next(it) for _ in range(5)] for _ in SECTIONS]
    header_digest = next(it)
    blob = data[HEADER_BYTES + 8:HEADER_BYTES + 8 + fields["meta_len"]]
    sections, covered = {}, [(0, HEADER_BYTES + 8 + fields["meta_len"])]
    for name, (sid, elem, count, offset, dg) in zip(SECTIONS, rows):
        raw = data[offset:offset + elem * count]
        sections[name] = {"id": sid, "elem_size": elem, "count": count, "offset": offset, "digest": dg, "bytes": raw,
                          "data": np.frombuffer(raw, dtype=_DTYPES[elem]).copy()}
        covered.append((offset, offset + elem * count))
    if check:
        assert fields["magic"] == MAGIC and version == VERSION and bom == BYTE_ORDER_MARK and fields["header_len"] == HEADER_BYTES
        assert header_digest == digest(data[:HEADER_BYTES - 8]), "header digest"
        assert file_len == len(data) and file_len % ALIGN == 0, "file length"
        assert struct.unpack_from("<Q", data, HEADER_BYTES)[0] == fields["meta_len"] and digest(blob) == fields["meta_digest"], "metadata"
        for i, name in enumerate(SECTIONS):
            s = sections[name]
            assert s["id"] == i + 1 and s["offset"] % ALIGN == 0 and len(s["bytes"]) == s["elem_size"] * s["count"], name
            assert digest(s["bytes"]) == s["digest"], f"digest of {name}"
        mask = np.ones(len(data), bool)  # what no part covers is zero
        for lo, hi in covered:
            mask[lo:hi] = False
        assert not np.frombuffer(data, np.uint8)[mask].any(), "padding"
    return {"fields": fields, "meta": json.loads(blob.decode("utf-8")) if blob else {}, "meta_bytes": blob, "sections": sections,
            "file_len": file_len, "header_digest": header_digest}


def arrays_of(parsed: dict) -> dict:
    return {name: s["data"] for name, s in parsed["sections"].items()}


def plain_fields(k: int, m: int, records: int, characters: int, occurrences: int, anchors: int, buckets: int = 8, bucket_limit: int = 64,
                 locating: int = 0) -> dict:
    """The header fields of an index without heavy buckets and payloads."""
    return {"k": k, "m": m, "records": records, "characters": characters, "occurrences": occurrences, "anchors": anchors, "buckets": buckets,
            "bucket_limit": bucket_limit, "heavy_buckets": 0, "heavy_windows": 0, "table_slots": 0, "shift": 64 - (buckets.bit_length() - 1),
            "locating": locating, "n_colors": 0, "weights": None, "colors": None, "win_offset_bytes": 0}
