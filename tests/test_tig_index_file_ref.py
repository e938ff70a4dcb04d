"""The index file format on the host: the numpy reader and writer (tig_index_file_ref) against the library's header
reader (api.tig_index_file_info, a host translation unit: no GPU), the digest against values worked out by hand, every header
refusal with a message that names its check, and the committed golden file of format version 1 under both readers."""
from pathlib import Path

import numpy as np
import pytest

import tig_index_file_ref as ref
from matchtigs_amd import api

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "tig_index_v1.mtgx"
M64 = (1 << 64) - 1
STEP = 0x9E3779B97F4A7C15


def _mix(x):
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & M64
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & M64
    return x ^ (x >> 31)


def test_digest_by_hand():
    # the empty array: no word, n = 0
    assert ref.digest(b"") == ref.digest_slow(b"") == 0
    # one zero word: 1 XOR mix(0 XOR 1 * STEP); mix(STEP) is the first output of splitmix64 seeded with 0, 0xE220A8397B1DCDAF
    assert _mix(STEP) == 0xE220A8397B1DCDAF
    assert ref.digest(b"\0" * 8) == 1 ^ 0xE220A8397B1DCDAF == 0xE220A8397B1DCDAE
    # a 5-byte tail alone: the word 0x0000000504030201, zero-padded
    assert ref.digest(bytes([1, 2, 3, 4, 5])) == 1 ^ _mix(0x0504030201 ^ STEP) == 0x89508AA2D09C7748
    # two words and a 5-byte tail: n = 3, the terms add mod 2^64
    data = bytes(range(21))
    words = [int.from_bytes(data[0:8], "little"), int.from_bytes(data[8:16], "little"), 0x1413121110]
    assert words[0] == 0x0706050403020100
    total = sum(_mix(w ^ ((i + 1) * STEP & M64)) for i, w in enumerate(words)) & M64
    assert ref.digest(data) == ref.digest_slow(data) == 3 ^ total == 0x6C7568028F9F6BDF
    assert ref.digest(bytes(range(16))) == 0x2C66BFBF605DCF39
    # a change confined to one word changes the digest; so does a zero byte more (n grows from 2 to 3)
    assert ref.digest(bytes(range(16))) != ref.digest(bytes(range(15)) + b"\x10")
    assert ref.digest(bytes(range(16)) + b"\0") != ref.digest(bytes(range(16)))
    rng = np.random.default_rng(1)
    for n in (7, 8, 9, 4096, 4099):
        blob = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert ref.digest(blob) == ref.digest_slow(blob)


def _hand_made():
    """The fields and arrays of a small, consistent index: k = 5, m = 3, two records of 12 and 8 bases, weights as runs, masks dense."""
    fields = ref.plain_fields(k=5, m=3, records=2, characters=20, occurrences=12, anchors=3, locating=1)
    fields.update(n_colors=9, win_offset_bytes=24,
                  weights={"layout": 2, "width": 1, "windows": 12, "runs": 2, "device_bytes": 24},
                  colors={"layout": 1, "width": 2, "windows": 12, "runs": 5, "device_bytes": 24})
    arrays = {"packed": np.arange(4, dtype=np.uint32), "off": np.array([0, 12, 20], np.uint64), "dir": np.array([0, 1, 1, 2, 2, 2, 3, 3, 3], np.uint64),
              "entries": np.array([1, 9, 14], np.uint64), "win_off": np.array([0, 8, 12], np.uint64),
              "weights.start": np.array([0, 7], np.uint64), "weights.value": np.array([3, 300], np.uint32),
              "colors.dense": np.arange(12, dtype=np.uint16)}
    return fields, arrays


def test_reference_writer_against_the_library_reader(tmp_path):
    fields, arrays = _hand_made()
    meta = {"indexed": "input", "colors": ["a.fa", "größe/β.fq", "样本.fa"], "min_abundance": 2, "cleaning": {"clip_tips": 5}}
    path = tmp_path / "hand.mtgx"
    data = ref.write(path, fields, arrays, meta)
    assert len(data) % 4096 == 0 and ref.read(path)["meta"] == meta
    head = api.tig_index_file_info(path)
    for f in ref.INFO_FIELDS:
        assert getattr(head["info"], f) == fields[f], f
    # device_bytes as the builder counts them: packed, off, dir, entries, win_off, the payloads
    assert head["info"].device_bytes == 4 * 4 + 3 * 8 + 9 * 8 + 3 * 8 + 24 + 24 + 24
    assert (head["locating"], head["weighted"], head["colored"], head["n_colors"], head["win_offset_bytes"]) == (True, True, True, 9, 24)
    assert head["payload_info"] == {"weights": dict(fields["weights"], layout="runs"), "colors": dict(fields["colors"], layout="dense")}
    assert head["meta"] == meta and head["file_bytes"] == len(data)
    ref.write(path, fields, arrays, None)  # no metadata given: an empty object
    assert api.tig_index_file_info(path)["meta"] == {}
    # the reader gives back what the writer took
    parsed = ref.read(data)
    for name, a in arrays.items():
        assert np.array_equal(parsed["sections"][name]["data"], a), name
    assert ref.write(None, parsed["fields"], ref.arrays_of(parsed), parsed["meta_bytes"]) == data


def _refusal(path, *needles):
    with pytest.raises(api.IndexFileError) as e:
        api.tig_index_file_info(path)
    assert str(path) in str(e.value) and all(n in str(e.value) for n in needles), str(e.value)
    assert isinstance(e.value, ValueError)


def test_header_refusals_name_their_check(tmp_path):
    fields, arrays = _hand_made()
    path = tmp_path / "bad.mtgx"
    good = ref.write(path, fields, arrays, {"x": 1})
    api.tig_index_file_info(path)

    ref.write(path, dict(fields, magic=b"MTGKMERX"), arrays)
    _refusal(path, "magic")
    ref.write(path, dict(fields, version=2), arrays)
    _refusal(path, "version", "version 2")
    swapped = bytearray(good)  # the two 32-bit fields as a host of the other byte order writes them
    swapped[8:12], swapped[12:16] = good[8:12][::-1], good[12:16][::-1]
    path.write_bytes(swapped)
    _refusal(path, "byte order")
    for at in (40, 300, 783):  # a flipped header bit: in a field, in the section table, in the digest itself
        flipped = bytearray(good)
        flipped[at] ^= 0x04
        path.write_bytes(flipped)
        _refusal(path, "header digest")
    for cut in (0, 100, 783):
        path.write_bytes(good[:cut])
        _refusal(path, "shorter than the header")
    path.write_bytes(good[:-4096])
    _refusal(path, "extent")
    ref.write(path, fields, arrays, counts={"colors.dense": 12 + 4096})  # a section reaching past the end of the file
    _refusal(path, "section colors.dense:", "extent", "past the end")
    ref.write(path, fields, arrays, offsets={"entries": 1 << 50})
    _refusal(path, "section entries:", "extent")
    ref.write(path, fields, arrays, counts={"off": 2})  # a count that contradicts the info fields (records + 1 = 3)
    _refusal(path, "section off:", "count", "imply 3")
    ref.write(path, dict(fields, records=1 << 60), arrays)  # 2^60 elements: refused on the host
    _refusal(path, "count")
    ref.write(path, dict(fields, anchors=2), arrays)
    _refusal(path, "section entries:", "count")
    ref.write(path, dict(fields, m=6), arrays)  # m > k
    _refusal(path, "limits", "minimizer length 6")
    ref.write(path, dict(fields, m=0), arrays)
    _refusal(path, "limits", "minimizer length 0")
    ref.write(path, dict(fields, n_colors=65), arrays)
    _refusal(path, "limits", "n_colors is 65")
    ref.write(path, dict(fields, bucket_limit=65537), arrays)
    _refusal(path, "limits", "bucket_limit")
    ref.write(path, dict(fields, k=1 << 32, m=3), arrays)
    _refusal(path, "limits", "k is")
    ref.write(path, dict(fields, colors=dict(fields["colors"], width=4, device_bytes=48)), dict(arrays, **{"colors.dense": np.arange(12, dtype=np.uint32)}))
    _refusal(path, "limits", "width")  # 9 colours take 2 bytes
    ref.write(path, dict(fields, shift=60), arrays)
    _refusal(path, "limits", "shift")
    blob = bytearray(good)
    blob[ref.HEADER_BYTES + 9] ^= 1
    path.write_bytes(blob)
    _refusal(path, "metadata")
    _refusal(tmp_path / "missing.mtgx", "cannot open")


def test_golden_file_of_version_1():
    """The file of the smallest plain case of tests/test_gpu_tig_index_file.py, as a GPU run wrote it: both readers, field for field.
    This pins format version 1."""
    data = GOLDEN.read_bytes()
    assert len(data) <= 64 << 10
    parsed = ref.read(data)  # (every digest, the padding, the magic and the version)
    head = api.tig_index_file_info(GOLDEN)
    f = parsed["fields"]
    assert (f["version"], f["k"], f["m"], f["locating"], f["n_colors"], f["table_slots"]) == (1, 5, 3, 0, 0, 0)
    for name in ref.INFO_FIELDS:
        assert getattr(head["info"], name) == f[name], name
    assert head["meta"] == parsed["meta"] == {"indexed": "golden"} and not head["weighted"] and not head["colored"]
    counts = {name: s["count"] for name, s in parsed["sections"].items()}
    assert counts["packed"] == (f["characters"] + 15) // 16 + 2 and counts["off"] == f["records"] + 1 == 10
    assert counts["dir"] == f["buckets"] + 1 and counts["entries"] == f["anchors"] > 0
    assert all(counts[name] == 0 for name in ref.SECTIONS[4:])
    off = parsed["sections"]["off"]["data"]
    assert off[0] == 0 and off[-1] == f["characters"] and (np.diff(off.astype(np.int64)) >= 0).all()
    # the packed bases spell the records: 2 bits per base, base i in bits 2 (i mod 16) of word i / 16
    import test_gpu_tig_index_file as T

    text = "".join(T._records(5))
    packed = parsed["sections"]["packed"]["data"]
    codes = [(int(packed[i // 16]) >> (2 * (i % 16))) & 3 for i in range(len(text))]
    assert "".join("ACGT"[c] for c in codes) == text
    assert ref.write(None, f, ref.arrays_of(parsed), parsed["meta_bytes"]) == data
