"""The sparse minimizer index written to a file and reopened on the GPU (tig_index_file_device.hpp, api.TigIndex.save / .load,
DESIGN.md 35): the round trip of every kind of index -- fields, device bytes, bytes of the file against the numpy reader and writer
(tig_index_file_ref, which shares nothing with the library), identical answers of every probe, a tally and a pseudoaligner on the
built and the loaded index --, determinism of the file, and the refusals: flipped bits, a truncated file, and files crafted with the
reference writer whose digests are right so that only the validation kernel can object. A test never probes an index obtained from
a damaged or crafted file: it asserts that load raises, and fails there if it does not."""
import dataclasses
import random
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import tig_index_cases as cases
import tig_index_file_ref as ref
import tig_index_ref as TR
from matchtigs_amd import api, synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
KM = [(5, 3), (31, None), (32, None), (63, None)]  # 32: the first wide k
VARIANTS = ["plain", "locating", "weights-dense", "weights-runs", "colors1-dense", "colors1-runs", "colors64-dense", "colors64-runs", "both"]


@pytest.fixture(scope="module")
def gpu(product_lib):
    import torch

    if product_lib.mtg_device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("these tests need a GPU: the tig index has no CPU path")
    return torch


def _records(k):
    """Short records: random ones, one shorter than k, a poly-A and a two-base repeat (with bucket_limit = 2 their buckets are heavy),
    and reverse-complement duplicates across records."""
    rng = random.Random(1000 + k)
    a, b = cases.dna(rng, 2 * k + 9), cases.dna(rng, k + 3)
    return [a, "ACGT"[:min(4, k - 1)], "A" * (k + 6), "AC" * (k // 2 + 6), b, synth.revcomp(a)[3:], cases.dna(rng, k), synth.revcomp(b), a[5:5 + k + 2]]


def _queries(k, index):
    rng = random.Random(2000 + k)
    long = "".join(index)
    return [index[0], synth.revcomp(index[4]), cases.dna(rng, 3 * k), index[2][:k + 1] + "N" + index[3][:k + 2], "ACG"[:min(3, k - 1)], "",
            index[3], long[7:7 + 4 * k].lower(), synth.revcomp(index[2]) + "NN" + index[6]]


def _payloads(variant, windows, rng):
    """(weights, colors, n_colors, layout) of a variant."""
    weights = masks = n_colors = layout = None
    if variant.startswith("weights") or variant == "both":
        weights = [1 + (i // 7) % 5 + (300 if i % 11 == 0 else 0) for i in range(windows)]  # runs of 7, two widths
        layout = variant.split("-")[1] if "-" in variant else "runs"
    if variant.startswith("colors") or variant == "both":
        n_colors = 64 if "64" in variant else 1 if variant.startswith("colors1") else 3
        top = (1 << n_colors) - 1
        masks = [(rng.getrandbits(n_colors) | (1 << (n_colors - 1) if i % 5 == 0 else 0)) & top if (i // 4) % 2 else top for i in range(windows)]
        layout = variant.split("-")[1] if "-" in variant else "runs"
    return weights, masks, n_colors, layout


def _build(variant, index, k, m):
    windows = sum(max(0, len(s) - k + 1) for s in index)
    weights, masks, n_colors, layout = _payloads(variant, windows, random.Random(f"{variant}-{k}"))
    if variant == "plain":
        return api.TigIndex(index, k, m, bucket_limit=2)
    if variant == "locating":
        return api.TigIndex(index, k, m, bucket_limit=2, locate=True)
    return api.TigIndex.annotated(index, k, m, bucket_limit=2, weights=weights, colors=masks, n_colors=n_colors, payload_layout=layout)


def _same(a, b, what):
    """Two results of the API are equal, array for array."""
    if dataclasses.is_dataclass(a):
        a, b = dataclasses.asdict(a), dataclasses.asdict(b)
    if isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for key in a:
            _same(a[key], b[key], (what, key))
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (what, a, b)
    else:
        assert a == b, (what, a, b)


def _held():
    api.release_device_memory(0)
    return api.device_memory_held(0)


def _same_answers(built, loaded, queries, mates, what):
    _same(built.query(queries, bits=True), loaded.query(queries, bits=True), (what, "query"))
    if not built.locating:
        with pytest.raises(ValueError):
            loaded.locate(queries)
        return
    _same(built.locate(queries), loaded.locate(queries), (what, "locate"))
    if built.weighted:
        _same(built.abundance(queries, per_window=True), loaded.abundance(queries, per_window=True), (what, "abundance"))
    if built.colored:
        _same(built.color_hits(queries, per_window=True), loaded.color_hits(queries, per_window=True), (what, "color_hits"))
    tallies = []
    for ix in (built, loaded):
        with api.TigTally(ix) as t:
            added = t.add(queries)
            tallies.append((added, t.coverage(queries, per_window=True), t.counters()))
    for x, y in zip(*tallies):
        _same(x, y, (what, "tally"))
    if built.colored:
        aligned = []
        for ix in (built, loaded):
            with api.Pseudoaligner(ix, 500, "valid") as p:
                aligned.append((p.align(queries, mates), p.classes(), p.totals))
        for x, y in zip(*aligned):
            _same(x, y, (what, "pseudoalign"))


@pytest.mark.parametrize("k,m", KM)
@pytest.mark.parametrize("variant", VARIANTS)
def test_round_trip(gpu, tmp_path, k, m, variant):
    index = _records(k)
    queries = _queries(k, index)
    mates = [synth.revcomp(q.upper().replace("N", "A")) for q in queries]
    first, second, again = (str(tmp_path / name) for name in ("first.mtgx", "second.mtgx", "again.mtgx"))
    meta = {"indexed": "input", "colors": ["a.fa", "ü/β.fa"], "min_abundance": 1, "cleaning": {}}
    before = _held()
    built = _build(variant, index, k, m)
    assert built.meta == {}
    n_bytes = built.save(first, meta)
    data = Path(first).read_bytes()
    assert n_bytes == len(data) and built.meta == meta and not Path(first + ".tmp").exists()
    assert built.info.heavy_buckets > 0 and built.info.table_slots > 0 and built.info.anchors > 0, built.info  # every array exists

    # the file by the reference reader: every digest (computed on the GPU) is the reference's of the bytes in the file, the padding
    # is zero, and the reference writer makes the same file from the same arrays
    parsed = ref.read(data)
    assert parsed["meta"] == meta and parsed["fields"]["locating"] == int(built.locating)
    assert ref.write(None, parsed["fields"], ref.arrays_of(parsed), parsed["meta_bytes"]) == data
    assert {f: parsed["fields"][f] for f in ref.INFO_FIELDS} == {f: getattr(built.info, f) for f in ref.INFO_FIELDS}
    head = api.tig_index_file_info(first)
    assert head["info"] == built.info and head["meta"] == meta and head["file_bytes"] == n_bytes
    assert (head["locating"], head["weighted"], head["colored"], head["n_colors"], head["payload_info"]) == (
        built.locating, built.weighted, built.colored, built.n_colors, built.payload_info)

    loaded = api.TigIndex.load(first)
    assert loaded.info == built.info and loaded.info.device_bytes == built.info.device_bytes
    assert (loaded.locating, loaded.weighted, loaded.colored, loaded.n_colors, loaded.payload_info, loaded.meta) == (
        built.locating, built.weighted, built.colored, built.n_colors, built.payload_info, meta)
    times = api.last_tig_index_file_times()
    assert set(times["save"]) == {"digest_ms", "download_ms", "write_ms"} and set(times["load"]) == {"read_ms", "upload_ms", "digest_ms", "validate_ms"}
    assert all(v >= 0 for part in times.values() for v in part.values()) and times["load"]["validate_ms"] > 0

    _same_answers(built, loaded, queries, mates, (k, variant))
    want = TR.query(TR.TigIndexRef(index, k, m, 2), [q.upper() for q in queries], k)  # not merely equally wrong
    got = loaded.query(queries, bits=True)
    for f in ("kmers", "valid", "found", "valid_bits", "present_bits"):
        assert getattr(got, f).tolist() == want[f], (k, variant, f)

    # a file is a function of the index and the metadata alone
    assert loaded.save(again, meta) == n_bytes and Path(again).read_bytes() == data  # the loaded index gives the bytes it came from
    assert built.save(again, meta) == n_bytes and Path(again).read_bytes() == data   # and a second save of one index the same bytes
    with _build(variant, index, k, m) as rebuilt:  # a second build: everything but the heavy table, whose slots are claimed in
        rebuilt.save(second, meta)                  # the order the atomics land in, is the same
    other = ref.read(second)
    assert other["fields"] == parsed["fields"]
    for name in ref.SECTIONS:
        if name not in ("table", "heavy_where"):
            assert other["sections"][name]["bytes"] == parsed["sections"][name]["bytes"], name
    if k < 32:  # (the slots hold the classes' codes: the same words, wherever they landed)
        assert sorted(other["sections"]["table"]["data"].tolist()) == sorted(parsed["sections"]["table"]["data"].tolist())
    built.close()
    loaded.close()
    assert _held() == before


def test_second_build_without_heavy_buckets_gives_the_same_file(gpu, tmp_path):
    rng = random.Random(5)
    index = [cases.dna(rng, 70), cases.dna(rng, 33)]
    files = []
    for name in ("a.mtgx", "b.mtgx"):
        with api.TigIndex(index, 31, locate=True) as ix:
            assert ix.info.heavy_buckets == 0
            ix.save(str(tmp_path / name))
            files.append((tmp_path / name).read_bytes())
    assert files[0] == files[1]
    assert ref.read(files[0])["sections"]["table"]["count"] == 0


def test_empty_index(gpu, tmp_path):
    """No record of length >= k: no window, no anchor; still a file, and the loaded index finds nothing."""
    path = str(tmp_path / "empty.mtgx")
    before = _held()
    for variant in ("plain", "both"):
        with _build(variant, ["ACG", "", "TT"], 5, 3) as built:
            assert built.info.occurrences == 0 and built.info.anchors == 0
            built.save(path)
            ref.read(path)
            with api.TigIndex.load(path) as loaded:
                assert loaded.info == built.info and loaded.payload_info == built.payload_info and loaded.meta == {}
                _same(built.query(["ACGTACGT", "N"], bits=True), loaded.query(["ACGTACGT", "N"], bits=True), variant)
                assert loaded.query(["ACGTACGT"]).found.tolist() == [0]
                with api.TigIndex.load(path) as twice:
                    assert twice.save(str(tmp_path / "again.mtgx")) and (tmp_path / "again.mtgx").read_bytes() == Path(path).read_bytes()
    assert _held() == before


def _refused(path, *needles):
    before = _held()
    with pytest.raises(api.IndexFileError) as e:
        api.TigIndex.load(str(path))  # (were it to succeed, the test fails here and the index is never probed)
    message = str(e.value)
    assert str(path) in message and all(n in message for n in needles), message
    assert _held() == before, message
    return message


@pytest.fixture(scope="module")
def both_file(gpu, tmp_path_factory):
    """(path, bytes) of the files of indexes that between them have every section, by (variant, k)."""
    d = tmp_path_factory.mktemp("index_files")
    out = {}
    for variant in ("both", "colors64-dense", "weights-dense", "colors1-runs"):
        for k, m in ((5, 3), (32, None)):
            path = d / f"{variant}-{k}.mtgx"
            with _build(variant, _records(k), k, m) as ix:
                ix.save(str(path), {"variant": variant})
            out[variant, k] = (path, path.read_bytes())
    return out


def test_a_flipped_bit_in_every_section_is_refused_by_name(both_file, tmp_path):
    seen = set()
    for (variant, k), (path, data) in both_file.items():
        parsed = ref.read(data)
        for name, s in parsed["sections"].items():
            if not s["count"]:
                continue
            damaged = bytearray(data)
            damaged[s["offset"] + len(s["bytes"]) // 2] ^= 0x10
            bad = tmp_path / "flipped.mtgx"
            bad.write_bytes(damaged)
            _refused(bad, f"section {name}:", "digest")
            seen.add(name)
    assert seen == set(ref.SECTIONS)


def test_truncated_and_damaged_headers_are_refused(both_file, tmp_path):
    path, data = both_file["both", 5]
    bad = tmp_path / "bad.mtgx"
    bad.write_bytes(data[:-4096])
    _refused(bad, "extent")
    bad.write_bytes(data[:100])
    _refused(bad, "shorter than the header")
    flipped = bytearray(data)
    flipped[50] ^= 1  # k
    bad.write_bytes(flipped)
    _refused(bad, "header digest")
    flipped = bytearray(data)
    flipped[ref.HEADER_BYTES + 8 + 3] ^= 1  # the metadata
    bad.write_bytes(flipped)
    _refused(bad, "metadata")
    parsed = ref.read(data)
    ref.write(bad, dict(parsed["fields"], version=2), ref.arrays_of(parsed), parsed["meta_bytes"])
    _refused(bad, "version 2")
    ref.write(bad, dict(parsed["fields"], records=1 << 60), ref.arrays_of(parsed), parsed["meta_bytes"])  # never reaches an allocation
    _refused(bad, "count")
    with pytest.raises(api.IndexFileError):
        api.TigIndex.load(str(tmp_path / "missing.mtgx"))


def _crafted(tmp_path, entry, section, change, fields=None):
    """The file of `entry` with one section changed by change(array) and every digest recomputed: only the validator can object."""
    _, data = entry
    parsed = ref.read(data)
    arrays = ref.arrays_of(parsed)
    arrays[section] = change(arrays[section].copy())
    path = tmp_path / "crafted.mtgx"
    ref.write(path, dict(parsed["fields"], **(fields or {})), arrays, parsed["meta_bytes"])
    ref.read(path)  # (sound as a file)
    return path


def test_crafted_files_are_refused_by_the_validator(both_file, tmp_path):
    for k in (5, 32):
        both, runs1, dense64 = both_file["both", k], both_file["colors1-runs", k], both_file["colors64-dense", k]
        characters = ref.read(both[1])["fields"]["characters"]

        def set_at(i, value):
            def change(a):
                a[i] = value
                return a
            return change

        def beyond(a):  # an entries word whose position lies beyond the text (its tag kept)
            a[len(a) // 2] = (int(a[len(a) // 2]) >> 40 << 40) | (characters + 5)
            return a

        def last_room(a):  # ... and one inside the text without room for its m-mer
            a[0] = (int(a[0]) >> 40 << 40) | (characters - 1)
            return a

        def decreasing(a):  # a bucket that starts behind the start of the next (its heavy bit kept)
            i, low = len(a) // 2, (1 << 63) - 1
            a[i] = (int(a[i]) & (1 << 63)) | ((int(a[i + 1]) & low) + 1)
            return a

        _refused(_crafted(tmp_path, both, "entries", beyond), "section entries:", "validation")
        _refused(_crafted(tmp_path, both, "entries", last_room), "section entries:", "validation")
        _refused(_crafted(tmp_path, both, "dir", decreasing), "section dir:", "validation")
        _refused(_crafted(tmp_path, both, "dir", lambda a: set_at(len(a) - 1, int(a[-1]) - 1)(a)), "section dir:", "validation")
        _refused(_crafted(tmp_path, both, "off", lambda a: set_at(len(a) - 1, int(a[-1]) - 1)(a)), "section off:", "validation")
        _refused(_crafted(tmp_path, both, "off", lambda a: set_at(1, int(a[2]) + 1)(a)), "section off:", "validation")
        _refused(_crafted(tmp_path, both, "win_off", lambda a: set_at(1, int(a[1]) + 1)(a)), "section win_off:", "validation")
        for name in ("weights.start", "colors.start"):  # out of order; not starting at 0; beyond the windows
            _refused(_crafted(tmp_path, both, name, lambda a: set_at(2, int(a[1]))(a)), f"section {name}:", "validation")
            _refused(_crafted(tmp_path, both, name, lambda a: set_at(0, 1)(a)), f"section {name}:", "validation")
            _refused(_crafted(tmp_path, both, name, lambda a: set_at(len(a) - 1, 1 << 40)(a)), f"section {name}:", "validation")
        _refused(_crafted(tmp_path, both, "colors.value", lambda a: set_at(1, int(a[1]) | 8)(a)), "section colors.value:", "n_colors")  # 3 colours
        _refused(_crafted(tmp_path, runs1, "colors.value", lambda a: set_at(0, 3)(a)), "section colors.value:", "n_colors")  # 1 colour
        # dense masks of 64 colours cannot break the rule: the same arrays under n_colors = 63 can
        path = _crafted(tmp_path, dense64, "colors.dense", lambda a: set_at(3, int(a[3]) | (1 << 63))(a), {"n_colors": 63})
        _refused(path, "section colors.dense:", "n_colors")
        slot = int(np.flatnonzero(ref.read(both[1])["sections"]["table"]["data"] != np.uint64(ref.M64))[0])
        _refused(_crafted(tmp_path, both, "heavy_where", set_at(slot, characters)), "section heavy_where:", "validation")
        if k >= 32:
            _refused(_crafted(tmp_path, both, "table", set_at(slot, (1 << 40) - 2)), "section table:", "validation")


def _cli_files(tmp_path, k=9):
    rng = random.Random(77)
    common = cases.dna(rng, 60)
    a = [common + cases.dna(rng, 30), cases.dna(rng, 45), "A" * 20]
    b = [synth.revcomp(common) + cases.dna(rng, 25), cases.dna(rng, 50)]
    q = [common[5:40], synth.revcomp(a[1])[:30] + "N" + b[1][:20], cases.dna(rng, 40), "ACG"]
    r = [a[0][:50], b[1], common, cases.dna(rng, 30)]
    for name, recs in (("a.fa", a), ("b.fa", b), ("q.fa", q), ("r.fa", r)):
        (tmp_path / name).write_text("".join(f">{name}{i}\n{s}\n" for i, s in enumerate(recs)))
    return a, b


def _cli(tmp_path, *argv):
    import os

    return subprocess.run([sys.executable, "-m", "matchtigs_amd", *argv], cwd=tmp_path, capture_output=True, text=True,
                          env=dict(os.environ, PYTHONPATH=str(ROOT)))


@pytest.mark.parametrize("over", ["input", "greedytigs"])
def test_command_line_round_trip(gpu, tmp_path, over):
    """A run that builds, saves and queries; then a run on the file alone: every output byte for byte, no compaction, no index build."""
    _cli_files(tmp_path)

    def outputs(d):
        (tmp_path / d).mkdir()
        return ["--query-fa", "q.fa", "--query-index", "minimizer", "--query-out", f"{d}/q.tsv", "--query-presence-out", f"{d}/p.txt",
                "--query-index-locate-out", f"{d}/l.tsv", "--query-index-abundance-out", f"{d}/a.tsv", "--query-index-colors-out", f"{d}/c.tsv",
                "--pseudoalign-fa", "r.fa", "--pseudoalign-index", "minimizer", "--pseudoalign-out", f"{d}/pa.tsv",
                "--pseudoalign-classes-out", f"{d}/pc.tsv"]

    extra = [] if over == "input" else ["--greedytigs-fa-out", "g.fa", "--index-over", "greedytigs", "--query-index-over", "greedytigs"]
    direct = _cli(tmp_path, "--seq-in", "a.fa", "--seq-in", "b.fa", "-k", "9", "--index-out", "x.mtgx", "--index-weights", "--index-colors",
                  *extra, *outputs("direct"))
    assert direct.returncode == 0, direct.stderr
    assert "x.mtgx" in direct.stderr and "minimizer index" in direct.stderr
    head = api.tig_index_file_info(tmp_path / "x.mtgx")
    assert head["meta"]["indexed"] == over and head["meta"]["colors"] == ["a.fa", "b.fa"] and head["weighted"] and head["colored"]
    # (the pseudoalignment of the direct run always indexes the input: the same k-mer set with the same colours, the same files)
    again = _cli(tmp_path, "--index-in", "x.mtgx", *[x for x in outputs("file") if x not in ("--query-index", "--pseudoalign-index", "minimizer")])
    assert again.returncode == 0, again.stderr
    assert not any(word in again.stderr for word in ("compacted", "Indexing", "unitigs")), again.stderr
    for name in ("q.tsv", "p.txt", "l.tsv", "a.tsv", "c.tsv", "pa.tsv", "pc.tsv"):
        assert (tmp_path / "file" / name).read_bytes() == (tmp_path / "direct" / name).read_bytes(), (over, name)
        assert len((tmp_path / "file" / name).read_bytes().splitlines()) >= 2, name  # (a header and a row at the least)


def test_command_line_refusals(gpu, tmp_path, monkeypatch, capsys):
    """A wrong -k names both values, a flag the file cannot serve names the flag and what the file lacks, a damaged file ends the run
    with status 2 and the library's message. In this process: the command line's main() is what is asked."""
    from matchtigs_amd.__main__ import main

    a, b = _cli_files(tmp_path)
    monkeypatch.chdir(tmp_path)
    with api.TigIndex(a + b, 9, locate=True) as ix:
        ix.save("x.mtgx", {"indexed": "input", "colors": []})
    assert main(["--index-in", "x.mtgx", "-k", "11", "--query-fa", "q.fa", "--query-out", "w.tsv"]) == 2
    err = capsys.readouterr().err
    assert "k = 9" in err and "-k 11" in err, err
    with pytest.raises(SystemExit) as e:
        main(["--index-in", "x.mtgx", "--query-fa", "q.fa", "--query-out", "w.tsv", "--query-index-abundance-out", "a.tsv"])
    err = capsys.readouterr().err
    assert e.value.code == 2 and "--query-index-abundance-out" in err and "weights" in err, err
    damaged = bytearray((tmp_path / "x.mtgx").read_bytes())
    damaged[ref.read(bytes(damaged))["sections"]["entries"]["offset"] + 9] ^= 1
    (tmp_path / "damaged.mtgx").write_bytes(damaged)
    held = _held()
    assert main(["--index-in", "damaged.mtgx", "--query-fa", "q.fa", "--query-out", "w.tsv"]) == 2
    assert "damaged.mtgx: section entries: digest" in capsys.readouterr().err
    assert not (tmp_path / "w.tsv").exists() and _held() == held
    assert main(["--index-in", "x.mtgx", "--query-fa", "q.fa", "--query-out", "w.tsv"]) == 0  # and the sound file serves
    assert len((tmp_path / "w.tsv").read_text().splitlines()) == 5


def test_golden_file_loads(gpu):
    """Format version 1 as committed: the file still loads, and answers."""
    path = ROOT / "tests" / "golden" / "tig_index_v1.mtgx"
    with api.TigIndex.load(str(path)) as ix:
        assert ix.info.k == 5 and ix.info.m == 3 and ix.meta == {"indexed": "golden"}
        index, queries = _records(5), _queries(5, _records(5))
        want = TR.query(TR.TigIndexRef(index, 5, 3), [q.upper() for q in queries], 5)
        got = ix.query(queries, bits=True)
        for f in ("kmers", "valid", "found", "valid_bits", "present_bits"):
            assert getattr(got, f).tolist() == want[f], f
