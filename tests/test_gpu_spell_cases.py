"""The spelling kernels (spell_device.hip) on the engineered cases of spell_cases.py, byte for byte against the restatement
spell_ref.py -- not against the host speller, the project's own second reading of the same lines. What each case reaches in the
kernels is said in spell_cases.py; test_spell_cases.py checks on the CPU that the cases do reach it (the censuses) and that the host
speller gives the same bytes.

  - every case in FASTA, GFA and GFA with a header of the caller's, every call made twice;
  - lower-case and mixed-case unitigs give the same upper-case text (the 2-bit store);
  - tigs that a finish on the GPU left in HBM are spelled in place (mark_starts32_kernel), to a FASTA and a GFA file, and only
    afterwards brought to the host for the restatement.

Not here, on purpose: walks on which the reference panics. The device entry point runs check_walks_spellable -- the function the host
speller's child-process tests exercise -- before its first GPU call; an abort on a GPU machine is not something this suite causes.
Out of scope: texts beyond 4 GB (the high plane of the 64-bit extent scan), more than 2^32 - 2 walks, characters outside ACGT (the
device path aborts by contract). No speed is asserted; the kernel's time is printed."""

import numpy as np
import pytest

import spell_cases as SC
import spell_ref
from matchtigs_amd import api

pytestmark = pytest.mark.gpu



@pytest.fixture(scope="module")
def gpu(product_lib):
    if product_lib.mtg_device_count() < 1:
        pytest.fail("these tests need a GPU: the device speller has no CPU fallback")
    return product_lib


def _first_difference(got, want):
    n = min(len(got), len(want))
    a, b = np.frombuffer(got, np.uint8, n), np.frombuffer(want, np.uint8, n)
    d = np.flatnonzero(a != b)
    at = int(d[0]) if len(d) else n
    return f"{len(got)} bytes for {len(want)}, first difference at byte {at}: got {got[max(at - 30, 0):at + 30]!r}, expected {want[max(at - 30, 0):at + 30]!r}"


def _units(case, seqs=None):
    seqs = case.seqs if seqs is None else seqs
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer("".join(seqs).encode(), np.uint8), off


@pytest.mark.parametrize("name", SC.NAMES)
def test_device_speller_equals_the_restatement(gpu, name):
    c = SC.case(name)
    G = SC.graph_of(c)
    units = _units(c)
    for fmt, kw in SC.FORMATS.items():
        want = SC.expected(name, fmt)
        for call in (1, 2):
            got = api.write_walks_text_device(G, c.walks, units, c.k, **kw)
            assert got == want, (name, fmt, call, _first_difference(got, want))
        info = api.last_spell_kernel()
        print(f"{name} {fmt}: {len(want)} bytes, kernel {info['ms']:.3f} ms")


def test_device_speller_gives_upper_case_text_for_lower_and_mixed_case_unitigs(gpu):
    c = SC.case("overlaps-9")
    G = SC.graph_of(c)
    for seqs in SC.mixed_case(c.seqs):
        assert seqs != c.seqs and set("".join(seqs)) <= set("ACGTacgt")
        for fmt, kw in SC.FORMATS.items():
            want = SC.expected("overlaps-9", fmt)
            for call in (1, 2):
                got = api.write_walks_text_device(G, c.walks, seqs, c.k, **kw)  # (unitigs as a list of str, the other input form)
                assert got == want, (fmt, call, _first_difference(got, want))


@pytest.mark.parametrize("euler", ["device", "reference-order"])
def test_resident_tigs_are_spelled_in_place(gpu, tmp_path, euler):
    """Search, claim replay and greedy finish on the GPU; the tigs stay in HBM, and mtg_write_tigs_text_file_device spells them from
    there (mark_starts32_kernel + the kernels of the cases above, on walks the engine made: dummy edges inside tigs, both
    orientations) into a FASTA and two GFA files. Only then do the tigs come to the host, and the files must hold the restatement's
    text of them -- with the dummy weights of the graph as the finish left it."""
    from matchtigs_amd import synth, torch_glue

    k = 21
    L = gpu
    ua = synth.g_seq_arrays(20_000, seed=12, k=k, haplotypes=4, sub_rate=0.02)
    inp = tmp_path / "unitigs.fa"
    inp.write_bytes(ua.bcalm2_text())
    G, store = api.read_bcalm2(str(inp), k)
    n_orig = G.edge_count()
    assert n_orig == 2 * len(store) == 2 * ua.n_unitigs
    dev = api.DeviceGraph(G, k)
    S = dev.classify()
    bufs = torch_glue.run_sssp(dev, 0, S)
    assert dev.replay_claims_resident(bufs.start.data_ptr(), bufs.count.data_ptr(), bufs.pool.data_ptr()) > 0
    mode = api.EulerMode.Device if euler == "device" else api.EulerMode.HostReferenceOrder
    tigs = api.finish_greedytigs_resident(G, dev, k, mode, 0, api.FinishStage.Device)
    files = {}
    for fmt, kw in SC.FORMATS.items():
        header = kw.get("header")
        for call in (1, 2):
            path = tmp_path / f"tigs-{fmt}-{call}"
            n = L.mtg_write_tigs_text_file_device(G.handle, tigs._wp, k, store.handle, 1 if kw["gfa"] else 0,
                                                  header.encode() if header else None, str(path).encode(), 0, 0)
            files[fmt, call] = path.read_bytes()
            assert n == len(files[fmt, call]) > 0
    lim, ed = tigs.arrays()  # only now
    assert len(lim) == tigs.count() and int(lim[-1]) == len(ed)
    walks = spell_ref.walks_of(lim, ed)
    ex = G.export()
    dummy_weights = ex["edge_weight"][n_orig::2].tolist()
    assert ex["edge_weight"][n_orig::2].tolist() == ex["edge_weight"][n_orig + 1::2].tolist()
    inside = sum(e >= n_orig for w in walks for e in w)
    assert inside > 0, "no dummy edge inside a tig: the case shows nothing"
    assert any(e & 1 for w in walks for e in w if e < n_orig) and any(not e & 1 for w in walks for e in w if e < n_orig)
    seqs = store.sequences()
    assert sorted(e >> 1 for w in walks for e in w if e < n_orig) == list(range(len(seqs)))  # every unitig once
    for fmt, kw in SC.FORMATS.items():
        want = spell_ref.spell_ref(k, seqs, n_orig, dummy_weights, walks, **kw)
        for call in (1, 2):
            assert files[fmt, call] == want, (euler, fmt, call, _first_difference(files[fmt, call], want))
    print(f"{euler}: {len(walks)} tigs, {inside} dummy edges inside tigs, {len(files['fasta', 1])} bytes of FASTA")
