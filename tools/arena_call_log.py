"""arena_call_log.py -- does a change of ownership leave the device arena's calls as they were?

Run it with a library whose DeviceArena::alloc and DeviceArena::free (hip_util.hpp) print one line per call to stderr,

    std::fprintf(stderr, "ARENA alloc %zu\\n", want);     // in alloc, once the range is found
    std::fprintf(stderr, "ARENA free %zu\\n", bytes);     // in free, once the range is looked up

(a scratch patch: never committed), once per tree:

    MATCHTIGS_LIBRARY=<that build> python tools/arena_call_log.py 2> calls.log

It makes one staged step (create without reserved work, classify, search over a quarter of the sources and over all, resident replay
twice, free) and one one-shot call at k = 31 and k = 300; per k in {5, 34} an index of each kind with one probe of each kind; the
plain-FASTA join, the speller, the k-mer set comparison and a compaction. Then

    python tools/arena_call_log.py --compare a.log b.log

says whether two logs are equal once every maximal run of consecutive frees is sorted: frees that follow each other with no allocation
in between reach the same arena state in any order, and each of them synchronises first. profiles/device_arrays_arena_calls_*.log."""
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def mark(s):
    sys.stderr.write(f"ARENA # {s}\n")
    sys.stderr.flush()


def normalised(path):
    out, run = [], []
    for line in open(path):
        f = line.split()
        if len(f) != 3 or f[0] != "ARENA" or f[1] == "#":
            continue
        if f[1] == "free":
            run.append(int(f[2]))
        else:
            out += [("free", x) for x in sorted(run)] + [("alloc", int(f[2]))]
            run = []
    return out + [("free", x) for x in sorted(run)]


def compare(path_a, path_b):
    a, b = normalised(path_a), normalised(path_b)
    print(len(a), len(b), "EQUAL" if a == b else "DIFFERENT")
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            print("first difference at call", i, a[max(0, i - 6):i + 6], b[max(0, i - 6):i + 6])
            break
    return 0 if a == b else 1


def calls():
    from matchtigs_amd import api, synth, torch_glue

    api.set_reserve_ahead(False)
    for k, mw in ((31, 8.0), (300, 50.0)):
        bg = synth.g_csr(20000, seed=5, k=k, mean_weight=mw)
        mark(f"staged step k={k}")
        G = api.Bigraph.from_edges(bg.mirror, bg.edge_from, bg.edge_to, bg.edge_weight)
        dev = api.DeviceGraph(G, k, reserve_work=False)
        S = dev.classify(torch_glue.current_stream_ptr())
        bufs = torch_glue.run_sssp(dev, 0, S // 4)
        bufs = torch_glue.run_sssp(dev, 0, S)
        n = dev.replay_claims_resident(bufs.start.data_ptr(), bufs.count.data_ptr(), bufs.pool.data_ptr(), torch_glue.current_stream_ptr())
        n2 = dev.replay_claims_resident(bufs.start.data_ptr(), bufs.count.data_ptr(), bufs.pool.data_ptr(), torch_glue.current_stream_ptr())
        assert n == n2
        on, mu, li = dev.classify_download()
        mark("free")
        del dev
        G.release_device_cache()
        del G
        mark(f"one-shot k={k}")
        G = api.Bigraph.from_edges(bg.mirror, bg.edge_from, bg.edge_to, bg.edge_weight)
        lim, ed = api.GreedytigAlgorithm.compute_tigs_np(G, api.GreedytigAlgorithmConfiguration.new(1, k))
        print("tigs", k, len(lim), int(ed.sum()))
        del lim, ed
        G.release_device_cache()
        del G

    rng = random.Random(3)
    dna = lambda n: "".join(rng.choices("ACGT", k=n))
    for k in (5, 34):
        index = [dna(rng.randint(200, 4000)) for _ in range(40)] + [dna(k - 1)]
        query = [index[0][10:700] + "N" + index[2][5:160], dna(1000), dna(k - 1), index[4][::-1]]
        windows = sum(max(0, len(s) - k + 1) for s in index)
        weights = [rng.getrandbits(32) for _ in range(windows)]
        masks = [rng.getrandbits(3) for _ in range(windows)]
        for kind, kw in (("plain", {}), ("locating", dict(locate=True)), ("weighted", dict(weights=weights)), ("coloured", dict(colors=masks, n_colors=3)),
                         ("all", dict(locate=True, weights=weights, colors=masks, n_colors=3))):
            mark(f"index {kind} k={k}")
            with api.KmerIndex(index, k, **kw) as ix:
                mark("query")
                r = ix.query(query, bits=True); ix.query(query)
                print(kind, k, r.found.tolist())
                if kind in ("locating", "all"):
                    mark("locate"); print(len(ix.locate(query).runs)); ix.locate(["N" * 80])
                if kind in ("weighted", "all"):
                    mark("abundance"); ix.abundance(query, per_window=True); ix.abundance(query)
                if kind in ("coloured", "all"):
                    mark("colours"); ix.color_hits(query, per_window=True); ix.color_hits(query)
                mark("free")
    mark("fasta-in / verify / spell")
    ug = synth.g_seq(3000, seed=2, k=21)
    unitigs = list(ug.unitigs)
    G = api.Bigraph.from_sequences(unitigs, 21)
    tigs = api.GreedytigAlgorithm.compute_tigs(G, api.GreedytigAlgorithmConfiguration.new(1, 21))
    mark("spell")
    text = api.write_walks_text_device(G, tigs, unitigs, 21)
    print(len(text))
    mark("verify")
    print(api.compare_kmer_sets(unitigs, unitigs, 21).equal)
    print(api.compare_kmer_sets(unitigs, unitigs[:-3], 21).equal)
    mark("compact")
    store, c = api.compact_unitigs(unitigs, 21)
    print(c.unitigs)
    G.release_device_cache()
    mark("end")


if __name__ == "__main__":
    sys.exit(compare(*sys.argv[2:4]) if sys.argv[1:2] == ["--compare"] else calls())
