"""Engineered inputs for the tig spellers (spell.cpp on the host, spell_device.hip on the GPU), with spell_ref.py as the expectation.

A speller reads walks, edge payloads and sequences, nothing of the graph's shape, so no de Bruijn graph is needed: U isolated unitigs
(api.Bigraph.from_unitig_links(weights, []): edge 2 u is unitig u forwards, 2 u + 1 the same unitig backwards), dummy biedges of
chosen weights appended with Bigraph.insert_pair_edges (dummy biedge i = edges n_orig + 2 i, n_orig + 2 i + 1, weight exactly as
given), and walks written by hand. Every builder is seeded, returns a Case and raises if its census -- the list of places it was
built to reach -- falls short. What the cases aim at in spell_device.hip:

  overlaps(k)          the overlap in front of an original edge (position_extent): k - 1 after an original edge, k - 1 - w after a
                       dummy of every weight w, for either orientation of the edge; dummy runs, trailing dummies, edges that add no
                       character; unitigs that start at every residue mod 16 of the 2-bit store and end on both sides of a word
  edges_of_blocks(..)  the workgroups of SP_BLOCK positions and the scan blocks of SCAN_BLOCK: the sentinel position P first, last or
                       alone in its block; walks that start on a block edge; a block that writes nothing; zero-extent positions on
                       block edges
  many_walks()         walk numbers of 1 to 7 digits and more than SCAN_BLOCK scan blocks (scan64_sums_kernel's second round)

Out of scope (not reachable in a test of seconds, or aborting by contract): texts beyond 4 GB (the high plane of the 64-bit extent
scan), more than 2^32 - 2 walks, characters outside ACGT on the device path."""
from dataclasses import dataclass, field

import numpy as np

SP_BLOCK = 256     # positions per workgroup of spell_kernel (spell_device.hip)
SCAN_BLOCK = 1024  # values per block of the scan64_* kernels; scan64_sums_kernel takes SCAN_BLOCK block sums per round

OVERLAP_KS = (1, 2, 3, 9, 31, 32, 33)
BLOCK_TOTALS = (255, 256, 257, 511, 512, 1023, 1024, 1025)
BLOCK_CASES = tuple(f"total-{p}" for p in BLOCK_TOTALS) + ("walk-starts", "silent-block", "zero-extents")
SEED = 7  # (chosen: with it every census below holds; test_spell_cases.py builds all of them)


@dataclass
class Case:
    k: int
    seqs: list            # unitig sequences (str)
    pairs: list           # dummy biedges (unitig a, unitig b, weight): from the end of a forwards to the start of b forwards
    walks: object         # list of lists of edge ids, or (limits uint64, edges uint32) numpy arrays
    census: dict = field(default_factory=dict)
    _lists: object = None

    @property
    def n_orig(self):
        return 2 * len(self.seqs)

    @property
    def dummy_weights(self):
        return [w for _, _, w in self.pairs]

    def walk_lists(self):
        """The walks as lists of Python ints (made once)."""
        if isinstance(self.walks, tuple) and self._lists is None:
            ed, b, self._lists = self.walks[1].tolist(), 0, []
            for e in self.walks[0].tolist():
                self._lists.append(ed[b:e])
                b = e
        return self._lists if isinstance(self.walks, tuple) else self.walks

    def n_positions(self):
        return int(self.walks[0][-1]) if isinstance(self.walks, tuple) else sum(len(w) for w in self.walks)


def graph_of(case):
    """The library's bigraph of a case: isolated unitigs + the dummy biedges. The dummy weights are checked against export()."""
    from matchtigs_amd import api

    weights = [len(s) - case.k + 1 for s in case.seqs]  # k-mers per unitig; 0 for a unitig of k - 1 bases
    G = api.Bigraph.from_unitig_links(weights, [])
    n_orig = G.edge_count()
    assert n_orig == case.n_orig
    if case.pairs:
        ex = G.export()
        rows = np.zeros(len(case.pairs), api.PAIR_DTYPE)
        for i, (a, b, w) in enumerate(case.pairs):
            rows[i] = (ex["edge_to"][2 * a], ex["edge_from"][2 * b], w)
        assert G.insert_pair_edges(rows) == len(case.pairs)
        ex = G.export()
        assert G.edge_count() == n_orig + 2 * len(case.pairs) and ex["edge_dummy_id"][:n_orig].max() == 0 and ex["edge_dummy_id"][n_orig:].min() > 0
        assert ex["edge_weight"][n_orig:].tolist() == [w for w in case.dummy_weights for _ in (0, 1)]
    return G


def dna(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


def mixed_case(seqs, seed=SEED):
    """-> (lower-case copies, copies with every character's case drawn at random)."""
    rng = np.random.default_rng(seed)
    return [s.lower() for s in seqs], ["".join(c.lower() if f else c for c, f in zip(s, rng.random(len(s)) < 0.5)) for s in seqs]


def census_of(k, seqs, pairs, walks):
    """What a set of walks contains, in the terms of position_extent: transitions = {(previous, forwards)} over the original edges
    that follow another edge, previous = "o" for an original edge or the weight of the dummy; the counts of dummy runs of two or
    more, walks that end in a dummy, original edges that add no character, original edges written with offset 0 behind a dummy of
    weight k - 1; the lengths of the unitigs and the residues mod 16 of their starts in the concatenated store."""
    n_orig = 2 * len(seqs)
    c = {"transitions": set(), "dummy_runs": 0, "ends_in_dummy": 0, "zero_character_edges": 0, "offset_zero_after_dummy": 0,
         "backwards_first": 0}
    for walk in walks:
        assert walk and walk[0] < n_orig
        c["backwards_first"] += walk[0] & 1
        c["ends_in_dummy"] += walk[-1] >= n_orig
        run = 0
        for prev, cur in zip(walk, walk[1:]):
            if cur >= n_orig:
                run = run + 1 if prev >= n_orig else 1
                c["dummy_runs"] += run == 2
                continue
            w = None if prev < n_orig else pairs[(prev - n_orig) >> 1][2]
            c["transitions"].add(("o" if w is None else w, cur % 2 == 0))
            offset = k - 1 if w is None else k - 1 - w
            assert 0 <= offset <= len(seqs[cur >> 1])
            c["zero_character_edges"] += w is None and len(seqs[cur >> 1]) == offset
            c["offset_zero_after_dummy"] += w is not None and offset == 0
    c["lengths"] = sorted(set(len(s) for s in seqs))
    c["start_residues"] = sorted(set(int(x) % 16 for x in np.cumsum([0] + [len(s) for s in seqs[:-1]])))
    return c


def overlap_lengths(k):
    return sorted(set(([k - 1] if k >= 2 else []) + [k, k + 1] + [n for n in (15, 16, 17, 31, 32, 33, 47, 64) if n >= k - 1]))


def overlaps(k, seed=SEED, n_unitigs=40, n_walks=300):
    rng = np.random.default_rng(seed + k)
    lengths = overlap_lengths(k)
    # every length at least three times, in an order that starts a unitig at every residue mod 16 of the concatenated store: of the
    # lengths left, shuffled, the next one is the first that ends on a residue not seen so far
    left, order, at, seen = [lengths[i % len(lengths)] for i in rng.permutation(n_unitigs)], [], 0, {0}
    while left:
        n = next((n for n in left if (at + n) % 16 not in seen), left[0])
        left.remove(n)
        order.append(n)
        at += n
        seen.add(at % 16)
    seqs = [dna(rng, n) for n in order]
    # three dummy biedges of every weight 1 .. k - 1, between unitigs drawn at random
    pairs = [(int(rng.integers(n_unitigs)), int(rng.integers(n_unitigs)), w) for w in range(1, k) for _ in range(3)]
    n_orig, n_dummy = 2 * n_unitigs, 2 * len(pairs)
    walks = []
    for _ in range(n_walks):
        walk = [int(rng.integers(n_orig))]
        for _ in range(int(rng.integers(0, 13))):
            dummy = n_dummy and rng.random() < 0.4
            walk.append(n_orig + int(rng.integers(n_dummy)) if dummy else int(rng.integers(n_orig)))
        walks.append(walk)
    c = census_of(k, seqs, pairs, walks)
    want = {(p, f) for p in ["o"] + list(range(1, k)) for f in (True, False)}
    short = []
    if c["transitions"] != want:
        short.append(f"transitions missing: {sorted(want - c['transitions'], key=str)}")
    if c["lengths"] != lengths or c["start_residues"] != list(range(16)) or not c["backwards_first"]:
        short.append(f"lengths {c['lengths']}, start residues {c['start_residues']}, backwards first edges {c['backwards_first']}")
    if k >= 2:
        short += [f"no {name}" for name in ("dummy_runs", "ends_in_dummy", "zero_character_edges", "offset_zero_after_dummy") if not c[name]]
    if short:
        raise AssertionError(f"overlaps({k}), seed {seed}: the census falls short: " + "; ".join(short))
    return Case(k, seqs, pairs, walks, c)


# ---- k = 5: positions against the edges of the workgroups and scan blocks ----
BLOCK_K = 5
_ZERO = 0  # unitig 0 has k - 1 bases: behind an original edge it adds no character


def _block_world(rng):
    """24 unitigs (unitig 0 of k - 1 bases), two dummy biedges of every weight 1 .. k - 1."""
    seqs = [dna(rng, n) for n in [BLOCK_K - 1] + [int(x) for x in rng.choice([4, 5, 6, 7, 15, 16, 17, 33], 23)]]
    pairs = [(int(rng.integers(24)), int(rng.integers(24)), w) for w in range(1, BLOCK_K) for _ in range(2)]
    return seqs, pairs


def _fill(rng, n, n_orig, n_dummy):
    """Random walks of 1 to 9 edges with exactly n positions in all."""
    walks = []
    while n > 0:
        m = min(n, int(rng.integers(1, 10)))
        walk = [int(rng.integers(n_orig))]
        for _ in range(m - 1):
            walk.append(n_orig + int(rng.integers(n_dummy)) if rng.random() < 0.3 else int(rng.integers(n_orig)))
        walks.append(walk)
        n -= m
    return walks


def _positions(walks, n_orig, seqs, pairs, k):
    """Per position: (starts a walk, bytes of sequence it adds)."""
    out = []
    for walk in walks:
        for j, e in enumerate(walk):
            if e >= n_orig:
                out.append((j == 0, 0))
                continue
            prev = walk[j - 1] if j else None
            offset = 0 if prev is None else k - 1 if prev < n_orig else k - 1 - pairs[(prev - n_orig) >> 1][2]
            out.append((j == 0, len(seqs[e >> 1]) - offset))
    return out


def edges_of_blocks(name, seed=SEED):
    assert name in BLOCK_CASES
    k = BLOCK_K
    rng = np.random.default_rng(seed + BLOCK_CASES.index(name))
    seqs, pairs = _block_world(rng)
    n_orig, n_dummy = 2 * len(seqs), 2 * len(pairs)
    orig = lambda: 2 + int(rng.integers(n_orig - 2))  # noqa: E731  (an original edge of a unitig other than the short one)
    dummy = lambda: n_orig + int(rng.integers(n_dummy))  # noqa: E731
    fill = lambda n: _fill(rng, n, n_orig, n_dummy)  # noqa: E731
    c = {}
    if name.startswith("total-"):
        # P positions and the sentinel position P behind them: P = 256 m puts the sentinel alone into the last workgroup, P = 1024 alone
        # into the last scan block; P = 256 m - 1 makes it the last position of a full block
        P = int(name.split("-")[1])
        walks = fill(P)
        c["sentinel_alone_in_workgroup"], c["sentinel_alone_in_scan_block"] = P % SP_BLOCK == 0, P % SCAN_BLOCK == 0
        c["sentinel_last_in_workgroup"], c["sentinel_last_in_scan_block"] = (P + 1) % SP_BLOCK == 0, (P + 1) % SCAN_BLOCK == 0
        want_total = P
    elif name == "walk-starts":
        # walks that start exactly at 256 m, m = 1 .. 5 (1024: also the first position of a scan block), each in front of a filled block
        walks = []
        for _ in range(5):
            walks += fill(SP_BLOCK)
        walks += fill(77)
        want_total = 5 * SP_BLOCK + 77
        starts = set(np.cumsum([0] + [len(w) for w in walks[:-1]]).tolist())
        if not {SP_BLOCK * m for m in range(1, 6)} <= starts:
            raise AssertionError("walk-starts: no walk starts at every 256 m")
        c["walk_starts_on_block_edges"] = sorted(s for s in starts if s % SP_BLOCK == 0)
    elif name == "silent-block":
        # one walk with 600 dummy edges at positions 200 .. 799: the workgroups of positions 256 .. 511 and 512 .. 767 write no byte at all,
        # the ones on either side end / begin with zero-extent positions
        walks = fill(190)
        walks.append([orig() for _ in range(10)] + [dummy() for _ in range(600)] + [orig() for _ in range(25)])
        walks += fill(300)
        want_total = 190 + 635 + 300
    else:
        # zero-extent positions on both sides of a block edge: (255, 256) = (zero-character edge, dummy), (511, 512) = (dummy, dummy),
        # (767, 768) = (zero-character, zero-character), (1023, 1024) = (dummy, dummy) on the edge of a scan block, and
        # (1279, 1280) = (zero-character, first edge of a walk). An original edge behind a dummy always adds the dummy's weight in
        # characters, so (dummy, zero-character) does not exist.
        z = lambda: _ZERO + int(rng.integers(2))  # noqa: E731  (unitig 0, either orientation)
        walks = fill(254) + [[orig(), z(), dummy(), orig()]]                 # 254 .. 257
        walks += fill(510 - 258) + [[orig(), dummy(), dummy(), orig()]]       # 510 .. 513
        walks += fill(766 - 514) + [[orig(), z(), z(), orig()]]               # 766 .. 769
        walks += fill(1022 - 770) + [[orig(), dummy(), dummy(), dummy()]]     # 1022 .. 1025 (ends in a dummy)
        walks += fill(1278 - 1026) + [[orig(), z()], [orig(), orig()]]        # 1278 .. 1281
        walks += fill(40)
        want_total = 1282 + 40
    pos = _positions(walks, n_orig, seqs, pairs, k)
    if len(pos) != want_total:
        raise AssertionError(f"{name}: {len(pos)} positions, not {want_total}")
    silent = [b for b in range(len(pos) // SP_BLOCK) if all(not s and n == 0 for s, n in pos[b * SP_BLOCK:(b + 1) * SP_BLOCK])]
    edges = [(p - 1, p) for p in range(SP_BLOCK, len(pos), SP_BLOCK) if not pos[p][0] and pos[p - 1][1] == 0 and pos[p][1] == 0 and not pos[p - 1][0]]
    c.update(positions=len(pos), silent_blocks=silent, zero_extent_block_edges=edges)
    if name == "silent-block" and (silent != [1, 2] or pos[255] != (False, 0) or pos[768] != (False, 0) or pos[199][1] == 0 or pos[800][1] == 0):
        raise AssertionError(f"silent-block: silent blocks {silent}")
    if name == "zero-extents":
        flat = [e for w in walks for e in w]
        got = {p: (("d" if flat[p - 1] >= n_orig else "z"), ("d" if flat[p] >= n_orig else "z")) for _, p in edges}
        if got != {256: ("z", "d"), 512: ("d", "d"), 768: ("z", "z"), 1024: ("d", "d")} or pos[1279] != (False, 0) or not pos[1280][0]:
            raise AssertionError(f"zero-extents: {got}")
    return Case(k, seqs, pairs, walks, c)


def many_walks(seed=SEED, n_walks=1_050_000):
    """One-edge walks over 64 short unitigs, as (limits, edges) arrays: walk numbers 1 .. 1 050 000 (every digit boundary 9 | 10 ..
    999 999 | 1 000 000 inside the text) and P + 1 = 1 050 001 > 1024 * 1024 positions, so that the block sums of the extent scan
    need a second round."""
    k = BLOCK_K
    rng = np.random.default_rng(seed)
    seqs = [dna(rng, int(n)) for n in rng.integers(k - 1, 13, 64)]
    edges = rng.integers(0, 128, n_walks).astype(np.uint32)
    limits = np.arange(1, n_walks + 1, dtype=np.uint64)
    c = {"walks": n_walks, "positions": n_walks, "digits": sorted(set(len(str(i)) for i in (1, 10, 100, 1000, 10**4, 10**5, 10**6) if i <= n_walks)),
         "scan_blocks": -(-(n_walks + 1) // SCAN_BLOCK)}
    if c["digits"] != [1, 2, 3, 4, 5, 6, 7] or c["scan_blocks"] <= SCAN_BLOCK or n_walks + 1 <= SCAN_BLOCK * SCAN_BLOCK:
        raise AssertionError(f"many_walks: {c}")
    return Case(k, seqs, [], (limits, edges), c)


# ---- the cases by name, built once per process, and their expected texts ----
NAMES = tuple(f"overlaps-{k}" for k in OVERLAP_KS) + BLOCK_CASES + ("many-walks",)
FORMATS = {"fasta": dict(gfa=False), "gfa": dict(gfa=True), "gfa-header": dict(gfa=True, header="H\tVN:Z:1.0\tKL:Z:77")}
_CASES, _EXPECTED = {}, {}


def case(name):
    if name not in _CASES:
        assert name in NAMES
        _CASES[name] = overlaps(int(name.split("-")[1])) if name.startswith("overlaps-") else many_walks() if name == "many-walks" else edges_of_blocks(name)
    return _CASES[name]


def expected(name, fmt):
    """spell_ref's text of a case in one of FORMATS (computed once, shared by the tests of a process, never changed)."""
    import spell_ref

    if (name, fmt) not in _EXPECTED:
        c = case(name)
        _EXPECTED[name, fmt] = spell_ref.spell_ref(c.k, c.seqs, c.n_orig, c.dummy_weights, c.walk_lists(), **FORMATS[fmt])
    return _EXPECTED[name, fmt]
