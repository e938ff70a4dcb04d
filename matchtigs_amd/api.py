"""Host-side mirror of the reference's operator interface for the greedy-matchtigs / eulertigs path.

Names, argument meaning and error behaviour follow the reference crate (citations into
/root/reference/src/):

* ``TigAlgorithm.compute_tigs(graph, configuration) -> walks``   implementation/mod.rs:49-59
* ``GreedytigAlgorithm`` / ``GreedytigAlgorithmConfiguration``  implementation/greedytigs/mod.rs:33-90
* ``EulertigAlgorithm`` / ``EulertigAlgorithmConfiguration``    implementation/eulertigs/mod.rs:18-45
* ``HeapType`` / ``NodeWeightArrayType`` / ``PerformanceDataType`` (+ ``from_str``) implementation/mod.rs:61-126
* ``MatchtigEdgeData`` view (``weight / is_dummy / is_original / is_forwards / is_backwards / mirror``)
  implementation/mod.rs:287-317
* the C-ABI of src/clib.rs through ``ClibGraph``.

Everything computes through libmatchtigs.so (HIP). PyTorch is only used by callers that want to own
device buffers (bench.py, multi-GPU); this module itself never imports torch.
"""
from __future__ import annotations

import ctypes as C
import enum
import json
import os
import re
from dataclasses import dataclass
from typing import Iterable, Optional, Sequence

import numpy as np

from . import _lib


# ---- configuration enums (implementation/mod.rs:61-126) ---------------------------------------
class _FromStr(enum.Enum):
    @classmethod
    def from_str(cls, s: str):
        for m in cls:
            if m.value == s:
                return m
        raise ValueError(f"Unknown {cls._label}: {s}")  # Err(format!("Unknown ...: {other}"))


class NodeWeightArrayType(_FromStr):
    EpochNodeWeightArray = "EpochNodeWeightArray"
    HashbrownHashMap = "HashbrownHashMap"


NodeWeightArrayType._label = "node weight array type"


class HeapType(_FromStr):
    StdBinaryHeap = "StdBinaryHeap"


HeapType._label = "heap type"


class PerformanceDataType(_FromStr):
    None_ = "None"
    Complete = "Complete"


PerformanceDataType._label = "performance data type"


class EulerMode(enum.IntEnum):
    """Engine-only option (mtg_config.euler_mode): HostReferenceOrder = the reference's walk order (bit-exact tigs);
    Device = parallel Euler bicycles on the GPU (valid walks, same #tigs / cumulative length, different order)."""

    HostReferenceOrder = 0
    Device = 1


class FinishStage(enum.IntEnum):
    """Engine-only option (mtg_config.finish_stage): where dummy insertion, the Euleriser and the cutter run. Auto = on the GPU
    whenever one is visible (same edges and tigs as the host stages)."""

    Auto = 0
    Host = 1
    Device = 2


@dataclass
class GreedytigAlgorithmConfiguration:
    """greedytigs/mod.rs:40-73. heap / node-weight-array / staged-parallelism settings select CPU data
    structures in the reference and never change results; the MI355X engine validates and otherwise ignores them.
    ``threads`` likewise: results always equal the reference's 1-thread order (its only deterministic one).
    ``euler_mode`` / ``device_ids`` are engine-only fields (mtg_config)."""

    threads: int
    k: int
    staged_parallelism_divisor: Optional[float] = None
    resource_limit_factor: int = 0
    node_weight_array_type: NodeWeightArrayType = NodeWeightArrayType.HashbrownHashMap
    heap_type: HeapType = HeapType.StdBinaryHeap
    performance_data_type: PerformanceDataType = PerformanceDataType.None_
    euler_mode: EulerMode = EulerMode.HostReferenceOrder
    device_ids: Sequence[int] = (0,)
    finish_stage: FinishStage = FinishStage.Auto

    @classmethod
    def new(cls, threads: int, k: int) -> "GreedytigAlgorithmConfiguration":
        return cls(threads, k)

    def to_c(self) -> "_lib.MtgConfig":
        c = _lib.MtgConfig()
        _lib.load().mtg_config_init(C.byref(c), self.threads, self.k)
        c.staged_parallelism_divisor = float(self.staged_parallelism_divisor or 0.0)
        c.resource_limit_factor = self.resource_limit_factor
        c.node_weight_array_type = list(NodeWeightArrayType).index(self.node_weight_array_type)
        c.heap_type = list(HeapType).index(self.heap_type)
        c.performance_data_type = list(PerformanceDataType).index(self.performance_data_type)
        c.euler_mode = int(self.euler_mode)
        c.finish_stage = int(self.finish_stage)
        c.n_devices = len(self.device_ids)
        for i, dv in enumerate(self.device_ids):
            c.device_ids[i] = int(dv)
        return c


@dataclass
class EulertigAlgorithmConfiguration:
    """eulertigs/mod.rs:42-45 (+ the engine-only euler_mode / device_id)."""

    k: int
    euler_mode: EulerMode = EulerMode.HostReferenceOrder
    device_id: int = 0
    finish_stage: FinishStage = FinishStage.Auto

    def to_c(self) -> "_lib.MtgConfig":
        return GreedytigAlgorithmConfiguration(1, self.k, euler_mode=self.euler_mode, device_ids=(self.device_id,),
                                               finish_stage=self.finish_stage).to_c()


@dataclass
class MatchtigAlgorithmConfiguration:
    """matchtigs/mod.rs:33-45 (+ the engine-only euler_mode / device_id). ``matcher_path`` is the external blossom5-compatible
    executable (`<matcher> -e <instance> -w <solution>`); the instance goes to ``<matching_file_prefix>.minimalperfectmatching``."""

    threads: int
    k: int
    matching_file_prefix: str
    matcher_path: str
    euler_mode: EulerMode = EulerMode.HostReferenceOrder
    device_id: int = 0

    def to_c(self) -> "_lib.MtgConfig":
        c = GreedytigAlgorithmConfiguration(self.threads, self.k, euler_mode=self.euler_mode, device_ids=(self.device_id,)).to_c()
        self._keep = (str(self.matching_file_prefix).encode(), str(self.matcher_path).encode())  # c_char_p fields borrow these
        c.matching_file_prefix, c.matcher_path = self._keep
        return c


# ---- edge payload view (implementation/mod.rs:287-317; clib.rs:45-85) -------------------------
@dataclass(frozen=True)
class MatchtigEdgeData:
    sequence_handle: int  # unitig id; 0 (= Default) for dummy edges
    forwards: bool
    _weight: int
    dummy_edge_id: int

    def weight(self) -> int:
        return self._weight

    def is_dummy(self) -> bool:
        return self.dummy_edge_id != 0

    def is_original(self) -> bool:
        return not self.is_dummy()

    def is_forwards(self) -> bool:
        return self.forwards

    def is_backwards(self) -> bool:
        return not self.forwards

    def mirror(self) -> "MatchtigEdgeData":
        return MatchtigEdgeData(self.sequence_handle, not self.forwards, self._weight, self.dummy_edge_id)

    @classmethod
    def new(cls, sequence_handle: int, forwards: bool, weight: int, dummy_id: int) -> "MatchtigEdgeData":
        return cls(sequence_handle, forwards, weight, dummy_id)


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Bigraph:
    """Edge-centric bigraph handle (replaces ``NodeBigraphWrapper<PetGraph<(), EdgeData>>``).

    compute_tigs mutates it (dummy edges are appended) exactly like the reference mutates its graph
    (greedytigs/mod.rs:678-689, implementation/mod.rs:492-493), and the returned walks index the mutated graph.
    """

    def __init__(self, handle: int):
        self._h = handle
        self._L = _lib.load()

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._L.mtg_graph_free(h)

    @classmethod
    def from_edges(cls, mirror, edge_from, edge_to, edge_weight) -> "Bigraph":
        L = _lib.load()
        m = np.ascontiguousarray(mirror, dtype=np.uint32)
        f = np.ascontiguousarray(edge_from, dtype=np.uint32)
        t = np.ascontiguousarray(edge_to, dtype=np.uint32)
        w = np.ascontiguousarray(edge_weight, dtype=np.uint64)
        if not (len(f) == len(t) == len(w)):
            raise ValueError("edge arrays differ in length")
        return cls(L.mtg_graph_from_edges(len(m), _ptr(m), len(f), _ptr(f), _ptr(t), _ptr(w)))

    @classmethod
    def from_unitig_links(cls, unitig_weights, links: Iterable[Sequence]) -> "Bigraph":
        """The clib.rs builder: links = (unitig_a, strand_a, unitig_b, strand_b)."""
        L = _lib.load()
        w = np.ascontiguousarray(unitig_weights, dtype=np.uint64)
        h = L.mtg_graph_builder_new(len(w))
        for (ua, sa, ub, sb) in links:
            L.mtg_graph_builder_merge(h, int(ua), 1 if sa else 0, int(ub), 1 if sb else 0)
        L.mtg_graph_builder_build(h, _ptr(w))
        return cls(h)

    @classmethod
    def from_unitig_links_arrays(cls, unitig_weights, links) -> "Bigraph":
        """The clib.rs builder over an int array [n, 4] of links (one call instead of one per link)."""
        L = _lib.load()
        w = np.ascontiguousarray(unitig_weights, dtype=np.uint64)
        lk = np.ascontiguousarray(links, dtype=np.int64)
        if lk.ndim != 2 or (len(lk) and lk.shape[1] != 4):
            raise ValueError("links must have shape [n, 4]")
        h = L.mtg_graph_builder_new(len(w))
        L.mtg_graph_builder_merge_links(h, len(lk), _ptr(lk) if len(lk) else None)
        L.mtg_graph_builder_build(h, _ptr(w))
        return cls(h)

    @classmethod
    def from_sequences(cls, seqs, k: int, device_id: int = 0) -> "Bigraph":
        """The plain-FASTA graph (`--fa-in`, read_fasta) of sequences held in memory: a list of str / bytes, or (data, offsets) with
        record u = data[offsets[u]:offsets[u + 1]] (data: bytes or a uint8 array, offsets: U + 1 values from 0). Joined on the GPU."""
        L = _lib.load()
        if isinstance(seqs, tuple) and len(seqs) == 2:
            data, off = seqs
            data = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8)
            off = np.ascontiguousarray(off, dtype=np.uint64)
        else:
            parts = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
            data = np.frombuffer(b"".join(parts), np.uint8)
            off = np.zeros(len(parts) + 1, np.uint64)
            np.cumsum([len(p) for p in parts], out=off[1:])
        if len(off) < 1 or int(off[0]) != 0 or int(off[-1]) > len(data):
            raise ValueError("offsets must start at 0 and end inside the data")
        data = np.ascontiguousarray(data) if len(data) else np.zeros(1, np.uint8)
        return cls(L.mtg_graph_from_sequences(_ptr(data), _ptr(off), len(off) - 1, k, device_id))

    @property
    def handle(self) -> int:
        return self._h

    def release_device_cache(self) -> None:
        """mtg_graph_release_device_cache: the device copy of the original edges (+ their buckets) goes back to the driver."""
        self._L.mtg_graph_release_device_cache(self._h)

    def reset(self) -> None:
        """Drop all dummy edges again (the reference clones its graph instead, bin.rs:1069)."""
        self._L.mtg_graph_reset(self._h)

    def node_count(self) -> int:
        return int(self._L.mtg_graph_node_count(self._h))

    def edge_count(self) -> int:
        return int(self._L.mtg_graph_edge_count(self._h))

    def export(self) -> dict:
        V, E = self.node_count(), self.edge_count()
        out = {
            "mirror": np.zeros(V, np.uint32), "edge_from": np.zeros(E, np.uint32), "edge_to": np.zeros(E, np.uint32),
            "edge_weight": np.zeros(E, np.uint64), "edge_dummy_id": np.zeros(E, np.uint64),
            "edge_unitig": np.zeros(E, np.uint64), "edge_forwards": np.zeros(E, np.uint8),
        }
        self._L.mtg_graph_export(self._h, *[_ptr(out[k]) for k in
                                            ("mirror", "edge_from", "edge_to", "edge_weight", "edge_dummy_id",
                                             "edge_unitig", "edge_forwards")])
        return out

    _EXPORT_FIELDS = (("edge_from", np.uint32), ("edge_to", np.uint32), ("edge_weight", np.uint64), ("edge_dummy_id", np.uint64),
                      ("edge_unitig", np.uint64), ("edge_forwards", np.uint8))

    def export_mirror(self) -> np.ndarray:
        m = np.empty(self.node_count(), np.uint32)
        self._L.mtg_graph_export(self._h, _ptr(m), None, None, None, None, None, None)
        return m

    def original_edge_count(self) -> int:
        return int(self._L.mtg_graph_original_edge_count(self._h))

    def export_range(self, first_edge: int, n_edges: int, fields: Sequence[str]) -> dict:
        """Selected edge arrays of the edges [first_edge, first_edge + n_edges) (mtg_graph_export_range)."""
        out = {name: np.empty(n_edges, dt) for name, dt in self._EXPORT_FIELDS if name in fields}
        self._L.mtg_graph_export_range(self._h, first_edge, n_edges, *[_ptr(out.get(name)) for name, _ in self._EXPORT_FIELDS])
        return out

    def edge_data(self, e: int, _cache={}) -> MatchtigEdgeData:
        ex = self.export()
        return MatchtigEdgeData(int(ex["edge_unitig"][e]), bool(ex["edge_forwards"][e]), int(ex["edge_weight"][e]),
                                int(ex["edge_dummy_id"][e]))

    # ---- host sub-stages (exported for parity tests) ----
    def replay_claims(self, out_nodes, multiplicity, is_in_node, cand_start, cand_count, pool) -> np.ndarray:
        on = np.ascontiguousarray(out_nodes, np.uint32)
        mu = np.ascontiguousarray(multiplicity, np.int32)
        li = np.ascontiguousarray(is_in_node, np.uint8)
        cs = np.ascontiguousarray(cand_start, np.uint64)
        cc = np.ascontiguousarray(cand_count, np.uint32)
        po = np.ascontiguousarray(pool, np.uint64)
        if len(mu) != self.node_count() or len(li) != self.node_count():
            raise ValueError("classification arrays must have node_count entries")
        pp = C.POINTER(_lib.MtgPair)()
        n = self._L.mtg_replay_claims(self._h, len(on), _ptr(on), _ptr(mu), _ptr(li), _ptr(cs), _ptr(cc), _ptr(po), C.byref(pp))
        dt = np.dtype([("out", np.uint32), ("in", np.uint32), ("dist", np.uint64)])
        arr = np.zeros(n, dt)
        if n:
            C.memmove(arr.ctypes.data, pp, n * C.sizeof(_lib.MtgPair))
        self._L.mtg_free(pp)
        return arr

    def insert_pair_edges(self, pairs: np.ndarray) -> int:
        p = np.ascontiguousarray(pairs)
        return int(self._L.mtg_insert_pair_edges(self._h, _ptr(p), len(p)))

    def make_eulerian(self, dummy_edge_id: int, k: int) -> int:
        return int(self._L.mtg_make_eulerian(self._h, dummy_edge_id, k))

    def euler_cycles(self) -> list[list[int]]:
        return _take_walks(self._L, self._L.mtg_euler_cycles(self._h))

    def euler_cycles_records(self, record_format: int) -> list[list[int]]:
        """mtg_euler_cycles_records: 0 = wide records from adjacency, 1 = 32-byte records, 2 = wide (256-byte) records seeded from
        32-byte ones, 3 = 128-byte records seeded from 32-byte ones."""
        return _take_walks(self._L, self._L.mtg_euler_cycles_records(self._h, record_format))

    def euler_cycles_device(self, device_id: int = 0) -> list[list[int]]:
        """Euler bicycles on the GPU (valid walks, not the reference's order)."""
        return _take_walks(self._L, self._L.mtg_euler_cycles_device(self._h, device_id))

    def euler_cycles_device_np(self, device_id: int = 0):
        """(limits, edges) arrays of the GPU Euler bicycles."""
        return _take_walks_np(self._L, self._L.mtg_euler_cycles_device(self._h, device_id))

    def cut_cycles(self, cycles: list[list[int]], k: int) -> list[list[int]]:
        """greedytigs/mod.rs:726-789 on given closed walks (edge ids into this graph)."""
        ed = np.fromiter((e for c in cycles for e in c), dtype=np.uint32)
        lim = np.cumsum([len(c) for c in cycles], dtype=np.uint64) if len(cycles) else np.zeros(0, np.uint64)
        w = self._L.mtg_walks_from_arrays(len(lim), _ptr(lim) if len(lim) else None, _ptr(ed) if len(ed) else None)
        try:
            return _take_walks(self._L, self._L.mtg_cut_cycles(self._h, w, k))
        finally:
            self._L.mtg_walks_free(w)

    def finish_greedytigs(self, pairs: np.ndarray, k: int) -> list[list[int]]:
        p = np.ascontiguousarray(pairs)
        return _take_walks(self._L, self._L.mtg_finish_greedytigs(self._h, _ptr(p), len(p), k))

    def flatten_clib(self, tigs: list[list[int]]):
        """clib.rs:393-407 on already-computed walks (recomputed through the C-ABI for algorithm output)."""
        ex = self.export()
        eo, io, lim = [], [], []
        for t in tigs:
            for e in t:
                eo.append(int(ex["edge_unitig"][e]) * (1 if ex["edge_forwards"][e] else -1))
                io.append(0 if ex["edge_dummy_id"][e] == 0 else int(ex["edge_weight"][e]))
            lim.append(len(eo))
        return eo, io, lim


def _take_walks(L, wp) -> list[list[int]]:
    n, tot = int(L.mtg_walks_count(wp)), int(L.mtg_walks_total_edges(wp))
    lim = np.zeros(max(n, 1), np.uint64)
    ed = np.zeros(max(tot, 1), np.uint32)
    L.mtg_walks_export(wp, _ptr(lim), _ptr(ed))
    L.mtg_walks_free(wp)
    out, b = [], 0
    for i in range(n):
        out.append(ed[b:int(lim[i])].tolist())
        b = int(lim[i])
    return out


def _take_walks_np(L, wp):
    """(limits, edges) as numpy VIEWS of the library's walk arrays (no copy: 0.5 GB at the bench size); the walks are freed when
    both views are gone."""
    import weakref

    n, tot = int(L.mtg_walks_count(wp)), int(L.mtg_walks_total_edges(wp))
    if n and tot:
        lp, ep = C.c_void_p(), C.c_void_p()
        L.mtg_walks_data(wp, C.byref(lp), C.byref(ep))
        left = [2]

        def done():
            left[0] -= 1
            if left[0] == 0:
                L.mtg_walks_free(C.c_void_p(wp))

        raw_l = (C.c_char * (n * 8)).from_address(lp.value)
        raw_e = (C.c_char * (tot * 4)).from_address(ep.value)
        weakref.finalize(raw_l, done)
        weakref.finalize(raw_e, done)
        return np.frombuffer(raw_l, dtype=np.uint64), np.frombuffer(raw_e, dtype=np.uint32)
    lim = np.zeros(n, np.uint64)
    ed = np.zeros(tot, np.uint32)
    L.mtg_walks_export(wp, _ptr(lim) if n else None, _ptr(ed) if tot else None)
    L.mtg_walks_free(wp)
    return lim, ed


class DeviceGraph:
    """One GPU's resident copy of a Bigraph (mtg_device). Raises/aborts without a GPU: no CPU path."""

    def __init__(self, graph: Bigraph, k: int, device_id: int = 0, lower_bounds: bool = True, reserve_work: bool = False):
        """lower_bounds=False: mtg_device_create_opts(MTG_DEVICE_NO_LOWER_BOUNDS) -- the device graph of a caller that searches once
        (what mtg_compute_tigs_cfg builds); build_lower_bounds() adds them later. reserve_work=True: MTG_DEVICE_RESERVE_WORK -- the
        device memory the stages of a step take beside the graph is reserved now, in one piece (a caller that steps through the stages)."""
        self._L = _lib.load()
        if self._L.mtg_device_count() <= device_id:
            raise RuntimeError(f"no HIP device {device_id}: the matchtigs_amd device stage has no CPU fallback")
        self.graph = graph
        self.k = k
        self._d = self._L.mtg_device_create_opts(graph.handle, k, device_id, (0 if lower_bounds else 1) | (2 if reserve_work else 0))
        self.n_sources = None

    def build_lower_bounds(self, stream: int = 0) -> float:
        """mtg_device_build_lower_bounds; returns the GPU milliseconds of the precompute (mtg_device_lower_bounds_ms)."""
        self._L.mtg_device_build_lower_bounds(self._d, stream)
        return self.lower_bounds_ms()

    def lower_bounds_ms(self) -> float:
        return float(self._L.mtg_device_lower_bounds_ms(self._d))

    def __del__(self):
        d, self._d = getattr(self, "_d", None), None
        if d:
            self._L.mtg_device_free(d)

    @property
    def handle(self) -> int:
        return self._d

    def graph_bytes(self) -> int:
        return int(self._L.mtg_device_graph_bytes(self._d))

    def classify(self, stream: int = 0) -> int:
        self.n_sources = int(self._L.mtg_classify(self._d, stream))
        return self.n_sources

    def classify_download(self, stream: int = 0):
        V = self.graph.node_count()
        on = np.zeros(self.n_sources, np.uint32)
        mu = np.zeros(V, np.int32)
        li = np.zeros(V, np.uint8)
        self._L.mtg_classify_download(self._d, stream, _ptr(on) if len(on) else None, _ptr(mu) if V else None,
                                      _ptr(li) if V else None)
        return on, mu, li

    def sssp_candidates(self, src_begin: int, src_end: int, d_pool: int, pool_capacity: int, d_cand_start: int,
                        d_cand_count: int, stream: int = 0):
        """Device pointers in, returns (status, pool_needed). status 1 = pool too small."""
        needed = C.c_uint64()
        rc = self._L.mtg_sssp_candidates(self._d, stream, src_begin, src_end, d_pool, pool_capacity, d_cand_start,
                                         d_cand_count, C.byref(needed))
        return int(rc), int(needed.value)

    def last_sssp_kernel_ms(self) -> float:
        return float(self._L.mtg_last_sssp_kernel_ms(self._d))

    def replay_claims_device(self, d_cand_start: int, d_cand_count: int, d_pool: int, stream: int = 0) -> np.ndarray:
        """The claim loop on the GPU over device-resident candidate arrays of ALL sources -> pairs (host numpy)."""
        pp = C.POINTER(_lib.MtgPair)()
        n = self._L.mtg_replay_claims_device(self._d, stream, self.n_sources, d_cand_start, d_cand_count, d_pool, C.byref(pp))
        return _adopt_pairs(self._L, pp, n)

    def replay_claims_resident(self, d_cand_start: int, d_cand_count: int, d_pool: int, stream: int = 0) -> int:
        """The claim loop on the GPU; the pairs stay in HBM for finish_greedytigs_resident_np. Returns their number."""
        return int(self._L.mtg_replay_claims_resident(self._d, stream, self.n_sources, d_cand_start, d_cand_count, d_pool))

    def download_resident_pairs(self) -> np.ndarray:
        pp = C.POINTER(_lib.MtgPair)()
        n = self._L.mtg_download_resident_pairs(self._d, C.byref(pp))
        return _adopt_pairs(self._L, pp, n)

    def set_replay_tuning(self, windows: int = 0, block: int = 0, grid: int = 0, role_mod: int = 0, plain_barrier: bool = False) -> None:
        """mtg_set_replay_tuning: launch geometry of the claim replay (0 = the engine's choice); never changes the pair list."""
        self._L.mtg_set_replay_tuning(self._d, windows, block, grid, role_mod, 1 if plain_barrier else 0)

    def last_replay_ms(self) -> dict:
        out = (C.c_double * 2)()
        self._L.mtg_last_replay_ms(self._d, out)
        return {"rounds_kernel_ms": float(out[0]), "gpu_ms": float(out[1])}

    def last_replay_rounds(self) -> int:
        return int(self._L.mtg_last_replay_rounds(self._d))

    def last_replay_visits(self) -> int:
        return int(self._L.mtg_last_replay_visits(self._d))

    def last_sssp_levels(self) -> list[dict]:
        ms = (C.c_double * 8)()
        src = (C.c_uint64 * 8)()
        n = self._L.mtg_last_sssp_levels(self._d, ms, src, 8)
        return [{"level": i, "ms": float(ms[i]), "sources": int(src[i]),
                 "kernel": self._L.mtg_last_sssp_level_name(self._d, i).decode()} for i in range(n)]

    def sssp_count(self, src_begin: int, src_end: int, stream: int = 0) -> dict:
        st = _lib.MtgSsspStats()
        self._L.mtg_sssp_count(self._d, stream, src_begin, src_end, C.byref(st))
        return st.as_dict()

    def sssp_count_visited(self, src_begin: int, src_end: int, stream: int = 0) -> dict:
        """Units of the search the default plan really runs (goal-directed pruning; mtg_engine.h): sources = sources searched."""
        st = _lib.MtgSsspStats()
        self._L.mtg_sssp_count_visited(self._d, stream, src_begin, src_end, C.byref(st))
        return st.as_dict()

    def prunes(self) -> bool:
        return bool(self._L.mtg_sssp_prunes(self._d))

    def last_searched_sources(self) -> int:
        return int(self._L.mtg_last_sssp_searched_sources(self._d))

    def set_plan(self, plan: int) -> int:
        """0 = default (path enumeration level + cooperative cascade), 1 = cooperative cascade only, 2 / 3 = plan 0 with
        quad-cooperative / per-lane block gathers regardless of the graph size, + 4 = without the goal-directed pruning, + 8 = the
        enumeration level on one workgroup (tests) (mtg_engine.h)."""
        return int(self._L.mtg_set_sssp_plan(self._d, plan))


def compute_pairs(devices: Sequence[DeviceGraph]) -> np.ndarray:
    """mtg_compute_pairs: SSSP sharded over the given (classified) device copies of one graph, gather on the first, claim replay."""
    L = _lib.load()
    arr = (C.c_void_p * len(devices))(*[d.handle for d in devices])
    pp = C.POINTER(_lib.MtgPair)()
    n = L.mtg_compute_pairs(arr, len(devices), C.byref(pp))
    return _adopt_pairs(L, pp, n)


def partition_sources(device: DeviceGraph, parts: int) -> list[int]:
    cuts = (C.c_uint64 * (parts + 1))()
    _lib.load().mtg_partition_sources(device.handle, parts, cuts)
    return [int(x) for x in cuts]


PAIR_DTYPE = np.dtype([("out", np.uint32), ("in", np.uint32), ("dist", np.uint64)])


def _adopt_pairs(L, pp, n: int) -> np.ndarray:
    """A numpy view of the library's malloc'd mtg_pair array (no copy); mtg_free runs when the last view is gone."""
    import weakref

    if not n:
        L.mtg_free(pp)
        return np.zeros(0, PAIR_DTYPE)
    addr = C.cast(pp, C.c_void_p).value
    raw = (C.c_char * (n * C.sizeof(_lib.MtgPair))).from_address(addr)
    weakref.finalize(raw, L.mtg_free, C.c_void_p(addr))
    return np.frombuffer(raw, dtype=PAIR_DTYPE)


class TigAlgorithm:
    """implementation/mod.rs:49-59."""

    Configuration = None

    @classmethod
    def compute_tigs(cls, graph: Bigraph, configuration) -> list[list[int]]:
        raise NotImplementedError


class GreedytigAlgorithm(TigAlgorithm):
    """greedytigs/mod.rs:75-90: walks of edge ids into the (mutated) graph."""

    Configuration = GreedytigAlgorithmConfiguration

    @classmethod
    def compute_tigs(cls, graph: Bigraph, configuration: GreedytigAlgorithmConfiguration):
        L = _lib.load()
        c = configuration.to_c()
        return _take_walks(L, L.mtg_compute_tigs_cfg(graph.handle, 5, C.byref(c)))

    @classmethod
    def compute_tigs_np(cls, graph: Bigraph, configuration: GreedytigAlgorithmConfiguration):
        """The same as flat numpy arrays (exclusive tig ends, edge ids): large graphs."""
        L = _lib.load()
        c = configuration.to_c()
        return _take_walks_np(L, L.mtg_compute_tigs_cfg(graph.handle, 5, C.byref(c)))


class EulertigAlgorithm(TigAlgorithm):
    """eulertigs/mod.rs:18-39."""

    Configuration = EulertigAlgorithmConfiguration

    @classmethod
    def compute_tigs(cls, graph: Bigraph, configuration: EulertigAlgorithmConfiguration):
        L = _lib.load()
        c = configuration.to_c()
        return _take_walks(L, L.mtg_compute_eulertigs_cfg(graph.handle, C.byref(c)))

    @classmethod
    def compute_tigs_np(cls, graph: Bigraph, configuration: EulertigAlgorithmConfiguration):
        L = _lib.load()
        c = configuration.to_c()
        return _take_walks_np(L, L.mtg_compute_eulertigs_cfg(graph.handle, C.byref(c)))


class MatchingInstance:
    """The minimum-perfect-matching instance of optimal matchtigs (matchtigs/mod.rs:150-719), built from the GPU's candidate
    lists: ``write`` produces the matcher's input file, ``read_solution`` turns the matcher's output into matched pairs."""

    def __init__(self, graph: Bigraph, k: int, device_id: int = 0, _handle=None):
        self._L = _lib.load()
        if _handle is not None:
            self._m = _handle
            return
        c = GreedytigAlgorithmConfiguration(1, k, device_ids=(device_id,)).to_c()
        self._m = self._L.mtg_matching_instance(graph.handle, C.byref(c))

    @classmethod
    def from_lists(cls, graph: Bigraph, k: int, out_nodes, multiplicity, cand_start, cand_count, pool) -> "MatchingInstance":
        """The host stage alone over caller-held candidate lists (mtg_matching_instance_from_lists)."""
        L = _lib.load()
        on = np.ascontiguousarray(out_nodes, np.uint32)
        mu = np.ascontiguousarray(multiplicity, np.int32)
        cs = np.ascontiguousarray(cand_start, np.uint64)
        cc = np.ascontiguousarray(cand_count, np.uint32)
        po = np.ascontiguousarray(pool, np.uint64)
        h = L.mtg_matching_instance_from_lists(graph.handle, k, len(on), _ptr(on) if len(on) else None, _ptr(mu),
                                               _ptr(cs) if len(cs) else None, _ptr(cc) if len(cc) else None,
                                               _ptr(po) if len(po) else None)
        return cls(graph, k, _handle=h)

    def stats(self) -> dict:
        st = _lib.MtgMatchingStats()
        self._L.mtg_matching_get_stats(self._m, C.byref(st))
        return st.as_dict()

    def write(self, path: str) -> int:
        return int(self._L.mtg_matching_write(self._m, str(path).encode()))

    def read_solution(self, path: str) -> np.ndarray:
        pp = C.POINTER(_lib.MtgPair)()
        n = self._L.mtg_matching_read_solution(self._m, str(path).encode(), C.byref(pp))
        arr = np.zeros(n, np.dtype([("out", np.uint32), ("in", np.uint32), ("dist", np.uint64)]))
        if n:
            C.memmove(arr.ctypes.data, pp, n * C.sizeof(_lib.MtgPair))
        self._L.mtg_free(pp)
        return arr

    def close(self):
        if self._m:
            self._L.mtg_matching_free(self._m)
            self._m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MatchtigAlgorithm(TigAlgorithm):
    """matchtigs/mod.rs:47-62: optimal matchtigs; the matching itself is solved by the external matcher the configuration names."""

    Configuration = MatchtigAlgorithmConfiguration

    @classmethod
    def compute_tigs(cls, graph: Bigraph, configuration: MatchtigAlgorithmConfiguration):
        L = _lib.load()
        c = configuration.to_c()
        return _take_walks(L, L.mtg_compute_matchtigs_cfg(graph.handle, C.byref(c)))

    @staticmethod
    def finish(graph: Bigraph, pairs: np.ndarray, k: int):
        """matchtigs/mod.rs:797-935 on already matched pairs (mtg_finish_matchtigs_cfg)."""
        L = _lib.load()
        p = np.ascontiguousarray(pairs)
        c = GreedytigAlgorithmConfiguration(1, k).to_c()
        return _take_walks(L, L.mtg_finish_matchtigs_cfg(graph.handle, _ptr(p) if len(p) else None, len(p), C.byref(c)))


def finish_greedytigs_np(graph: Bigraph, pairs: np.ndarray, k: int, euler_mode: EulerMode = EulerMode.HostReferenceOrder,
                         device_id: int = 0, finish_stage: FinishStage = FinishStage.Auto):
    """mtg_finish_greedytigs_cfg returning flat numpy walks (limits, edges) -- for large graphs."""
    L = _lib.load()
    p = np.ascontiguousarray(pairs)
    c = GreedytigAlgorithmConfiguration(1, k, euler_mode=euler_mode, device_ids=(device_id,), finish_stage=finish_stage).to_c()
    return _take_walks_np(L, L.mtg_finish_greedytigs_cfg(graph.handle, _ptr(p) if len(p) else None, len(p), C.byref(c)))


class Tigs:
    """Handle of a tig set (mtg_walks). After a finish on the GPU the tigs are still in HBM: count() and total_edges() cost nothing,
    arrays() brings them to the host -- once, through the pinned ring -- and returns (limits, edges) as views of the library's arrays
    (valid while this object lives)."""

    def __init__(self, L, wp):
        self._L, self._wp = L, wp

    def __del__(self):
        wp, self._wp = getattr(self, "_wp", None), None
        if wp:
            self._L.mtg_walks_free(C.c_void_p(wp))

    def count(self) -> int:
        return int(self._L.mtg_walks_count(self._wp))

    def total_edges(self) -> int:
        return int(self._L.mtg_walks_total_edges(self._wp))

    def arrays(self):
        n, tot = self.count(), self.total_edges()
        if not (n and tot):
            return np.zeros(n, np.uint64), np.zeros(tot, np.uint32)
        lp, ep = C.c_void_p(), C.c_void_p()
        self._L.mtg_walks_data(self._wp, C.byref(lp), C.byref(ep))
        lim = np.frombuffer((C.c_char * (n * 8)).from_address(lp.value), dtype=np.uint64)
        ed = np.frombuffer((C.c_char * (tot * 4)).from_address(ep.value), dtype=np.uint32)
        self._views = (lim, ed)
        return lim, ed


def finish_greedytigs_resident(graph: Bigraph, device: "DeviceGraph", k: int, euler_mode: EulerMode = EulerMode.HostReferenceOrder,
                               device_id: int = 0, finish_stage: FinishStage = FinishStage.Auto) -> Tigs:
    """mtg_finish_greedytigs_resident as a handle: the tigs of a finish on the GPU stay in HBM until Tigs.arrays() asks for them."""
    L = _lib.load()
    c = GreedytigAlgorithmConfiguration(1, k, euler_mode=euler_mode, device_ids=(device_id,), finish_stage=finish_stage).to_c()
    return Tigs(L, L.mtg_finish_greedytigs_resident(graph.handle, device.handle, C.byref(c)))


def finish_greedytigs_resident_np(graph: Bigraph, device: "DeviceGraph", k: int, euler_mode: EulerMode = EulerMode.HostReferenceOrder,
                                  device_id: int = 0, finish_stage: FinishStage = FinishStage.Auto):
    """mtg_finish_greedytigs_resident: the finish over the pairs the last replay_claims_resident left on the GPU."""
    L = _lib.load()
    c = GreedytigAlgorithmConfiguration(1, k, euler_mode=euler_mode, device_ids=(device_id,), finish_stage=finish_stage).to_c()
    return _take_walks_np(L, L.mtg_finish_greedytigs_resident(graph.handle, device.handle, C.byref(c)))


RECORD_FORMATS = {None: 0, "auto": 0, "lean": 1, "mid": 2, "wide": 3}


def set_finish_tuning(records=None, wait_for_records: bool = False, no_pin: bool = False, no_edge_cache: bool = False,
                      record_delay_us: int = 0, keep_awake: bool = False, no_cut_first: bool = False) -> None:
    """mtg_set_finish_tuning: walk-record format of the reference-order mode ("lean" 32-byte / "mid" 128-byte / "wide" 256-byte
    records, None = the engine's choice), whether the walk waits for all of its records, page-locking, the graph's device cache, and
    a delay per arriving slice of records (tests). Process-wide; never changes a result."""
    flags = (1 if wait_for_records else 0) | (2 if no_pin else 0) | (4 if no_edge_cache else 0) | (8 if keep_awake else 0) | (16 if no_cut_first else 0)
    _lib.load().mtg_set_finish_tuning(RECORD_FORMATS[records], flags, int(record_delay_us))


def set_default_device(device_id: int) -> None:
    """mtg_set_default_device: the GPU whose memory a graph's construction reserves ahead of the call that follows."""
    _lib.load().mtg_set_default_device(device_id)


def set_reserve_ahead(on: bool) -> None:
    """mtg_set_reserve_ahead: False = host-only graph constructors reserve nothing on any GPU (no helper thread)."""
    _lib.load().mtg_set_reserve_ahead(1 if on else 0)


def release_device_memory(device_id: int = 0) -> None:
    """mtg_release_device_memory: the work arrays the finishing stages keep on that GPU between calls."""
    _lib.load().mtg_release_device_memory(device_id)


def device_arena_stats(device_id: int = 0, reset_peak: bool = False) -> dict:
    """mtg_device_arena_stats: bytes in chunks, bytes live, peak of live bytes since the last reset, driver allocations so far."""
    a = (C.c_uint64 * 4)()
    _lib.load().mtg_device_arena_stats(device_id, a, 1 if reset_peak else 0)
    return {"chunk_bytes": int(a[0]), "live_bytes": int(a[1]), "peak_bytes": int(a[2]), "driver_allocations": int(a[3])}


def device_memory_held(device_id: int = 0) -> int:
    return int(_lib.load().mtg_device_memory_held(device_id))


def last_finish_device_times() -> dict:
    """Segments of the last device finish on this thread (mtg_last_finish_device_times)."""
    out = (C.c_double * 6)()
    _lib.load().mtg_last_finish_device_times(out)
    return {"insert_eulerise_s": out[0], "host_graph_s": out[1], "euler_s": out[2], "cut_s": out[3], "euler_kernel_ms": out[4],
            "breaking_biedges": int(out[5])}


def last_finish_device_stage_ms() -> dict:
    """GPU ms per stage of the last device finish (mtg_last_finish_device_stage_ms) + its dart and unit counts."""
    out = (C.c_double * 6)()
    _lib.load().mtg_last_finish_device_stage_ms(out)
    return {"insert_eulerise_ms": out[0], "records_ms": out[1], "decomposition_ms": out[2], "cut_ms": out[3], "darts": int(out[4]),
            "units": int(out[5])}


def last_performance_data() -> dict:
    """greedytigs/mod.rs:647-673 counters of the last greedy run with PerformanceDataType.Complete."""
    out = _lib.MtgDijkstraPerformanceData()
    _lib.load().mtg_last_performance_data(C.byref(out))
    return out.as_dict()


class UnitigStore:
    """Sequence store filled by read_bcalm2 / read_fasta (replaces DefaultSequenceStore<DnaAlphabet>, bin.rs:871)."""

    def __init__(self, handle: int):
        self._h = handle
        self._L = _lib.load()

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._L.mtg_unitigs_free(h)

    @property
    def handle(self) -> int:
        return self._h

    def __len__(self) -> int:
        return int(self._L.mtg_unitigs_count(self._h))

    def arrays(self):
        """(uint8 data, uint64 offsets) as views of the store's memory: valid while the store lives."""
        n = len(self)
        off = np.ctypeslib.as_array(C.cast(self._L.mtg_unitigs_offsets(self._h), C.POINTER(C.c_uint64)), shape=(n + 1,))
        total = int(off[n])
        if total == 0:
            return np.zeros(0, np.uint8), off
        return np.ctypeslib.as_array(C.cast(self._L.mtg_unitigs_data(self._h), C.POINTER(C.c_uint8)), shape=(total,)), off

    def sequences(self) -> list[str]:
        n = len(self)
        off = np.ctypeslib.as_array(C.cast(self._L.mtg_unitigs_offsets(self._h), C.POINTER(C.c_uint64)), shape=(n + 1,))
        data = C.string_at(self._L.mtg_unitigs_data(self._h), int(off[n])).decode()
        return [data[int(off[i]):int(off[i + 1])] for i in range(n)]


def read_bcalm2(path: str, k: int):
    """`--bcalm-in path -k k` (bin.rs:902-912): BCALM2/GGCAT unitig FASTA (optionally .gz) -> (Bigraph, UnitigStore)."""
    L = _lib.load()
    st = C.c_void_p()
    g = L.mtg_read_bcalm2(str(path).encode(), k, C.byref(st))
    return Bigraph(g), UnitigStore(st.value)


def read_fasta(path: str, k: int, device_id: int = 0):
    """`--fa-in path -k k` (bin.rs:71-75, 891-901): plain unitig FASTA (optionally .gz) -> (Bigraph, UnitigStore). The graph
    comes from the (k-1)-mer overlaps of the unitig ends, joined on GPU `device_id`."""
    L = _lib.load()
    st = C.c_void_p()
    g = L.mtg_read_fasta(str(path).encode(), k, device_id, C.byref(st))
    return Bigraph(g), UnitigStore(st.value)


def last_fasta_in_times() -> dict:
    """Phases of the last read_fasta / Bigraph.from_sequences on this thread (ms; bytes = what the join kernels must move)."""
    out = (C.c_double * 6)()
    _lib.load().mtg_last_fasta_in_times(out)
    return dict(zip(("parse_ms", "upload_ms", "kernel_ms", "download_ms", "build_ms", "bytes"), list(out)))


def read_sequences(path: str, split_non_acgt: bool = False) -> UnitigStore:
    """Any FASTA file (optionally .gz, multi-line records, either case) as a sequence store: no graph, no length rule, no GPU.
    split_non_acgt: a run of characters outside ACGT (the `N` of real assemblies) ends a piece instead of aborting; every maximal
    ACGT stretch becomes a record, empty pieces are dropped, and the store's `pieces_cut` holds the number of runs met."""
    st = C.c_void_p()
    if split_non_acgt:
        cut = C.c_uint64()
        _lib.load().mtg_read_sequences_split(str(path).encode(), C.byref(st), C.byref(cut))
        store = UnitigStore(st.value)
        store.pieces_cut = int(cut.value)
        return store
    _lib.load().mtg_read_sequences(str(path).encode(), C.byref(st))
    return UnitigStore(st.value)


@dataclass(frozen=True)
class Compaction:
    """mtg_compaction (include/mtg_engine.h): the counts of one unitig compaction, in exact integers.
    distinct_kmers == unitig_characters - (k - 1) * unitigs."""

    records: int
    characters: int
    windows: int
    distinct_kmers: int
    unitigs: int
    unitig_characters: int
    closed_walks: int
    longest_unitig_kmers: int

    def describe(self) -> str:
        return (f"{self.records} records, {self.characters} characters, {self.windows} windows -> {self.distinct_kmers} distinct k-mers "
                f"in {self.unitigs} unitigs of {self.unitig_characters} characters ({self.closed_walks} closed, longest "
                f"{self.longest_unitig_kmers} k-mers)")


def compact_unitigs(seqs_or_store, k: int, device_id: int = 0):
    """The maximal unitigs of the k-mer set of arbitrary sequences, compacted on GPU `device_id` (mtg_compact_unitigs)
    -> (UnitigStore, Compaction). seqs_or_store: UnitigStore, list of str, or (uint8 array, offsets). The store is an ordinary one:
    Bigraph.from_sequences((data, offsets) of it), the writers and compare_kmer_sets take it."""
    return _compact(_PLAIN, seqs_or_store, k, device_id)[:2]


@dataclass(frozen=True, eq=False)
class Abundance:
    """mtg_abundance plus the per-unitig sums (include/mtg_engine.h): what a counted compaction counted, in exact
    integers. spectrum[c] = distinct k-mers of the input with abundance c (the last bin: 255 or more), taken before the filter;
    unitig_sums[u] = the sum of abundance over the k-mers of record u of the store; their total is kept_occurrences. kmer_counts
    (compact_unitigs_counted(..., kmer_counts=True); else None): the abundance of every kept k-mer in window order of
    the store -- the k-mers of record 0 from left to right, then those of record 1, ... --, the `weights` a KmerIndex of the store takes."""

    distinct_all: int
    distinct_kept: int
    max_abundance: int
    kept_occurrences: int
    spectrum: np.ndarray     # uint64[256]
    unitig_sums: np.ndarray  # uint64[unitigs]
    kmer_counts: Optional[np.ndarray] = None  # uint32[distinct_kept]

    @property
    def dropped(self) -> int:
        return self.distinct_all - self.distinct_kept

    def describe(self) -> str:
        return (f"{self.distinct_all} distinct k-mers -> {self.distinct_kept} kept, {self.dropped} dropped; "
                f"max abundance {self.max_abundance}")


def compact_unitigs_counted(seqs_or_store, k: int, min_abundance: int, device_id: int = 0, kmer_counts: bool = False):
    """compact_unitigs over the k-mers whose abundance -- the windows that show them, on either strand -- is at least min_abundance
    (mtg_compact_unitigs_counted) -> (UnitigStore, Compaction, Abundance). Creators and readings are taken over all
    windows; with min_abundance = 1 store and Compaction equal compact_unitigs'. Compaction.distinct_kmers counts the kept k-mers.
    kmer_counts=True (mtg_compact_unitigs_counted_kmers): Abundance.kmer_counts also holds every kept k-mer's abundance."""
    if min_abundance < 1:
        raise ValueError("min_abundance must be >= 1")
    return _compact(_COUNTED_KMERS if kmer_counts else _COUNTED, seqs_or_store, k, device_id, min_abundance)[:3]


MAX_COLORS = 64


@dataclass(frozen=True, eq=False)
class Colors:
    """What a coloured compaction knows about the inputs of every kept k-mer (mtg_compact_unitigs_colored), in exact
    integers. kmer_colors[i] = the mask of k-mer i in window order of the store (the indexing of Abundance.kmer_counts): bit c is set
    iff a window of a record of colour c shows the k-mer, on either strand. per_color[c] = the kept k-mers with bit c; shared[i, j] =
    those with bits i and j (symmetric, the diagonal is per_color); occupancy[j] = those carried by exactly j colours."""

    n_colors: int
    kmer_colors: np.ndarray  # uint64[distinct_kept]
    per_color: np.ndarray    # uint64[n_colors]
    occupancy: np.ndarray    # uint64[65]
    shared: np.ndarray       # uint64[n_colors, n_colors]

    @property
    def core(self) -> int:
        """The kept k-mers every colour carries."""
        return int(self.occupancy[self.n_colors])

    @property
    def private(self) -> int:
        """The kept k-mers exactly one colour carries."""
        return int(self.occupancy[1])

    def jaccard(self) -> np.ndarray:
        """|i and j| / |i or j| over the kept k-mers as float64[n_colors, n_colors]; nan where both colours are empty."""
        inter = self.shared.astype(np.float64)
        union = self.per_color[:, None].astype(np.float64) + self.per_color[None, :].astype(np.float64) - inter
        out = np.full(inter.shape, np.nan)
        np.divide(inter, union, out=out, where=union > 0)
        return out

    def describe(self) -> str:
        return (f"{self.n_colors} colours over {int(self.occupancy.sum())} k-mers: {self.core} core, {self.private} private")


def _record_count(seqs_or_store) -> int:
    """The records of a UnitigStore, a list of str or (uint8 array, offsets)."""
    return len(seqs_or_store[1]) - 1 if isinstance(seqs_or_store, tuple) else len(seqs_or_store)


def _record_colors(record_colors, n_colors, n_records: int) -> np.ndarray:
    """The colours of a coloured call as uint8[n_records]; ValueError for what the library would abort on."""
    if isinstance(n_colors, bool) or not isinstance(n_colors, (int, np.integer)) or not 1 <= n_colors <= MAX_COLORS:
        raise ValueError(f"n_colors must be in 1..{MAX_COLORS}, not {n_colors!r}")
    wide = np.asarray(record_colors)
    if wide.ndim != 1 or len(wide) != n_records:
        raise ValueError(f"record_colors must hold one entry per record: {wide.shape} for {n_records} records")
    if len(wide) and (wide.dtype.kind not in "iu" or int(wide.min()) < 0 or int(wide.max()) >= n_colors):
        raise ValueError(f"every colour must be an integer in 0..{n_colors - 1}")
    return np.ascontiguousarray(wide, np.uint8)


def compact_unitigs_colored(seqs_or_store, k: int, record_colors, n_colors: int, min_abundance: int = 1, device_id: int = 0):
    """compact_unitigs_counted(..., kmer_counts=True) -- the same store, Compaction and Abundance -- that also tells which inputs carry
    every kept k-mer (mtg_compact_unitigs_colored) -> (UnitigStore, Compaction, Abundance, Colors). record_colors: one
    integer in 0..n_colors - 1 per input record (its file, sample or haplotype), n_colors in 1..64."""
    if min_abundance < 1:
        raise ValueError("min_abundance must be >= 1")
    rc = _record_colors(record_colors, n_colors, _record_count(seqs_or_store))
    return _compact(_COLORED, seqs_or_store, k, device_id, min_abundance, rc, int(n_colors))[:4]


# the counts kernel of the class dictionary (compact_device.hip): the classes it keeps in LDS, its largest grid, its block
COLOR_CLASS_LDS = 2048
COLOR_CLASS_GRID = 512
COLOR_CLASS_BLOCK = 256


@dataclass(frozen=True, eq=False)
class ColorClasses:
    """The dictionary of a coloured store's masks (mtg_compact_unitigs_colored_classes), in exact integers. The classes
    are the distinct masks, numbered in the order of the first window of the store that shows them; a run is a maximal stretch of
    consecutive windows of one unitig with equal masks. masks[c], kmers[c] = the windows of class c, runs[c] = its runs, first[c] =
    the first window that shows it (strictly increasing); kmer_class[i] = the class of window i: masks[kmer_class] == kmer_colors."""

    masks: np.ndarray       # uint64[classes]
    kmers: np.ndarray       # uint64[classes]
    runs: np.ndarray        # uint64[classes]
    first: np.ndarray       # uint64[classes]
    kmer_class: np.ndarray  # uint32[distinct_kept]

    def unitig_classes(self, unitig_kmers) -> np.ndarray:
        """The class of each unitig's first k-mer as uint32[unitigs] (unitig_kmers: the k-mers of every unitig in the store's order)
        -- on a split store the class of the whole unitig."""
        n = np.asarray(unitig_kmers, np.int64)
        if n.ndim != 1 or int(n.sum()) != len(self.kmer_class) or (len(n) and int(n.min()) < 1):
            raise ValueError(f"unitig_kmers must hold the k-mers of every unitig: they sum to {int(n.sum())}, the store has {len(self.kmer_class)}")
        return self.kmer_class[np.cumsum(n) - n]

    def describe(self) -> str:
        if not len(self.masks):
            return "0 classes in 0 runs"
        top = int(np.argmax(self.kmers))  # (ties: the first class)
        return (f"{len(self.masks)} classes in {int(self.runs.sum())} runs, the largest class {top} (mask {int(self.masks[top]):x}, "
                f"{bin(int(self.masks[top])).count('1')} carriers) with {int(self.kmers[top])} of {int(self.kmers.sum())} k-mers")


def _taken(n, pointer, dtype) -> np.ndarray:
    """A copy of the n entries of a vector behind one of the library's handles."""
    ctype = np.ctypeslib.as_ctypes_type(dtype)
    return np.ctypeslib.as_array(C.cast(pointer, C.POINTER(ctype)), shape=(int(n),)).copy() if n else np.zeros(0, dtype)


def _color_classes_taken(L, classes) -> ColorClasses:
    """The arrays of an mtg_color_classes handle, copied."""
    nc = L.mtg_color_classes_count(classes)
    return ColorClasses(*(_taken(nc, f(classes), np.uint64) for f in (L.mtg_color_classes_masks, L.mtg_color_classes_kmers,
                                                                        L.mtg_color_classes_runs, L.mtg_color_classes_first)),
                        _taken(L.mtg_color_classes_kmer_class_count(classes), L.mtg_color_classes_kmer_class(classes), np.uint32))


def color_classes(kmer_colors, unitig_kmers, device_id: int = 0) -> ColorClasses:
    """The colour classes of masks handed in (mtg_color_classes_build): kmer_colors, one non-zero mask per k-mer in window
    order of a store (Colors.kmer_colors), and unitig_kmers, the k-mers of every unitig of that store."""
    masks = np.ascontiguousarray(kmer_colors, np.uint64)
    n = np.asarray(unitig_kmers)
    if masks.ndim != 1 or n.ndim != 1 or (len(n) and (n.dtype.kind not in "iu" or int(n.min()) < 1)) or int(n.sum()) != len(masks):
        raise ValueError("unitig_kmers must hold the k-mers (>= 1) of every unitig and sum to len(kmer_colors)")
    if len(masks) and not masks.all():
        raise ValueError("a kept k-mer's mask is never 0")
    n = np.ascontiguousarray(n, np.uint64)
    L = _lib.load()
    classes = C.c_void_p()
    L.mtg_color_classes_build(_ptr(masks), len(masks), _ptr(n), len(n), device_id, C.byref(classes))
    try:
        return _color_classes_taken(L, classes)
    finally:
        L.mtg_color_classes_free(classes)


def compact_unitigs_colored_classes(seqs_or_store, k: int, record_colors, n_colors: int, min_abundance: int = 1, split: bool = False,
                                    device_id: int = 0):
    """compact_unitigs_colored plus the colour classes of the output store (mtg_compact_unitigs_colored_classes) ->
    (UnitigStore, Compaction, Abundance, Colors, ColorClasses). split=False: the first four are compact_unitigs_colored's. split=True:
    the unitigs are cut wherever the colour set changes, so that each is monochromatic -- one run, one class --, and store, Compaction,
    unitig_sums, kmer_counts and kmer_colors describe the split store."""
    if min_abundance < 1:
        raise ValueError("min_abundance must be >= 1")
    if not isinstance(split, (bool, np.bool_)):
        raise ValueError(f"split must be True or False, not {split!r}")
    rc = _record_colors(record_colors, n_colors, _record_count(seqs_or_store))
    return _compact(_CLASSES, seqs_or_store, k, device_id, min_abundance, rc, int(n_colors), split)[:5]


@dataclass(frozen=True)
class Cleaning:
    """mtg_cleaning (include/mtg_engine.h): what the rounds of a cleaned compaction removed, in exact integers. A tip is
    an open unitig of fewer than clip_tips k-mers with one free end and one end that shares its side of a fork; an isolated unitig
    has fewer than remove_isolated k-mers and two free ends. rounds_run counts the round that removed nothing too."""

    rounds_run: int
    tips: int
    tip_kmers: int
    isolated: int
    isolated_kmers: int
    removed_occurrences: int

    @property
    def removed_kmers(self) -> int:
        return self.tip_kmers + self.isolated_kmers

    def describe(self) -> str:
        return (f"{self.tips} tips of {self.tip_kmers} k-mers and {self.isolated} isolated unitigs of {self.isolated_kmers} k-mers "
                f"removed in {self.rounds_run} rounds")


MAX_CLEAN_ROUNDS = 64


def compact_unitigs_cleaned(seqs_or_store, k: int, clip_tips: int = 0, remove_isolated: int = 0, rounds: int = 1, min_abundance: int = 1,
                            record_colors=None, n_colors: int = 0, split: bool = False, kmer_counts: bool = False, device_id: int = 0):
    """The counted, coloured or classed compaction with tips clipped and isolated unitigs dropped before the final pass
    (mtg_compact_unitigs_cleaned) -> (UnitigStore, Compaction, Abundance, Colors | None, ColorClasses | None, Cleaning).
    clip_tips = L removes the open unitigs of fewer than L k-mers that dead-end on one side and share their side of a fork on the other
    (0: off; the conventional value is k); remove_isolated = L those with two dead ends; at most `rounds` rounds, each on the unitigs
    the one before left. record_colors / n_colors as for compact_unitigs_colored_classes (None: no colours, the fourth and fifth
    entries are None); split needs colours and is decided on the unsplit unitigs. Compaction, unitig_sums, kmer_counts, kmer_colors
    and the classes describe the final store; Abundance's scalars keep their meaning (distinct_kept = the k-mers that reach
    min_abundance), so unitig_sums.sum() == kept_occurrences - Cleaning.removed_occurrences. With both lengths 0 the result is the
    uncleaned call's."""
    for name, v, lo, hi in (("clip_tips", clip_tips, 0, 2 ** 64 - 1), ("remove_isolated", remove_isolated, 0, 2 ** 64 - 1),
                            ("rounds", rounds, 1, MAX_CLEAN_ROUNDS)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError(f"{name} must be an integer in {lo}..{hi}, not {v!r}")
    if min_abundance < 1:
        raise ValueError("min_abundance must be >= 1")
    if not isinstance(split, (bool, np.bool_)):
        raise ValueError(f"split must be True or False, not {split!r}")
    if record_colors is None:
        if split:
            raise ValueError("split needs record_colors")
        return _compact(_COUNTED_KMERS if kmer_counts else _COUNTED, seqs_or_store, k, device_id, min_abundance,
                        cleaning=(int(clip_tips), int(remove_isolated), int(rounds)))[:6]
    rc = _record_colors(record_colors, n_colors, _record_count(seqs_or_store))
    return _compact(_CLASSES, seqs_or_store, k, device_id, min_abundance, rc, int(n_colors), split,
                    cleaning=(int(clip_tips), int(remove_isolated), int(rounds)))[:6]


def last_clean_times() -> dict:
    """Of the last compaction on this thread: the ms of the decision and removal kernels over all rounds (HIP events) and the rounds
    run. last_compact_times' nodes_ms and rank_ms include every round's."""
    out = (C.c_double * 2)()
    _lib.load().mtg_last_clean_times(out)
    return {"clean_ms": float(out[0]), "rounds_run": int(out[1])}


@dataclass(frozen=True)
class Bubbles:
    """mtg_bubbles (include/mtg_engine.h): what the rounds of a simplified compaction popped, in exact integers. An arm
    is an open unitig of fewer than pop_bubbles k-mers between two nodes that another such unitig joins too; of the arms between
    one pair of nodes the one with the largest mean abundance stays (ties: the earliest creator at an end), and another goes iff
    the best has at least bubble_ratio times its mean abundance."""

    arms: int
    arm_kmers: int
    removed_occurrences: int

    def describe(self) -> str:
        return f"{self.arms} bubble arms of {self.arm_kmers} k-mers popped"


MAX_BUBBLE_RATIO = 255


def compact_unitigs_simplified(seqs_or_store, k: int, pop_bubbles: int = 0, bubble_ratio: int = 1, clip_tips: int = 0, remove_isolated: int = 0,
                               rounds: int = 1, min_abundance: int = 1, record_colors=None, n_colors: int = 0, split: bool = False,
                               kmer_counts: bool = False, device_id: int = 0):
    """compact_unitigs_cleaned whose rounds also pop the weaker arms of simple bubbles (mtg_compact_unitigs_simplified) ->
    (UnitigStore, Compaction, Abundance, Colors | None, ColorClasses | None, Cleaning, Bubbles). pop_bubbles = L looks at the open
    unitigs of fewer than L k-mers (0: off; a SNP's arms have k k-mers, so k + 1 is the least L that pops them and 2 k the usual
    value); bubble_ratio = R pops an arm only if the best arm between the same two nodes has at least R times its mean abundance
    (1: every arm but the best goes). Tips, isolated unitigs and arms of a round are decided on one snapshot and leave together.
    Everything describes the final store: unitig_sums.sum() == kept_occurrences - Cleaning.removed_occurrences -
    Bubbles.removed_occurrences. With pop_bubbles = 0 the first six entries are compact_unitigs_cleaned's."""
    for name, v, lo, hi in (("pop_bubbles", pop_bubbles, 0, 2 ** 64 - 1), ("bubble_ratio", bubble_ratio, 1, MAX_BUBBLE_RATIO),
                            ("clip_tips", clip_tips, 0, 2 ** 64 - 1), ("remove_isolated", remove_isolated, 0, 2 ** 64 - 1),
                            ("rounds", rounds, 1, MAX_CLEAN_ROUNDS)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError(f"{name} must be an integer in {lo}..{hi}, not {v!r}")
    if min_abundance < 1:
        raise ValueError("min_abundance must be >= 1")
    if not isinstance(split, (bool, np.bool_)):
        raise ValueError(f"split must be True or False, not {split!r}")
    cleaning, bubbles = (int(clip_tips), int(remove_isolated), int(rounds)), (int(pop_bubbles), int(bubble_ratio))
    if record_colors is None:
        if split:
            raise ValueError("split needs record_colors")
        return _compact(_COUNTED_KMERS if kmer_counts else _COUNTED, seqs_or_store, k, device_id, min_abundance, cleaning=cleaning, bubbles=bubbles)
    rc = _record_colors(record_colors, n_colors, _record_count(seqs_or_store))
    return _compact(_CLASSES, seqs_or_store, k, device_id, min_abundance, rc, int(n_colors), split, cleaning=cleaning, bubbles=bubbles)


def last_bubble_times() -> dict:
    """Of the last compaction on this thread: the ms of the bubble kernels (list, sums, choose, verdict) over all rounds, by HIP
    events; 0.0 where nothing was to be popped. last_clean_times leaves them out."""
    out = (C.c_double * 1)()
    _lib.load().mtg_last_bubble_times(out)
    return {"bubble_ms": float(out[0])}


def _color_mask(colors, name: str) -> int:
    """A colour mask given as an int or as an iterable of colour numbers."""
    if isinstance(colors, bool):
        raise ValueError(f"{name} must be a mask or an iterable of colour numbers, not {colors!r}")
    if isinstance(colors, (int, np.integer)):
        mask = int(colors)
        if not 0 <= mask < 2 ** MAX_COLORS:
            raise ValueError(f"{name} must be a mask of {MAX_COLORS} bits, not {colors!r}")
        return mask
    mask = 0
    for c in colors:
        if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 0 <= c < MAX_COLORS:
            raise ValueError(f"{name} holds colour numbers in 0..{MAX_COLORS - 1}, not {c!r}")
        mask |= 1 << int(c)
    return mask


_NOT_ACGT = re.compile("[^ACGTacgt]+")


class KmerSelection:
    """Which k-mers of S_m (those that reach min_abundance) a selected compaction keeps (mtg_selection_params and the filter records of
    mtg_compact_unitigs_selected). A k-mer is selected iff, in this order: none of its colours is in `forbid`; all of
    `require` are among them; min_colors <= its carriers <= max_colors; it occurs fewer than subtract_min_abundance times in the
    windows of `subtract`; it occurs at least intersect_min_abundance times in the windows of `intersect`. require / forbid: a mask
    or an iterable of colour numbers. subtract / intersect: None, a list of str (either case; whatever is outside ACGT ends a piece,
    as in the `--seq-in` readers), a UnitigStore or (uint8 array, offsets) of ACGT records; a rule applies only if its set has a record.
    The filter sets are looked up, never inserted: they create, count and colour nothing. The defaults select everything.
    filter_records: further filter records as (role, str) pairs, role "subtract" or "intersect", stored in the order given behind the
    two sets (the sets' members are stored set by set; what is selected does not depend on the order)."""

    def __init__(self, require=0, forbid=0, min_colors: int = 0, max_colors: int = MAX_COLORS, subtract=None, subtract_min_abundance: int = 1,
                 intersect=None, intersect_min_abundance: int = 1, filter_records=None):
        self.require, self.forbid = _color_mask(require, "require"), _color_mask(forbid, "forbid")
        for name, v, lo, hi in (("min_colors", min_colors, 0, MAX_COLORS), ("max_colors", max_colors, 0, MAX_COLORS),
                                ("subtract_min_abundance", subtract_min_abundance, 1, 2 ** 64 - 1),
                                ("intersect_min_abundance", intersect_min_abundance, 1, 2 ** 64 - 1)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
                raise ValueError(f"{name} must be an integer in {lo}..{hi}, not {v!r}")
        if self.require & self.forbid:
            raise ValueError(f"require and forbid share colour {(self.require & self.forbid).bit_length() - 1}")
        if min_colors > max_colors:
            raise ValueError(f"min_colors {min_colors} exceeds max_colors {max_colors}")
        self.min_colors, self.max_colors = int(min_colors), int(max_colors)
        self.subtract_min_abundance, self.intersect_min_abundance = int(subtract_min_abundance), int(intersect_min_abundance)
        self.subtract, self.intersect = subtract, intersect
        self.filter_records = list(filter_records) if filter_records is not None else []
        if any(role not in ("subtract", "intersect") or not isinstance(seq, str) for role, seq in self.filter_records):
            raise ValueError('filter_records holds (role, str) pairs with the role "subtract" or "intersect"')

    @property
    def colour_rule(self) -> bool:
        return bool(self.require or self.forbid or self.min_colors > 0 or self.max_colors < MAX_COLORS)

    def _params(self, n_colors: int):
        """The fields of mtg_selection_params; ValueError for a colour the call does not have."""
        if self.colour_rule and not n_colors:
            raise ValueError("require, forbid, min_colors and max_colors need record_colors")
        for name, mask in (("require", self.require), ("forbid", self.forbid)):
            if n_colors and mask >> n_colors:
                raise ValueError(f"{name} names colour {mask.bit_length() - 1} of {n_colors}")
        return (self.require, self.forbid, self.min_colors, self.max_colors, self.subtract_min_abundance, self.intersect_min_abundance)

    @staticmethod
    def _records(x):
        """-> (uint8 data, offsets as a list) of one filter set."""
        if x is None:
            return np.zeros(0, np.uint8), [0]
        if isinstance(x, UnitigStore):
            data, off = x.arrays()
            return np.array(data, np.uint8), [int(o) for o in off]
        if isinstance(x, tuple):
            return np.ascontiguousarray(x[0], np.uint8), [int(o) for o in x[1]]
        pieces = [p for s in x for p in _NOT_ACGT.split(s) if p]
        return np.frombuffer("".join(pieces).encode(), np.uint8), [0] + list(np.cumsum([len(p) for p in pieces], dtype=np.int64))

    def _filter_arrays(self):
        """The filter store of the call: data, offsets, one role byte per record (0 subtract, 1 intersect)."""
        (ds, os_), (di, oi) = self._records(self.subtract), self._records(self.intersect)
        off = os_ + [os_[-1] + o for o in oi[1:]]
        roles = [0] * (len(os_) - 1) + [1] * (len(oi) - 1)
        more = [(role == "intersect", p) for role, seq in self.filter_records for p in _NOT_ACGT.split(seq) if p]
        for role, p in more:
            off.append(off[-1] + len(p))
            roles.append(int(role))
        dm = np.frombuffer("".join(p for _, p in more).encode(), np.uint8)
        return np.ascontiguousarray(np.concatenate([ds, di, dm]), np.uint8), np.array(off, np.uint64), np.array(roles, np.uint8)


@dataclass(frozen=True, eq=False)
class Selection:
    """mtg_selection (include/mtg_engine.h): what a selected compaction selected, in exact integers. input_kmers = the
    k-mers that reach min_abundance; a rejected k-mer is counted under the first rule it fails, so the five counts and `selected` add
    up to input_kmers; *_windows: the windows of the filter records, *_hits: those whose k-mer is in the input at all;
    per_color_selected[c]: the selected k-mers colour c carries (empty in a call without colours)."""

    input_kmers: int
    rejected_forbid: int
    rejected_require: int
    rejected_carriers: int
    rejected_subtract: int
    rejected_intersect: int
    selected: int
    selected_occurrences: int
    subtract_windows: int
    intersect_windows: int
    subtract_hits: int
    intersect_hits: int
    per_color_selected: np.ndarray  # uint64[n_colors]

    @property
    def rejected(self) -> int:
        return self.input_kmers - self.selected

    def describe(self) -> str:
        rules = [f"{n} by {name}" for name, n in (("forbid", self.rejected_forbid), ("require", self.rejected_require),
                                                  ("carriers", self.rejected_carriers), ("subtract", self.rejected_subtract),
                                                  ("intersect", self.rejected_intersect)) if n]
        return f"{self.selected} of {self.input_kmers} k-mers selected" + (", rejected " + ", ".join(rules) if rules else "")


def compact_unitigs_selected(seqs_or_store, k: int, selection: KmerSelection, pop_bubbles: int = 0, bubble_ratio: int = 1, clip_tips: int = 0,
                             remove_isolated: int = 0, rounds: int = 1, min_abundance: int = 1, record_colors=None, n_colors: int = 0,
                             split: bool = False, kmer_counts: bool = False, device_id: int = 0):
    """compact_unitigs_simplified over the k-mers a KmerSelection keeps (mtg_compact_unitigs_selected) -> (UnitigStore,
    Compaction, Abundance, Colors | None, ColorClasses | None, Cleaning, Bubbles, Selection). The selection acts where min_abundance
    does, in front of the unitigs: store, Compaction, unitig_sums, kmer_counts, kmer_colors and the classes describe the selected (and
    then cleaned) set; Abundance's scalars keep their meaning, and Colors' per_color, shared and occupancy are taken over the k-mers
    that reach min_abundance, before the selection: they are how a carrier threshold is chosen. With KmerSelection() the store and
    the per-k-mer arrays are compact_unitigs_simplified's. Nothing selected is a result: an empty store, the statistics filled."""
    if not isinstance(selection, KmerSelection):
        raise ValueError(f"selection must be a KmerSelection, not {selection!r}")
    for name, v, lo, hi in (("pop_bubbles", pop_bubbles, 0, 2 ** 64 - 1), ("bubble_ratio", bubble_ratio, 1, MAX_BUBBLE_RATIO),
                            ("clip_tips", clip_tips, 0, 2 ** 64 - 1), ("remove_isolated", remove_isolated, 0, 2 ** 64 - 1),
                            ("rounds", rounds, 1, MAX_CLEAN_ROUNDS)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError(f"{name} must be an integer in {lo}..{hi}, not {v!r}")
    if min_abundance < 1:
        raise ValueError("min_abundance must be >= 1")
    if not isinstance(split, (bool, np.bool_)):
        raise ValueError(f"split must be True or False, not {split!r}")
    cleaning, bubbles = (int(clip_tips), int(remove_isolated), int(rounds)), (int(pop_bubbles), int(bubble_ratio))
    if record_colors is None:
        if split:
            raise ValueError("split needs record_colors")
        selection._params(0)
        return _compact(_COUNTED_KMERS if kmer_counts else _COUNTED, seqs_or_store, k, device_id, min_abundance, cleaning=cleaning, bubbles=bubbles,
                        selection=selection)
    rc = _record_colors(record_colors, n_colors, _record_count(seqs_or_store))
    selection._params(int(n_colors))
    return _compact(_CLASSES, seqs_or_store, k, device_id, min_abundance, rc, int(n_colors), split, cleaning=cleaning, bubbles=bubbles, selection=selection)


# The rungs of the compaction ladder and the C symbol each reaches (+ "_store" for a UnitigStore). The argument list of a rung is
# the one below it plus its own (_compact): a new rung is one row here and one `if` there.
_PLAIN, _COUNTED, _COUNTED_KMERS, _COLORED, _CLASSES = range(5)
_COMPACT_SYMBOLS = ("mtg_compact_unitigs", "mtg_compact_unitigs_counted", "mtg_compact_unitigs_counted_kmers", "mtg_compact_unitigs_colored",
                    "mtg_compact_unitigs_colored_classes")


def _compact(rung: int, seqs_or_store, k: int, device_id: int, min_abundance: int = 1, record_colors=None, n_colors: int = 0,
             split: bool = False, cleaning=None, bubbles=None, selection=None):
    """The one body of compact_unitigs* -> (UnitigStore, Compaction, Abundance, Colors, ColorClasses, Cleaning, Bubbles), None above the
    rung. cleaning: None, or (clip_tips, remove_isolated, rounds) -- the call then goes through mtg_compact_unitigs_cleaned, which takes
    the arguments of every rung and null out-pointers above the one asked for; bubbles: None, or (pop_bubbles, bubble_ratio) beside
    a cleaning -- then through mtg_compact_unitigs_simplified; selection: None, or a KmerSelection beside both -- then through
    mtg_compact_unitigs_selected, and the tuple ends with the Selection. The arguments are the callers' to check."""
    L = _lib.load()
    out, sums, counts, masks, classes = (C.c_void_p() for _ in range(5))
    stats, ab, cs = _lib.MtgCompaction(), _lib.MtgAbundance(), _lib.MtgColorStats()
    if cleaning is None:
        symbol = _COMPACT_SYMBOLS[rung]
        ins, outs = [k], [C.byref(out), C.byref(stats)]
        if rung >= _COUNTED:
            ins += [min_abundance]
            outs += [C.byref(ab), C.byref(sums)]
        if rung >= _COUNTED_KMERS:
            outs += [C.byref(counts)]
        if rung >= _COLORED:
            ins += [_ptr(record_colors), n_colors]
            outs += [C.byref(masks), C.byref(cs)]
        if rung >= _CLASSES:
            ins += [int(bool(split))]
            outs += [C.byref(classes)]
        ins += [device_id]
    else:
        symbol = "mtg_compact_unitigs_cleaned" if bubbles is None else "mtg_compact_unitigs_simplified" if selection is None else "mtg_compact_unitigs_selected"
        params, cleaned = _lib.MtgCleaningParams(*cleaning), _lib.MtgCleaning()
        ins = [k, min_abundance, _ptr(record_colors) if rung >= _COLORED else None, n_colors, int(bool(split)), C.byref(params)]
        if bubbles is not None:
            bubble_params, popped = _lib.MtgBubbleParams(*bubbles), _lib.MtgBubbles()
            ins += [C.byref(bubble_params)]
        if selection is not None:
            sel_params, chosen = _lib.MtgSelectionParams(*selection._params(n_colors if rung >= _COLORED else 0)), _lib.MtgSelection()
            f_data, f_off, f_roles = selection._filter_arrays()
            ins += [C.byref(sel_params), _ptr(f_data) if len(f_data) else None, _ptr(f_off), _ptr(f_roles) if len(f_roles) else None, len(f_roles)]
        ins += [device_id]
        outs = [C.byref(out), C.byref(stats), C.byref(ab), C.byref(sums), C.byref(counts) if rung >= _COUNTED_KMERS else None,
                C.byref(masks) if rung >= _COLORED else None, C.byref(cs) if rung >= _COLORED else None,
                C.byref(classes) if rung >= _CLASSES else None, C.byref(cleaned)]
        if bubbles is not None:
            outs += [C.byref(popped)]
        if selection is not None:
            outs += [C.byref(chosen)]
    if isinstance(seqs_or_store, UnitigStore):
        getattr(L, symbol + "_store")(seqs_or_store.handle, *ins, *outs)
    else:
        d, o, n, keep = _sequence_arrays(seqs_or_store)
        getattr(L, symbol)(d, o, n, *ins, *outs)
        del keep
    abundance = colors = cc = None
    try:  # (a handle the rung does not reach is still null: nothing to take, and freeing it is a no-op)
        if rung >= _COUNTED:
            per_kmer = _taken(L.mtg_kmer_counts_count(counts), L.mtg_kmer_counts_array(counts), np.uint32) if rung >= _COUNTED_KMERS else None
            abundance = Abundance(int(ab.distinct_all), int(ab.distinct_kept), int(ab.max_abundance), int(ab.kept_occurrences),
                                  np.array(ab.spectrum, dtype=np.uint64),
                                  _taken(L.mtg_abundance_sums_count(sums), L.mtg_abundance_sums_array(sums), np.uint64), per_kmer)
        if rung >= _COLORED:
            colors = Colors(n_colors, _taken(L.mtg_kmer_colors_count(masks), L.mtg_kmer_colors_array(masks), np.uint64),
                            np.array(cs.per_color, dtype=np.uint64)[:n_colors].copy(), np.array(cs.occupancy, dtype=np.uint64),
                            np.array(cs.shared, dtype=np.uint64).reshape(MAX_COLORS, MAX_COLORS)[:n_colors, :n_colors].copy())
        if rung >= _CLASSES:
            cc = _color_classes_taken(L, classes)
    finally:
        L.mtg_abundance_sums_free(sums)
        L.mtg_kmer_counts_free(counts)
        L.mtg_kmer_colors_free(masks)
        L.mtg_color_classes_free(classes)
    result = (UnitigStore(out.value), Compaction(**stats.as_dict()), abundance, colors, cc,
              Cleaning(**cleaned.as_dict()) if cleaning is not None else None, Bubbles(**popped.as_dict()) if bubbles is not None else None)
    if selection is None:
        return result
    scalars = {name: int(getattr(chosen, name)) for name, _ in chosen._fields_ if name != "per_color_selected"}
    per_color = np.array(chosen.per_color_selected, dtype=np.uint64)[:n_colors if rung >= _COLORED else 0].copy()
    return result + (Selection(per_color_selected=per_color, **scalars),)


def last_color_class_times() -> dict:
    """In ms, the class dictionary of the last compact_unitigs_colored_classes on this thread: run heads, class table, class ids,
    counts (HIP events around the kernels), download (host clock)."""
    out = (C.c_double * 5)()
    _lib.load().mtg_last_color_class_times(out)
    return dict(zip(("heads_ms", "table_ms", "ids_ms", "counts_ms", "download_ms"), map(float, out)))


def color_class_limits() -> dict:
    """The library's own values of COLOR_CLASS_LDS, COLOR_CLASS_GRID and COLOR_CLASS_BLOCK."""
    out = (C.c_uint64 * 3)()
    _lib.load().mtg_color_class_limits(out)
    return dict(zip(("lds", "grid", "block"), map(int, out)))


def last_compact_times() -> dict:
    """Phases of the last compact_unitigs / compact_unitigs_counted on this thread: ms by HIP events around the kernel phases (pack, insert, ids, nodes, rank,
    emit), upload / download / total by the host clock, the pointer-jumping rounds, the least bytes the kernels must move and the
    peak of live device-arena bytes."""
    out = (C.c_double * 12)()
    _lib.load().mtg_last_compact_times(out)
    names = ("upload_ms", "pack_ms", "insert_ms", "ids_ms", "nodes_ms", "rank_ms", "emit_ms", "download_ms", "total_ms", "rounds", "bytes",
             "peak_arena_bytes")
    d = dict(zip(names, list(out)))
    for n in names[9:]:
        d[n] = int(d[n])
    sel = (C.c_double * 2)()
    _lib.load().mtg_last_select_times(sel)  # (a selected call's filter probe and keep stage; 0.0 elsewhere)
    d["filter_ms"], d["select_ms"] = float(sel[0]), float(sel[1])
    return d


_NONE64 = 2 ** 64 - 1


@dataclass(frozen=True)
class KmerComparison:
    """mtg_kmer_comparison (include/mtg_engine.h): the k-mer sets of two sequence sets A and B, in exact integers. The witnesses
    (first_only_in_*: record and position of the first occurrence whose k-mer the other set lacks) are 2^64 - 1 when there is none."""

    records_a: int
    records_b: int
    characters_a: int
    characters_b: int
    occurrences_a: int
    occurrences_b: int
    distinct_a: int
    distinct_b: int
    common: int
    only_in_a: int
    only_in_b: int
    first_only_in_a_record: int
    first_only_in_a_pos: int
    first_only_in_b_record: int
    first_only_in_b_pos: int

    @property
    def equal(self) -> bool:
        return self.only_in_a == 0 and self.only_in_b == 0

    @property
    def repeated_a(self) -> int:
        return self.occurrences_a - self.distinct_a

    @property
    def repeated_b(self) -> int:
        return self.occurrences_b - self.distinct_b

    def describe(self) -> str:
        """One line: B (the tigs) against A (the input)."""
        head = (f"{self.distinct_b} distinct k-mers in {self.occurrences_b} occurrences ({self.repeated_b} repeated), "
                f"{self.characters_a} -> {self.characters_b} characters")
        if self.equal:
            return f"k-mer sets equal: {head}"
        return f"k-mer sets DIFFER: {self.only_in_a} missing, {self.only_in_b} foreign; {head}"


def _sequence_arrays(x):
    """UnitigStore, list of str or (uint8 array, offsets) -> (data pointer or bytes, offsets pointer, count, keep-alive)."""
    if isinstance(x, UnitigStore):
        L = _lib.load()
        return L.mtg_unitigs_data(x.handle), L.mtg_unitigs_offsets(x.handle), len(x), x
    if isinstance(x, tuple):
        cat = np.ascontiguousarray(x[0], np.uint8)
        off = np.ascontiguousarray(x[1], np.uint64)
    else:
        cat = np.frombuffer("".join(x).encode(), np.uint8)
        off = np.zeros(len(x) + 1, np.uint64)
        off[1:] = np.cumsum([len(u) for u in x])
    if len(off) < 1:
        raise ValueError("offsets must hold count + 1 entries")
    return (_ptr(cat) if len(cat) else None), _ptr(off), len(off) - 1, (cat, off)


def compare_kmer_sets(a, b, k: int, device_id: int = 0) -> KmerComparison:
    """Do the sequence sets a and b hold the same canonical k-mers? Computed on GPU `device_id` (mtg_compare_kmer_sets,
    DESIGN.md 15). a, b: UnitigStore, list of str, or (uint8 array, offsets)."""
    L = _lib.load()
    da, oa, na, keep_a = _sequence_arrays(a)
    db, ob, nb, keep_b = _sequence_arrays(b)
    out = _lib.MtgKmerComparison()
    L.mtg_compare_kmer_sets(da, oa, na, db, ob, nb, k, device_id, C.byref(out))
    del keep_a, keep_b
    return KmerComparison(**out.as_dict())


def last_kmer_compare_times() -> dict:
    """Phases of the last compare_kmer_sets on this thread, in ms (HIP events around the kernels; upload and total by the host clock)."""
    out = (C.c_double * 6)()
    _lib.load().mtg_last_kmer_compare_times(out)
    return dict(zip(("upload_ms", "pack_ms", "insert_a_ms", "insert_b_ms", "count_ms", "total_ms"), list(out)))


def read_sequences_named(path: str):
    """Any FASTA file (optionally .gz, multi-line records) -> (UnitigStore, names): read_sequences without an alphabet rule and
    without case folding -- `N`, IUPAC codes and lower case stay as they are (the queries of a KmerIndex) -- plus the record names,
    the header text behind `>` up to the first white space (mtg_read_sequences_named)."""
    st, names = C.c_void_p(), C.c_void_p()
    _lib.load().mtg_read_sequences_named(str(path).encode(), C.byref(st), C.byref(names))
    return UnitigStore(st.value), UnitigStore(names.value).sequences()


@dataclass(frozen=True)
class FastqStats:
    """mtg_fastq_stats (include/mtg_engine.h): what one read_fastq call met, in exact integers. bases = the characters of the sequence
    lines; pieces / bases_kept = records and characters of the store; pieces_cut = the runs of bases that are not good (outside ACGT
    or below the quality threshold), counted as read_sequences(split_non_acgt=True) counts its runs; tile_bytes = the text bytes one
    block of the scan kernels takes."""

    records: int
    bases: int
    non_acgt_bases: int
    masked_bases: int
    pieces: int
    bases_kept: int
    pieces_cut: int
    tile_bytes: int

    def describe(self) -> str:
        return (f"{self.records} records, {self.bases} bases, {self.non_acgt_bases} non-ACGT bases, {self.masked_bases} bases masked by "
                f"quality -> {self.pieces} pieces of {self.bases_kept} bases")


class FastqFormatError(ValueError):
    """A FASTQ file breaks a rule of the format (read_fastq): an error of the input, the process goes on."""


def sequence_file_format(path: str) -> int:
    """What the first byte that is no line end says about a sequence file (optionally .gz): 0 = there is none, 1 = FASTA (`>`),
    2 = FASTQ (`@`), -1 = anything else (mtg_sequence_file_format). The file name plays no part."""
    return int(_lib.load().mtg_sequence_file_format(str(path).encode()))


def read_fastq(path: str, min_base_quality: int = 0, device_id: int = 0, named: bool = False):
    """Strict four-line FASTQ (optionally .gz), read on GPU `device_id` (mtg_read_fastq_split / _named). A base is good
    when it is one of ACGTacgt and its Phred quality (byte - 33) is at least min_base_quality (0 .. 93). named=False ->
    (UnitigStore, FastqStats): the maximal runs of good bases, upper-cased, in file order -- with min_base_quality = 0 exactly
    read_sequences(twin.fa, split_non_acgt=True); the store's `pieces_cut` is set as there. named=True -> (UnitigStore, names,
    FastqStats): the records whole, characters as they are, a base below the threshold replaced by `N`, as read_sequences_named.
    A malformed file raises ValueError naming the path, the first offending record (0-based), its line (1-based) and the reason."""
    if not 0 <= int(min_base_quality) <= 93:
        raise ValueError("min_base_quality must be in 0 .. 93")
    L = _lib.load()
    st, names, stats = C.c_void_p(), C.c_void_p(), _lib.MtgFastqStats()
    err = C.create_string_buffer(4096)
    if named:
        status = L.mtg_read_fastq_named(str(path).encode(), int(min_base_quality), device_id, C.byref(st), C.byref(names), C.byref(stats),
                                        err, len(err))
    else:
        status = L.mtg_read_fastq_split(str(path).encode(), int(min_base_quality), device_id, C.byref(st), C.byref(stats), err, len(err))
    if status != 0:
        raise FastqFormatError(err.value.decode(errors="replace"))
    fs = FastqStats(**stats.as_dict())
    store = UnitigStore(st.value)
    if named:
        return store, UnitigStore(names.value).sequences(), fs
    store.pieces_cut = fs.pieces_cut
    return store, fs


def last_fastq_times() -> dict:
    """Phases of the last read_fastq on this thread, in ms: read + inflate, upload, download and total by the host clock, lines (with
    the structural check) and pieces by HIP events around the kernels."""
    out = (C.c_double * 6)()
    _lib.load().mtg_last_fastq_times(out)
    return dict(zip(("read_ms", "upload_ms", "lines_ms", "pieces_ms", "download_ms", "total_ms"), list(out)))


@dataclass(frozen=True)
class KmerIndexInfo:
    """mtg_kmer_index_info (include/mtg_engine.h)."""

    k: int
    records: int
    characters: int
    occurrences: int
    distinct: int
    slots: int
    device_bytes: int


@dataclass(frozen=True, eq=False)
class KmerQueryResult:
    """What KmerIndex.query found, per query record (numpy uint64 arrays): kmers = windows, valid = windows of ACGT only, found =
    valid windows whose canonical k-mer is in the index. With bits=True also valid_bits / present_bits: one bit per global base
    position of the query (bit p & 63 of word p >> 6), set where a valid / a found window starts."""

    k: int
    offsets: np.ndarray
    kmers: np.ndarray
    valid: np.ndarray
    found: np.ndarray
    valid_bits: Optional[np.ndarray] = None
    present_bits: Optional[np.ndarray] = None

    def presence(self, i: int) -> str:
        """One character per window of record i: `1` in the index, `0` not, `-` invalid (a character outside ACGT in the window)."""
        return self.presence_lines(i, i + 1)[:-1].decode()

    def presence_lines(self, first: int = 0, last: Optional[int] = None) -> bytes:
        """presence() of the records first .. last - 1, each followed by a newline, in one vectorised pass: only the bytes of the bit
        arrays that cover those records are unpacked, so the cost is linear in their bases."""
        if self.valid_bits is None or self.present_bits is None:
            raise ValueError("presence() needs a query made with bits=True")
        last = len(self.kmers) if last is None else last
        if not 0 <= first <= last <= len(self.kmers):
            raise IndexError(f"records {first} .. {last} of {len(self.kmers)}")
        off = self.offsets[first:last + 1].astype(np.int64)
        n = self.kmers[first:last].astype(np.int64)
        byte_lo = int(off[0]) >> 3
        byte_hi = (int(off[-1]) + 7) >> 3

        def bits(a):
            return np.unpackbits(a.view(np.uint8)[byte_lo:byte_hi], bitorder="little")

        chars = np.where(bits(self.valid_bits) == 0, ord("-"), np.where(bits(self.present_bits) == 1, ord("1"), ord("0"))).astype(np.uint8)
        line_at = np.cumsum(n + 1) - (n + 1)  # where each record's line starts in the output
        out = np.full(int(n.sum()) + len(n), ord("\n"), np.uint8)
        rec = np.repeat(np.arange(len(n)), n)
        within = np.arange(len(rec)) - np.repeat(line_at - np.arange(len(n)), n)  # the window's number inside its record
        out[line_at[rec] + within] = chars[off[rec] - (byte_lo << 3) + within]
        return out.tobytes()


KMER_RUN_DTYPE = np.dtype([("q_record", np.uint64), ("q_start", np.uint64), ("kmers", np.uint64), ("strand", np.uint8),
                           ("t_record", np.uint64), ("t_start", np.uint64)])


@dataclass(frozen=True, eq=False)
class KmerLocateResult:
    """What KmerIndex.locate found: kmers / valid / found per query record as KmerIndex.query gives them, and `runs`, a structured
    array (KMER_RUN_DTYPE) with one entry per maximal collinear run of found windows, in ascending query position: the `kmers`
    windows from offset q_start of query record q_record on lie, one after the other, from offset t_start of index record t_record
    on -- read forwards (strand 0) or as the reverse complement (strand 1). Query bases [q_start, q_start + kmers + k - 1) equal
    index bases [t_start, t_start + kmers + k - 1)."""

    k: int
    offsets: np.ndarray
    kmers: np.ndarray
    valid: np.ndarray
    found: np.ndarray
    runs: np.ndarray


@dataclass(frozen=True, eq=False)
class KmerAbundanceResult:
    """What KmerIndex.abundance found, per query record: kmers / valid / found as KmerIndex.query gives them (uint64), and over the
    found windows of the record sum (uint64), min and max (uint32) of the weights of their k-mers -- all 0 where nothing was found.
    With per_window=True also per_window (uint32, one entry per global base position of the query): the weight of the k-mer of the
    window that starts there if it is valid and found, else 0."""

    k: int
    offsets: np.ndarray
    kmers: np.ndarray
    valid: np.ndarray
    found: np.ndarray
    sum: np.ndarray
    min: np.ndarray
    max: np.ndarray
    per_window: Optional[np.ndarray] = None

    @property
    def mean(self) -> np.ndarray:
        """sum / found per record as float64; nan where nothing was found."""
        out = np.full(len(self.found), np.nan)
        np.divide(self.sum, self.found, out=out, where=self.found > 0)
        return out


@dataclass(frozen=True, eq=False)
class KmerColorResult:
    """What KmerIndex.color_hits found, per query record: kmers / valid / found as KmerIndex.query gives them (uint64), and per_color
    (uint32[records, n_colors]): the found windows of the record whose k-mer's mask has bit c -- a mask of 0 is found and touches no
    column. With per_window=True also per_window (uint64, one entry per global base position of the query): the mask of the k-mer of
    the window that starts there if it is valid and found, else 0."""

    k: int
    offsets: np.ndarray
    kmers: np.ndarray
    valid: np.ndarray
    found: np.ndarray
    per_color: np.ndarray
    per_window: Optional[np.ndarray] = None


def _window_count(seqs_or_store, k: int) -> int:
    """The windows of length k inside the records: what a KmerIndex of them reports as info.occurrences."""
    if isinstance(seqs_or_store, UnitigStore):
        lengths = np.diff(seqs_or_store.arrays()[1]).astype(np.int64)
    elif isinstance(seqs_or_store, tuple):
        lengths = np.diff(np.asarray(seqs_or_store[1], np.uint64)).astype(np.int64)
    else:
        lengths = np.array([len(s) for s in seqs_or_store], np.int64)
    return int(np.maximum(lengths - (k - 1), 0).sum())


def _take_runs(L, h) -> np.ndarray:
    """The runs of a mtg_kmer_runs handle as a KMER_RUN_DTYPE array of its own; the handle is freed."""
    try:
        count = int(L.mtg_kmer_runs_count(h))
        runs = np.zeros(count, KMER_RUN_DTYPE)
        if count:
            ptrs = [C.c_void_p() for _ in range(6)]
            L.mtg_kmer_runs_arrays(h, *(C.byref(p) for p in ptrs))
            for name, p in zip(("q_record", "q_start", "kmers", "strand", "t_record", "t_start"), ptrs):
                ctype = C.c_uint8 if name == "strand" else C.c_uint64
                runs[name] = np.ctypeslib.as_array(C.cast(p, C.POINTER(ctype)), shape=(count,))
    finally:
        L.mtg_kmer_runs_free(h)
    return runs


KMER_WALK_DTYPE = np.dtype([(name, np.uint64) for name in ("q_record", "q_start", "q_end", "kmers", "steps", "first_step", "path_len",
                                                           "path_start", "path_end")])


@dataclass(frozen=True, eq=False)
class KmerThreadResult:
    """What KmerIndex.thread found: kmers / valid / found per query record as KmerIndex.query gives them; `walks`, a
    structured array (KMER_WALK_DTYPE) with one entry per walk in ascending query position; and `steps` (uint64), the steps of all
    walks one after the other, (t_record << 1) | strand each -- those of walk w are steps[first_step : first_step + steps]. A walk
    spells query bases [q_start, q_end) as bases [path_start, path_end) of its path, the steps as oriented glued with k - 1
    overlapping bases, path_len bases long. The result holds the library's handle until close() (or its collection): gaf() formats
    from it."""

    k: int
    offsets: np.ndarray
    kmers: np.ndarray
    valid: np.ndarray
    found: np.ndarray
    walks: np.ndarray
    steps: np.ndarray
    _handle: list = None  # [the mtg_kmer_walks handle or None]

    def close(self) -> None:
        if self._handle and self._handle[0]:
            _lib.load().mtg_kmer_walks_free(self._handle[0])
            self._handle[0] = None

    __del__ = close

    def gaf(self, query_names, segment_names=None, query_lengths=None) -> bytes:
        """The walks as GAF text, one line per walk (mtg_kmer_walks_gaf; made by the library, no Python loop over walks or steps).
        query_names / segment_names: one name per query record / per index record (list of str, UnitigStore, or (uint8 array,
        offsets)); segment_names=None names index record u by its decimal number, as --unitigs-gfa-out does. query_lengths: default
        the lengths of the threaded records."""
        if not self._handle or not self._handle[0]:
            raise ValueError("the result is closed")
        L = _lib.load()
        qd, qo, qn, keep_q = _sequence_arrays(query_names)
        if qn != len(self.kmers):
            raise ValueError(f"{qn} query names for {len(self.kmers)} records")
        lengths = np.ascontiguousarray(np.diff(self.offsets) if query_lengths is None else query_lengths, np.uint64)
        if len(lengths) != qn:
            raise ValueError(f"{len(lengths)} query lengths for {qn} records")
        sd, so, sn, keep_s = (None, None, 0, None) if segment_names is None else _sequence_arrays(segment_names)
        if segment_names is not None and sd is None:
            sd = b""  # (names of no bytes are names all the same)
        if segment_names is not None and len(self.steps) and int(self.steps.max() >> np.uint64(1)) >= sn:
            raise ValueError(f"{sn} segment names, but a step on segment {int(self.steps.max() >> np.uint64(1))}")
        text = C.c_void_p()
        n = int(L.mtg_kmer_walks_gaf(self._handle[0], qn, qd, qo, _ptr(lengths), sn, sd, so, C.byref(text)))
        try:
            return C.string_at(text, n)
        finally:
            L.mtg_free(text)
            del keep_q, keep_s


def _take_walks_result(L, h, k, off, kmers, valid, found) -> KmerThreadResult:
    """The walks of a mtg_kmer_walks handle as arrays of their own; the result keeps the handle for gaf()."""
    count, n_steps = int(L.mtg_kmer_walks_count(h)), int(L.mtg_kmer_walks_steps_count(h))
    walks, steps = np.zeros(count, KMER_WALK_DTYPE), np.zeros(n_steps, np.uint64)
    if count:
        ptrs = (C.c_void_p * 9)()
        L.mtg_kmer_walks_arrays(h, ptrs)
        for name, p in zip(KMER_WALK_DTYPE.names, ptrs):
            walks[name] = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint64)), shape=(count,))
        steps[:] = np.ctypeslib.as_array(C.cast(L.mtg_kmer_walks_steps(h), C.POINTER(C.c_uint64)), shape=(n_steps,))
    return KmerThreadResult(k, off, kmers, valid, found, walks, steps, [h])


def _thread(index, call: str, seqs_or_store, min_kmers: int) -> KmerThreadResult:
    """KmerIndex.thread and TigIndex.thread."""
    if int(min_kmers) < 0:
        raise ValueError("min_kmers must be >= 0")
    d, o, n, keep, off, kmers, valid, found = index._probe_inputs(seqs_or_store, index.locating, "thread() needs an index built with locate=True")
    h = C.c_void_p()
    getattr(index._L, call)(index._h, d, o, n, int(min_kmers), _ptr(kmers), _ptr(valid), _ptr(found), C.byref(h))
    del keep
    return _take_walks_result(index._L, h, index.info.k, off, kmers, valid, found)


def _payload_arrays(seqs_or_store, k: int, weights, colors, n_colors):
    """The per-window payloads of an index as the library takes them (KmerIndex, TigIndex): weights as a uint32 array, colors as a
    uint64 array, None for one not given; ValueError unless each holds one entry per window, n_colors is in 1..64 and no mask has
    a bit beyond it."""
    if colors is not None:
        if isinstance(n_colors, bool) or not isinstance(n_colors, (int, np.integer)) or not 1 <= n_colors <= MAX_COLORS:
            raise ValueError(f"n_colors must be in 1..{MAX_COLORS}, not {n_colors!r}")
    elif n_colors is not None:
        raise ValueError("n_colors needs colors")
    c = w = None
    if colors is not None or weights is not None:
        windows = _window_count(seqs_or_store, k) if k >= 1 else -1
    if colors is not None:
        c = np.ascontiguousarray(colors, np.uint64)
        if c.ndim != 1 or len(c) != windows:
            raise ValueError(f"colors must hold one entry per window: {c.shape} for {windows} windows")
        if n_colors < MAX_COLORS and len(c) and int(c.max()) >> int(n_colors):
            raise ValueError(f"a mask has a colour beyond the {n_colors} given")
    if weights is not None:
        w = np.ascontiguousarray(weights, np.uint32)
        if w.ndim != 1 or len(w) != windows:
            raise ValueError(f"weights must hold one entry per window: {w.shape} for {windows} windows")
    return w, c


class KmerIndex:
    """The canonical k-mers of a sequence set, kept on GPU `device_id` and asked which k-mers of other sequences they hold
    (mtg_kmer_index_*). seqs_or_store: UnitigStore, list of str, or (uint8 array, offsets); ACGT of either case only.
    The index holds device memory until close() (or its collection); release_device_memory leaves it intact. locate=True: the index
    also keeps where its k-mers are (more device memory, see info.device_bytes) and answers locate(). weights: an
    array-like of uint32, one per window of the sequences in window order (the k-mers of record 0 from left to right, then record
    1's, ...; a record shorter than k has none): the index also keeps a weight per k-mer -- that of its first occurrence -- and
    answers abundance(). colors with n_colors (1..64): an array-like of uint64, one mask per window in the same order:
    the index also keeps a mask per k-mer -- that of its first occurrence -- and answers color_hits(). An index may
    carry weights, colours, both or neither."""

    def __init__(self, seqs_or_store, k: int, device_id: int = 0, locate: bool = False, weights=None, colors=None, n_colors=None):
        self._L = _lib.load()
        self._h = None
        self.locating = bool(locate)
        self.weighted = weights is not None
        self.colored = colors is not None
        self.n_colors = 0
        w, c = _payload_arrays(seqs_or_store, k, weights, colors, n_colors)
        # one symbol (+ "_store" for a UnitigStore) and what it takes behind k, per kind of index
        if self.colored:
            build, payload = "mtg_kmer_index_build_annotated", (_ptr(w), len(w) if self.weighted else 0, _ptr(c), len(c), int(n_colors),
                                                                int(self.locating), device_id)
            self.n_colors = int(n_colors)
        elif self.weighted:
            build, payload = "mtg_kmer_index_build_weighted", (_ptr(w), len(w), int(self.locating), device_id)
        else:
            build, payload = "mtg_kmer_index_build_locating" if locate else "mtg_kmer_index_build", (device_id,)
        if isinstance(seqs_or_store, UnitigStore):
            self._h = getattr(self._L, build + "_store")(seqs_or_store.handle, k, *payload)
        else:
            d, o, n, keep = _sequence_arrays(seqs_or_store)
            self._h = getattr(self._L, build)(d, o, n, k, *payload)
            del keep
        out = _lib.MtgKmerIndexInfo()
        self._L.mtg_kmer_index_get_info(self._h, C.byref(out))
        self.info = KmerIndexInfo(**out.as_dict())

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._L.mtg_kmer_index_free(h)

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _probe_inputs(self, seqs_or_store, able: bool = True, needs: str = ""):
        """What every probe starts from -- the index open (checked first) and `able` to answer, else ValueError(needs) -- as (data,
        offsets pointer, records, keep-alive, a copy of the offsets, and kmers, valid, found: zeroed uint64 per record)."""
        if not self._h:
            raise ValueError("the index is closed")
        if not able:
            raise ValueError(needs)
        d, o, n, keep = _sequence_arrays(seqs_or_store)
        off = np.ctypeslib.as_array(C.cast(o, C.POINTER(C.c_uint64)), shape=(n + 1,)).copy()
        return (d, o, n, keep, off, *(np.zeros(n, np.uint64) for _ in range(3)))

    def query(self, seqs_or_store, bits: bool = False) -> KmerQueryResult:
        """Per record of seqs_or_store (UnitigStore, list of str, or (uint8 array, offsets); ANY bytes): windows, valid windows,
        windows found in the index. bits: also the two bit arrays that presence() reads."""
        d, o, n, keep, off, kmers, valid, found = self._probe_inputs(seqs_or_store)
        words = (int(off[n]) + 63) // 64
        vb, pb = (np.zeros(words, np.uint64), np.zeros(words, np.uint64)) if bits else (None, None)
        self._L.mtg_kmer_index_query(self._h, d, o, n, _ptr(kmers), _ptr(valid), _ptr(found), _ptr(pb) if bits else None,
                                     _ptr(vb) if bits else None)
        del keep
        return KmerQueryResult(self.info.k, off, kmers, valid, found, vb, pb)

    def locate(self, seqs_or_store) -> KmerLocateResult:
        """query()'s counts per record plus where the found windows lie in the indexed sequences, folded into maximal collinear
        runs (KmerLocateResult). A k-mer that occurs several times in the index is reported at its smallest position only. Needs
        an index built with locate=True."""
        d, o, n, keep, off, kmers, valid, found = self._probe_inputs(seqs_or_store, self.locating, "locate() needs an index built with locate=True")
        h = C.c_void_p()
        self._L.mtg_kmer_index_locate(self._h, d, o, n, _ptr(kmers), _ptr(valid), _ptr(found), C.byref(h))
        del keep
        return KmerLocateResult(self.info.k, off, kmers, valid, found, _take_runs(self._L, h))

    def thread(self, seqs_or_store, min_kmers: int = 1) -> KmerThreadResult:
        """query()'s counts per record plus the walks of the records through the indexed sequences (KmerThreadResult):
        the runs of locate() joined wherever one leaves an index record at its end and the next enters another at its start. Over
        unitigs every walk is a path of the unitig graph. Walks of fewer than min_kmers k-mers are dropped on the device. Needs an
        index built with locate=True."""
        return _thread(self, "mtg_kmer_index_thread", seqs_or_store, min_kmers)

    def abundance(self, seqs_or_store, per_window: bool = False) -> KmerAbundanceResult:
        """query()'s counts per record plus the sum, the smallest and the largest weight over the record's found windows
        (KmerAbundanceResult); per_window: also the weight at every window start. Needs an index built with weights."""
        d, o, n, keep, off, kmers, valid, found = self._probe_inputs(seqs_or_store, self.weighted, "abundance() needs an index built with weights")
        total, lo, hi = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        pw = np.zeros(int(off[n]), np.uint32) if per_window else None
        self._L.mtg_kmer_index_abundance(self._h, d, o, n, _ptr(kmers), _ptr(valid), _ptr(found), _ptr(total), _ptr(lo), _ptr(hi),
                                         _ptr(pw) if per_window else None)
        del keep
        return KmerAbundanceResult(self.info.k, off, kmers, valid, found, total, lo, hi, pw)

    def color_hits(self, seqs_or_store, per_window: bool = False) -> KmerColorResult:
        """query()'s counts per record plus, per record and colour, the found windows whose k-mer that colour carries
        (KmerColorResult); per_window: also the mask at every window start. Needs an index built with colors."""
        d, o, n, keep, off, kmers, valid, found = self._probe_inputs(seqs_or_store, self.colored, "color_hits() needs an index built with colors")
        per_color = np.zeros((n, self.n_colors), np.uint32)
        pw = np.zeros(int(off[n]), np.uint64) if per_window else None
        self._L.mtg_kmer_index_colors(self._h, d, o, n, _ptr(kmers), _ptr(valid), _ptr(found), _ptr(per_color), _ptr(pw) if per_window else None)
        del keep
        return KmerColorResult(self.info.k, off, kmers, valid, found, per_color, pw)


@dataclass(frozen=True, eq=False)
class KmerCoverageResult:
    """What KmerTally.coverage found, per asked record (numpy uint64 arrays): kmers / valid / found as KmerIndex.query gives them,
    and over the found windows of the record covered = those whose k-mer was added at least once, sum = the sum of the tallies of
    their k-mers, max = the largest such tally -- all 0 where nothing was found. With per_window=True also per_window (one entry per
    global base position of the asked sequences): the tally of the k-mer of the window that starts there if it is valid and found,
    else 0."""

    k: int
    offsets: np.ndarray
    kmers: np.ndarray
    valid: np.ndarray
    found: np.ndarray
    covered: np.ndarray
    sum: np.ndarray
    max: np.ndarray
    per_window: Optional[np.ndarray] = None


class KmerTally:
    """How often other sequences see the k-mers of a KmerIndex (mtg_kmer_tally_*): one 64-bit counter per k-mer of the
    index, zero at first, on the index's GPU (device_bytes, until close() or collection). add(reads) counts every valid window of
    the reads whose k-mer is in the index, on either strand, repeats included; any number of adds accumulate. coverage(sequences)
    reads the counters back along any sequences -- the indexed ones give their depth in the reads. The index may be plain, locating,
    weighted or coloured and is never changed; the tally keeps a reference to it, and several tallies on one index are independent."""

    def __init__(self, index: KmerIndex):
        self._h = None
        if not isinstance(index, KmerIndex):
            raise TypeError("KmerTally counts on a KmerIndex")
        if not index._h:
            raise ValueError("the index is closed")
        self.index = index
        self._L = index._L
        self._h = self._L.mtg_kmer_tally_create(index._h)
        self.device_bytes = int(self._L.mtg_kmer_tally_device_bytes(self._h))

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._L.mtg_kmer_tally_free(h)

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _open(self) -> None:
        """The tally open and its index open, else ValueError: before the library is asked."""
        if not self._h:
            raise ValueError("the tally is closed")
        if not self.index._h:
            raise ValueError("the index is closed")

    def add(self, seqs_or_store) -> KmerQueryResult:
        """Count the k-mers of seqs_or_store (UnitigStore, list of str, or (uint8 array, offsets); ANY bytes) that the index holds
        -> what KmerIndex.query says of them."""
        self._open()
        d, o, n, keep, off, kmers, valid, found = self.index._probe_inputs(seqs_or_store)
        if isinstance(seqs_or_store, UnitigStore):
            self._L.mtg_kmer_tally_add_store(self._h, seqs_or_store.handle, _ptr(kmers), _ptr(valid), _ptr(found))
        else:
            self._L.mtg_kmer_tally_add(self._h, d, o, n, _ptr(kmers), _ptr(valid), _ptr(found))
        del keep
        return KmerQueryResult(self.index.info.k, off, kmers, valid, found)

    def coverage(self, seqs_or_store, per_window: bool = False) -> KmerCoverageResult:
        """KmerIndex.query's counts per record of seqs_or_store plus, over its found windows, how many were added at least once, the
        sum and the largest of their tallies (KmerCoverageResult); per_window: also the tally at every window start."""
        self._open()
        d, o, n, keep, off, kmers, valid, found = self.index._probe_inputs(seqs_or_store)
        covered, total, hi = (np.zeros(n, np.uint64) for _ in range(3))
        pw = np.zeros(int(off[n]), np.uint64) if per_window else None
        outs = (_ptr(kmers), _ptr(valid), _ptr(found), _ptr(covered), _ptr(total), _ptr(hi), _ptr(pw) if per_window else None)
        if isinstance(seqs_or_store, UnitigStore):
            self._L.mtg_kmer_tally_coverage_store(self._h, seqs_or_store.handle, *outs)
        else:
            self._L.mtg_kmer_tally_coverage(self._h, d, o, n, *outs)
        del keep
        return KmerCoverageResult(self.index.info.k, off, kmers, valid, found, covered, total, hi, pw)

    def reset(self) -> None:
        """Every counter zero again."""
        self._open()
        self._L.mtg_kmer_tally_reset(self._h)


def last_kmer_tally_times() -> dict:
    """Phases of the last KmerTally.add or KmerTally.coverage on this thread, in ms (HIP events around the kernels; upload and
    download by the host clock)."""
    out = (C.c_double * 4)()
    _lib.load().mtg_last_kmer_tally_times(out)
    return dict(zip(("upload_ms", "pack_ms", "probe_ms", "download_ms"), list(out)))


def default_minimizer_length(k: int) -> int:
    """The minimizer length a TigIndex takes when none is given: min(19, ceil(2 k / 3)) -- 19 at k = 31."""
    return min(19, (2 * k + 2) // 3)


@dataclass(frozen=True)
class TigIndexInfo:
    """mtg_tig_index_info (include/mtg_engine.h)."""

    k: int
    m: int
    records: int
    characters: int
    occurrences: int
    anchors: int
    buckets: int
    bucket_limit: int
    heavy_buckets: int
    heavy_windows: int
    table_slots: int
    device_bytes: int

    @property
    def bytes_per_kmer(self) -> float:
        """Device bytes per k-mer window of the indexed sequences; 0.0 for an index without windows."""
        return self.device_bytes / self.occurrences if self.occurrences else 0.0

    def describe(self) -> str:
        return (f"minimizer index (m = {self.m}): {self.characters} bases in {self.records} records, {self.anchors} anchors in "
                f"{self.buckets} buckets, {self.heavy_buckets} heavy buckets with {self.heavy_windows} windows, {self.device_bytes} device "
                f"bytes, {self.bytes_per_kmer:.2f} bytes per k-mer window")


class IndexFileError(ValueError):
    """An index file is refused (TigIndex.load, tig_index_file_info) or cannot be written (TigIndex.save): an error of the file,
    the process goes on. The message names the path, the section where there is one, and the check."""


def _payload_info_dict(pi) -> dict:
    names = {1: "dense", 2: "runs"}
    return {key: dict(one.as_dict(), layout=names[int(one.layout)]) for key, one in (("weights", pi.weights), ("colors", pi.colors)) if one.layout}


def _meta_dict(blob: bytes, path) -> dict:
    if not blob:
        return {}
    try:
        meta = json.loads(blob.decode("utf-8"))
    except ValueError as e:
        raise IndexFileError(f"{path}: metadata: not a UTF-8 JSON object ({e})") from None
    if not isinstance(meta, dict):
        raise IndexFileError(f"{path}: metadata: not a JSON object")
    return meta


def tig_index_file_info(path) -> dict:
    """What the header of an index file says (mtg_tig_index_file_info), after the header checks of a load and nothing
    more -- on the host alone, no GPU is touched: {"info": TigIndexInfo, "locating", "weighted", "colored", "n_colors",
    "payload_info", "win_offset_bytes", "meta": dict, "file_bytes"}. A refused header raises IndexFileError."""
    L = _lib.load()
    info, pi, locating, meta_len = _lib.MtgTigIndexInfo(), _lib.MtgTigPayloadInfo(), C.c_int(0), C.c_uint64(0)
    err = C.create_string_buffer(4096)
    blob = C.create_string_buffer(1)
    for _ in range(2):  # (the second call has room for the whole blob)
        if L.mtg_tig_index_file_info(str(path).encode(), C.byref(info), C.byref(pi), C.byref(locating), blob, len(blob), C.byref(meta_len),
                                     err, len(err)) != 0:
            raise IndexFileError(err.value.decode(errors="replace"))
        if meta_len.value <= len(blob):
            break
        blob = C.create_string_buffer(int(meta_len.value))
    return {"info": TigIndexInfo(**info.as_dict()), "locating": bool(locating.value), "weighted": bool(pi.weights.layout),
            "colored": bool(pi.colors.layout), "n_colors": int(pi.n_colors), "payload_info": _payload_info_dict(pi),
            "win_offset_bytes": int(pi.win_offset_bytes), "meta": _meta_dict(blob.raw[:int(meta_len.value)], path),
            "file_bytes": os.path.getsize(path)}


def last_tig_index_file_times() -> dict:
    """Phases on this thread, in ms: of the last TigIndex.save the digest kernels (HIP events), the download and the write (host
    clock); of the last TigIndex.load the read and the upload (host clock), the digest kernels and the validation kernel (HIP events)."""
    out = (C.c_double * 7)()
    _lib.load().mtg_last_tig_index_file_times(out)
    return {"save": dict(zip(("digest_ms", "download_ms", "write_ms"), out[0:3])),
            "load": dict(zip(("read_ms", "upload_ms", "digest_ms", "validate_ms"), out[3:7]))}


class TigIndex:
    """The canonical k-mers of a sequence set as a sparse index on GPU `device_id` (mtg_tig_index_*): the 2-bit packed
    bases plus one word per minimizer anchor instead of KmerIndex's table slot per window, so its size follows the cumulative length
    of the sequences -- tigs index smaller than unitigs. query() answers exactly as KmerIndex.query does. seqs_or_store: UnitigStore,
    list of str, or (uint8 array, offsets); ACGT of either case only. m: the minimizer length, 1 .. min(k, 31) (None:
    default_minimizer_length(k)). bucket_limit: a directory bucket with more anchors sends its windows to a class table (None: 64).
    The index holds device memory until close() (or its collection); release_device_memory leaves it intact. locate=True (DESIGN.md
    30): a LOCATING index, which also answers locate() exactly as KmerIndex(locate=True).locate does, at the coordinates of
    seqs_or_store; it keeps 8 B per slot of the heavy buckets' table more, nothing more where no bucket is heavy.
    TigIndex.annotated(..., weights=, colors=, n_colors=, payload_layout=): weights / colors with n_colors are
    exactly what KmerIndex takes, one entry per window in window order; the index is then locating and also answers abundance() /
    color_hits() exactly as the annotated KmerIndex does -- the payload of a k-mer is that of its first occurrence. Each payload is
    kept per window of the text, dense or as runs of equal entries, whichever is smaller (a tie is dense; payload_layout "dense" or
    "runs" forces one): see payload_info ({"weights": {...}, "colors": {...}}, each with layout, width, windows, runs,
    device_bytes; {} on an index without payloads).
    save(path, meta) / TigIndex.load(path): the index as a file and back, without its sequences; `meta` is the dict
    given to the last save or read by load ({} otherwise)."""

    _LAYOUTS = {None: 0, "dense": 1, "runs": 2}

    def __init__(self, seqs_or_store, k: int, m: Optional[int] = None, device_id: int = 0, bucket_limit: Optional[int] = None,
                 locate: bool = False):
        self._build(seqs_or_store, k, m, device_id, bucket_limit, locate)

    @classmethod
    def annotated(cls, seqs_or_store, k: int, m: Optional[int] = None, device_id: int = 0, bucket_limit: Optional[int] = None,
                  weights=None, colors=None, n_colors=None, payload_layout: Optional[str] = None) -> "TigIndex":
        """A locating index with weights, colours, both or neither (see the class). The ValueErrors are KmerIndex's, raised before
        the library is asked."""
        ix = cls.__new__(cls)
        ix._build(seqs_or_store, k, m, device_id, bucket_limit, True, weights, colors, n_colors, payload_layout)
        return ix

    def _build(self, seqs_or_store, k, m, device_id, bucket_limit, locate, weights=None, colors=None, n_colors=None, payload_layout=None):
        self._h = None
        self.weighted = weights is not None
        self.colored = colors is not None
        self.n_colors = 0
        self.payload_info = {}
        self.meta = {}
        if m is not None and not 1 <= m <= min(k, 31):
            raise ValueError(f"m must be in 1..min(k, 31), not {m!r}")
        if bucket_limit is not None and not 1 <= bucket_limit <= 65536:
            raise ValueError(f"bucket_limit must be in 1..65536, not {bucket_limit!r}")
        if payload_layout not in self._LAYOUTS:
            raise ValueError(f"payload_layout must be None, 'dense' or 'runs', not {payload_layout!r}")
        if payload_layout is not None and not (self.weighted or self.colored):
            raise ValueError("payload_layout needs weights or colors")
        w, c = _payload_arrays(seqs_or_store, k, weights, colors, n_colors)
        self._L = _lib.load()
        annotated = self.weighted or self.colored
        self.locating = bool(locate) or annotated
        if annotated:
            build = "mtg_tig_index_build_annotated"
            payload = (_ptr(w) if self.weighted else None, len(w) if self.weighted else 0, _ptr(c) if self.colored else None,
                       len(c) if self.colored else 0, int(n_colors) if self.colored else 0, self._LAYOUTS[payload_layout], device_id)
        else:
            build, payload = "mtg_tig_index_build_locating" if locate else "mtg_tig_index_build", (device_id,)
        if isinstance(seqs_or_store, UnitigStore):
            self._h = getattr(self._L, build + "_store")(seqs_or_store.handle, k, m or 0, bucket_limit or 0, *payload)
        else:
            d, o, n, keep = _sequence_arrays(seqs_or_store)
            self._h = getattr(self._L, build)(d, o, n, k, m or 0, bucket_limit or 0, *payload)
            del keep
        out = _lib.MtgTigIndexInfo()
        self._L.mtg_tig_index_get_info(self._h, C.byref(out))
        self.info = TigIndexInfo(**out.as_dict())
        if annotated:
            pi = _lib.MtgTigPayloadInfo()
            self._L.mtg_tig_index_get_payload_info(self._h, C.byref(pi))
            self.payload_info = _payload_info_dict(pi)
            self.n_colors = int(pi.n_colors)

    def save(self, path, meta: Optional[dict] = None) -> int:
        """Writes the index to `path` (mtg_tig_index_save; conventional suffix .mtgx) and returns the bytes written.
        meta: a JSON-serialisable dict the file carries and load() returns; the library stores it without reading it. The file is a
        function of the index and meta alone. A file that cannot be written raises IndexFileError."""
        if not self._h:
            raise ValueError("the index is closed")
        blob = json.dumps(meta if meta is not None else {}, ensure_ascii=False, sort_keys=True, separators=(",", ":")).encode("utf-8")
        err = C.create_string_buffer(4096)
        if self._L.mtg_tig_index_save(self._h, str(path).encode(), blob, len(blob), err, len(err)) != 0:
            raise IndexFileError(err.value.decode(errors="replace"))
        self.meta = dict(meta) if meta is not None else {}
        return os.path.getsize(path)

    @classmethod
    def load(cls, path, device_id: int = 0) -> "TigIndex":
        """The index of a file written by save() (mtg_tig_index_load): read and uploaded, not rebuilt; info,
        locating, weighted, colored, n_colors and payload_info as the builder filled them, plus meta. A file that is damaged,
        truncated, of a later format version or whose arrays break an invariant of the probes raises IndexFileError naming the
        path, the section and the check; nothing of it stays on the device."""
        ix = cls.__new__(cls)
        ix._h = None
        ix._L = _lib.load()
        err = C.create_string_buffer(4096)
        ix._h = ix._L.mtg_tig_index_load(str(path).encode(), device_id, err, len(err))
        if not ix._h:
            raise IndexFileError(err.value.decode(errors="replace"))
        out, pi, n = _lib.MtgTigIndexInfo(), _lib.MtgTigPayloadInfo(), C.c_uint64(0)
        ix._L.mtg_tig_index_get_info(ix._h, C.byref(out))
        ix._L.mtg_tig_index_get_payload_info(ix._h, C.byref(pi))
        ix.info = TigIndexInfo(**out.as_dict())
        ix.locating = bool(ix._L.mtg_tig_index_is_locating(ix._h))
        ix.weighted, ix.colored = bool(pi.weights.layout), bool(pi.colors.layout)
        ix.payload_info = _payload_info_dict(pi)
        ix.n_colors = int(pi.n_colors)
        p = ix._L.mtg_tig_index_meta(ix._h, C.byref(n))
        ix.meta = _meta_dict(C.string_at(p, int(n.value)) if n.value else b"", path)
        return ix

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._L.mtg_tig_index_free(h)

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def query(self, seqs_or_store, bits: bool = False) -> KmerQueryResult:
        """KmerIndex.query's answer: per record of seqs_or_store (ANY bytes) windows, valid windows, windows found in the index;
        bits: also the two bit arrays that presence() reads."""
        if not self._h:
            raise ValueError("the index is closed")
        d, o, n, keep = _sequence_arrays(seqs_or_store)
        off = np.ctypeslib.as_array(C.cast(o, C.POINTER(C.c_uint64)), shape=(n + 1,)).copy()
        kmers, valid, found = (np.zeros(n, np.uint64) for _ in range(3))
        words = (int(off[n]) + 63) // 64
        vb, pb = (np.zeros(words, np.uint64), np.zeros(words, np.uint64)) if bits else (None, None)
        self._L.mtg_tig_index_query(self._h, d, o, n, _ptr(kmers), _ptr(valid), _ptr(found), _ptr(pb) if bits else None,
                                    _ptr(vb) if bits else None)
        del keep
        return KmerQueryResult(self.info.k, off, kmers, valid, found, vb, pb)

    def locate(self, seqs_or_store) -> KmerLocateResult:
        """KmerIndex.locate's answer: query()'s counts per record plus where the found windows lie in the indexed sequences, folded
        into maximal collinear runs (KmerLocateResult). A k-mer that occurs several times in the index is reported at its smallest
        position only. Needs an index built with locate=True."""
        if not self._h:
            raise ValueError("the index is closed")
        if not self.locating:
            raise ValueError("locate() needs an index built with locate=True")
        d, o, n, keep = _sequence_arrays(seqs_or_store)
        off = np.ctypeslib.as_array(C.cast(o, C.POINTER(C.c_uint64)), shape=(n + 1,)).copy()
        kmers, valid, found = (np.zeros(n, np.uint64) for _ in range(3))
        h = C.c_void_p()
        self._L.mtg_tig_index_locate(self._h, d, o, n, _ptr(kmers), _ptr(valid), _ptr(found), C.byref(h))
        del keep
        return KmerLocateResult(self.info.k, off, kmers, valid, found, _take_runs(self._L, h))

    _probe_inputs = KmerIndex._probe_inputs  # (the same checks in the same order: closed first, then the missing payload)

    def thread(self, seqs_or_store, min_kmers: int = 1) -> KmerThreadResult:
        """KmerIndex.thread's answer, field for field, for every m and bucket_limit. Needs an index built with
        locate=True."""
        return _thread(self, "mtg_tig_index_thread", seqs_or_store, min_kmers)

    def abundance(self, seqs_or_store, per_window: bool = False) -> KmerAbundanceResult:
        """KmerIndex.abundance's answer: query()'s counts per record plus the sum, the smallest and the largest weight
        over the record's found windows; per_window: also the weight at every window start. Needs an index built with weights."""
        d, o, n, keep, off, kmers, valid, found = self._probe_inputs(seqs_or_store, self.weighted, "abundance() needs an index built with weights")
        total, lo, hi = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        pw = np.zeros(int(off[n]), np.uint32) if per_window else None
        self._L.mtg_tig_index_abundance(self._h, d, o, n, _ptr(kmers), _ptr(valid), _ptr(found), _ptr(total), _ptr(lo), _ptr(hi),
                                        _ptr(pw) if per_window else None)
        del keep
        return KmerAbundanceResult(self.info.k, off, kmers, valid, found, total, lo, hi, pw)

    def color_hits(self, seqs_or_store, per_window: bool = False) -> KmerColorResult:
        """KmerIndex.color_hits' answer: query()'s counts per record plus, per record and colour, the found windows
        whose k-mer that colour carries; per_window: also the mask at every window start. Needs an index built with colors."""
        d, o, n, keep, off, kmers, valid, found = self._probe_inputs(seqs_or_store, self.colored, "color_hits() needs an index built with colors")
        per_color = np.zeros((n, self.n_colors), np.uint32)
        pw = np.zeros(int(off[n]), np.uint64) if per_window else None
        self._L.mtg_tig_index_colors(self._h, d, o, n, _ptr(kmers), _ptr(valid), _ptr(found), _ptr(per_color), _ptr(pw) if per_window else None)
        del keep
        return KmerColorResult(self.info.k, off, kmers, valid, found, per_color, pw)


def last_tig_payload_times() -> dict:
    """Phases on this thread, in ms (HIP events around the kernels; uploads by the host clock): of the last annotated TigIndex build,
    per payload the upload, the max-reduction, flag + scan and the compaction or the narrowing copy; of the last TigIndex.abundance
    or .color_hits the upload, the pack, the probe (the locate pass with the fill of the hit array) and the gather."""
    out = (C.c_double * 12)()
    _lib.load().mtg_last_tig_payload_times(out)
    phases = ("upload_ms", "reduce_ms", "flag_scan_ms", "store_ms")
    return {"weights": dict(zip(phases, out[0:4])), "colors": dict(zip(phases, out[4:8])),
            **dict(zip(("upload_ms", "pack_ms", "probe_ms", "gather_ms"), out[8:12]))}


class TigTally:
    """KmerTally on the sparse index (mtg_tig_tally_*): how often other sequences see the k-mers of a LOCATING TigIndex
    (locate=True or TigIndex.annotated). One 64-bit counter per window of the indexed text (`windows` of them, 8 B each; device_bytes
    also counts the windows-before-every-record array where the index keeps none), zero at first, on the index's GPU until close()
    or collection. add / coverage / reset answer exactly as KmerTally's do on a KmerIndex over the same sequences: a k-mer is counted
    at the window where its class occurs first in the text, so counters() -- the counters in window order -- holds 0 at every later
    occurrence and sums to the found windows added. The index is never changed; the tally keeps a reference to it, and several
    tallies on one index are independent."""

    def __init__(self, index: "TigIndex"):
        self._h = None
        if not isinstance(index, TigIndex):
            raise TypeError("TigTally counts on a TigIndex")
        if not index._h:
            raise ValueError("the index is closed")
        if not index.locating:
            raise ValueError("TigTally needs an index built with locate=True")
        self.index = index
        self._L = index._L
        self._h = self._L.mtg_tig_tally_create(index._h)
        self.device_bytes = int(self._L.mtg_tig_tally_device_bytes(self._h))
        self.windows = int(self._L.mtg_tig_tally_windows(self._h))

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._L.mtg_tig_tally_free(h)

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _open(self) -> None:
        """The tally open and its index open, else ValueError: before the library is asked."""
        if not self._h:
            raise ValueError("the tally is closed")
        if not self.index._h:
            raise ValueError("the index is closed")

    def add(self, seqs_or_store) -> KmerQueryResult:
        """Count the k-mers of seqs_or_store (UnitigStore, list of str, or (uint8 array, offsets); ANY bytes) that the index holds
        -> what TigIndex.query says of them."""
        self._open()
        d, o, n, keep, off, kmers, valid, found = self.index._probe_inputs(seqs_or_store)
        if isinstance(seqs_or_store, UnitigStore):
            self._L.mtg_tig_tally_add_store(self._h, seqs_or_store.handle, _ptr(kmers), _ptr(valid), _ptr(found))
        else:
            self._L.mtg_tig_tally_add(self._h, d, o, n, _ptr(kmers), _ptr(valid), _ptr(found))
        del keep
        return KmerQueryResult(self.index.info.k, off, kmers, valid, found)

    def coverage(self, seqs_or_store, per_window: bool = False) -> KmerCoverageResult:
        """KmerTally.coverage's answer: query()'s counts per record of seqs_or_store plus, over its found windows, how many were
        added at least once, the sum and the largest of their tallies; per_window: also the tally at every window start."""
        self._open()
        d, o, n, keep, off, kmers, valid, found = self.index._probe_inputs(seqs_or_store)
        covered, total, hi = (np.zeros(n, np.uint64) for _ in range(3))
        pw = np.zeros(int(off[n]), np.uint64) if per_window else None
        outs = (_ptr(kmers), _ptr(valid), _ptr(found), _ptr(covered), _ptr(total), _ptr(hi), _ptr(pw) if per_window else None)
        if isinstance(seqs_or_store, UnitigStore):
            self._L.mtg_tig_tally_coverage_store(self._h, seqs_or_store.handle, *outs)
        else:
            self._L.mtg_tig_tally_coverage(self._h, d, o, n, *outs)
        del keep
        return KmerCoverageResult(self.index.info.k, off, kmers, valid, found, covered, total, hi, pw)

    def counters(self) -> np.ndarray:
        """The counters in window order of the indexed sequences (uint64, `windows` of them)."""
        self._open()
        out = np.zeros(self.windows, np.uint64)
        self._L.mtg_tig_tally_counters(self._h, _ptr(out))
        return out

    def reset(self) -> None:
        """Every counter zero again."""
        self._open()
        self._L.mtg_tig_tally_reset(self._h)


def last_tig_tally_times() -> dict:
    """Phases of the last TigTally.add or TigTally.coverage on this thread, in ms (HIP events around the kernels; upload and download
    by the host clock): probe = the locate pass with the fill of the hit array, pass2 = the add or the gather over the hits."""
    out = (C.c_double * 5)()
    _lib.load().mtg_last_tig_tally_times(out)
    return dict(zip(("upload_ms", "pack_ms", "probe_ms", "pass2_ms", "download_ms"), list(out)))


@dataclass(frozen=True, eq=False)
class PseudoalignResult:
    """What Pseudoaligner.align found, per fragment (numpy uint64 arrays): kmers / valid / found as KmerIndex.query gives them, summed
    over the fragment's one or two records, and masks: bit c set iff the rule assigns colour c to the fragment. offsets: those of the
    reads (the first mates)."""

    k: int
    offsets: np.ndarray
    kmers: np.ndarray
    valid: np.ndarray
    found: np.ndarray
    masks: np.ndarray

    def colors(self, i: int) -> list[int]:
        """The colours of fragment i, ascending."""
        m = int(self.masks[i])
        return [c for c in range(MAX_COLORS) if (m >> c) & 1]


class Pseudoaligner:
    """Which colours is each read compatible with, and how many reads fall into each distinct colour set? (mtg_pseudoaligner_*,
    DESIGN.md 33). index: a coloured KmerIndex or a coloured TigIndex (TigIndex.annotated(..., colors=...)), never changed; the
    aligner keeps a reference to it, and several aligners on one index are independent. A fragment is one record, or with mates the
    pair of record r of the reads and record r of the mates. Per fragment, hits[c] = its found windows whose k-mer carries colour c
    (KmerIndex.color_hits' per_color, summed over the mates) and denom = its found windows (over="found") or its valid windows
    (over="valid"); colour c is assigned iff denom >= min_kmers, hits[c] > 0 and hits[c] * 1000 >= threshold_permille * denom, in
    integers. threshold_permille=1000 over found is the intersection of the found k-mers' colour sets. The per-colour counters stay
    on the GPU: a call brings back four words per fragment and its distinct masks. The aligner holds no device memory between calls."""

    def __init__(self, index, threshold_permille: int = 1000, over: str = "found", min_kmers: int = 1):
        self._h = None
        if not isinstance(index, (KmerIndex, TigIndex)):
            raise TypeError("Pseudoaligner aligns on a KmerIndex or a TigIndex")
        if not index._h:
            raise ValueError("the index is closed")
        if not index.colored:
            raise ValueError("Pseudoaligner needs an index built with colors")
        if isinstance(threshold_permille, bool) or not isinstance(threshold_permille, (int, np.integer)) or not 1 <= threshold_permille <= 1000:
            raise ValueError(f"threshold_permille must be an integer in 1..1000, not {threshold_permille!r}")
        if over not in ("found", "valid"):
            raise ValueError(f"over must be 'found' or 'valid', not {over!r}")
        if isinstance(min_kmers, bool) or not isinstance(min_kmers, (int, np.integer)) or not 1 <= min_kmers < 1 << 64:
            raise ValueError(f"min_kmers must be an integer >= 1, not {min_kmers!r}")
        self.index = index
        self.n_colors = index.n_colors
        self.threshold_permille, self.over, self.min_kmers = int(threshold_permille), over, int(min_kmers)
        self._L = index._L
        params = (C.c_uint64 * 3)(self.threshold_permille, int(over == "valid"), self.min_kmers)
        create = self._L.mtg_pseudoaligner_create if isinstance(index, KmerIndex) else self._L.mtg_pseudoaligner_create_tig
        self._h = create(index._h, C.cast(params, C.c_void_p))

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._L.mtg_pseudoaligner_free(h)

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _open(self) -> None:
        """The aligner open and its index open, else ValueError: before the library is asked."""
        if not self._h:
            raise ValueError("the aligner is closed")
        if not self.index._h:
            raise ValueError("the index is closed")

    def align(self, seqs_or_store, mates=None) -> PseudoalignResult:
        """One fragment per record of seqs_or_store (UnitigStore, list of str, or (uint8 array, offsets); ANY bytes); mates: the
        second mates in the same order, as many records. The fragments take the next ordinals of the aligner."""
        self._open()
        d, o, n, keep, off, kmers, valid, found = self.index._probe_inputs(seqs_or_store)
        masks = np.zeros(n, np.uint64)
        md = mo = keep_m = None
        if mates is not None:
            md, mo, mn, keep_m = _sequence_arrays(mates)
            if mn != n:
                raise ValueError(f"{n} reads and {mn} mates: the mates pair with the reads record by record")
            if md is None:  # (mates without a base: the library tells the mates from the two pointers)
                keep_m = (keep_m, np.zeros(1, np.uint8))
                md = _ptr(keep_m[1])
        outs = (_ptr(kmers), _ptr(valid), _ptr(found), _ptr(masks))
        if isinstance(seqs_or_store, UnitigStore) and (mates is None or isinstance(mates, UnitigStore)):
            self._L.mtg_pseudoaligner_align_store(self._h, seqs_or_store.handle, None if mates is None else mates.handle, *outs)
        else:
            self._L.mtg_pseudoaligner_align(self._h, d, o, n, md, mo, *outs)
        del keep, keep_m
        return PseudoalignResult(self.index.info.k, off, kmers, valid, found, masks)

    def classes(self) -> dict:
        """The equivalence classes since creation or reset(), ordered by their first fragment: {"mask", "carriers" (the colours in
        the mask), "fragments" (the fragments with exactly that mask), "first" (the smallest ordinal of one)} as uint64 arrays."""
        self._open()
        ptrs = [C.c_void_p() for _ in range(3)]
        n = int(self._L.mtg_pseudoaligner_classes(self._h, *(C.byref(p) for p in ptrs)))
        mask, fragments, first = [_taken(n, p, np.uint64) for p in ptrs]
        for p in ptrs:
            self._L.mtg_free(p)
        carriers = np.array([bin(int(m)).count("1") for m in mask], np.uint64)
        return {"mask": mask, "carriers": carriers, "fragments": fragments, "first": first}

    @property
    def totals(self) -> dict:
        """Since creation or reset(): fragments, eligible (denom >= min_kmers), assigned (a colour at least), ambiguous (two at least)."""
        self._open()
        out = (C.c_uint64 * 4)()
        self._L.mtg_pseudoaligner_totals(self._h, out)
        return dict(zip(("fragments", "eligible", "assigned", "ambiguous"), (int(x) for x in out)))

    @property
    def color_reads(self):
        """(assigned[n_colors], unique[n_colors]): the fragments whose mask has the colour, and those whose mask is that colour alone."""
        cl = self.classes()
        assigned, unique = np.zeros(self.n_colors, np.uint64), np.zeros(self.n_colors, np.uint64)
        for m, f in zip(cl["mask"], cl["fragments"]):
            m = int(m)
            for c in range(self.n_colors):
                if (m >> c) & 1:
                    assigned[c] += f
                    if m == 1 << c:
                        unique[c] += f
        return assigned, unique

    def reset(self) -> None:
        """No class, every total zero, the next fragment has the ordinal 0."""
        self._open()
        self._L.mtg_pseudoaligner_reset(self._h)


def last_pseudoalign_times() -> dict:
    """Phases of the last Pseudoaligner.align on this thread, in ms (HIP events around the kernels; upload and download by the host
    clock): probe = the colour probe of the reads and of the mates, mask = the counters to one mask per fragment, dictionary = the
    distinct masks and their compaction."""
    out = (C.c_double * 6)()
    _lib.load().mtg_last_pseudoalign_times(out)
    return dict(zip(("upload_ms", "pack_ms", "probe_ms", "mask_ms", "dictionary_ms", "download_ms"), list(out)))


@dataclass(frozen=True, eq=False)
class CorrectionResult:
    """What ReadCorrector.correct found. Per record (numpy uint64 arrays): kmers / valid / found as KmerIndex.query gives them on the
    input, found_after = found on the corrected text, candidates = the positions of round 1 that no present window covers, ambiguous
    = the positions of the last round with two equally good bases, corrected = the positions substituted. Per call: positions (uint64
    indices into the concatenated records, ascending) and bases (uint8: the letters A C G T) of the substitutions, and
    round_corrected[8], the substitutions made in each round."""

    k: int
    offsets: np.ndarray
    kmers: np.ndarray
    valid: np.ndarray
    found: np.ndarray
    found_after: np.ndarray
    candidates: np.ndarray
    ambiguous: np.ndarray
    corrected: np.ndarray
    positions: np.ndarray
    bases: np.ndarray
    round_corrected: np.ndarray

    def record_of(self, i: int) -> int:
        """The record that holds substitution i."""
        return int(np.searchsorted(self.offsets, self.positions[i], side="right")) - 1

    def apply(self, seqs) -> list:
        """The records (a list of str, as they were given to correct) with the substitutions made; a replacement takes the case of
        the letter it replaces."""
        lengths = [len(s) for s in seqs]
        if len(lengths) + 1 != len(self.offsets) or (np.cumsum([0] + lengths) != self.offsets).any():
            raise ValueError("apply() takes the records that were corrected")
        text = np.frombuffer("".join(seqs).encode("latin-1"), np.uint8).copy()
        text[self.positions.astype(np.int64)] = patched_bytes(text[self.positions.astype(np.int64)], self.bases)
        whole = text.tobytes().decode("latin-1")
        return [whole[int(a):int(b)] for a, b in zip(self.offsets[:-1], self.offsets[1:])]


def patched_bytes(old: np.ndarray, bases: np.ndarray) -> np.ndarray:
    """The upper-case letters `bases` in the case of the letters `old` they replace (uint8 arrays of one length)."""
    lower = (old >= ord("a")) & (old <= ord("z"))
    return np.where(lower, bases | np.uint8(0x20), bases).astype(np.uint8)


class ReadCorrector:
    """Puts right the substitution errors of reads against the k-mers of a KmerIndex (mtg_kmer_index_correct). The
    index's k-mer set is the solid set; the index is never changed, the corrector keeps a reference to it, and several correctors on
    one index are independent. In each of `rounds` rounds (1..8) a base that no present window covers is a candidate; each of the
    three other bases is tried, and the one that makes the most covering windows solid -- at least min(min_solid, the valid windows
    that cover it), and more than either other base -- replaces it. All decisions of a round read the round's input. The search runs
    on the GPU, one wave per candidate; only six words per record and the substitutions come back. The corrector holds no device
    memory between calls."""

    def __init__(self, index, min_solid: int = 4, rounds: int = 2):
        self._open_flag = False
        if isinstance(index, TigIndex):
            raise TypeError("ReadCorrector corrects on a KmerIndex: the sparse minimizer index is not served")
        if not isinstance(index, KmerIndex):
            raise TypeError("ReadCorrector corrects on a KmerIndex")
        if not index._h:
            raise ValueError("the index is closed")
        if isinstance(min_solid, bool) or not isinstance(min_solid, (int, np.integer)) or not 1 <= min_solid < 1 << 32:
            raise ValueError(f"min_solid must be an integer >= 1, not {min_solid!r}")
        if isinstance(rounds, bool) or not isinstance(rounds, (int, np.integer)) or not 1 <= rounds <= 8:
            raise ValueError(f"rounds must be an integer in 1..8, not {rounds!r}")
        self.index = index
        self.min_solid, self.rounds = int(min_solid), int(rounds)
        self._L = index._L
        self._open_flag = True

    def close(self) -> None:
        self._open_flag = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def correct(self, seqs_or_store) -> CorrectionResult:
        """seqs_or_store: UnitigStore, list of str, or (uint8 array, offsets); ANY bytes. The input is not changed: the result
        names the substitutions, and CorrectionResult.apply makes them."""
        if not getattr(self, "_open_flag", False):
            raise ValueError("the corrector is closed")
        d, o, n, keep, off, kmers, valid, found = self.index._probe_inputs(seqs_or_store)
        found_after, candidates, ambiguous, corrected = (np.zeros(n, np.uint64) for _ in range(4))
        params = (C.c_uint32 * 2)(self.min_solid, self.rounds)
        positions, bases, count = C.c_void_p(), C.c_void_p(), C.c_uint64(0)
        per_round = (C.c_uint64 * 8)()
        outs = (_ptr(kmers), _ptr(valid), _ptr(found), _ptr(found_after), _ptr(candidates), _ptr(ambiguous), _ptr(corrected),
                C.byref(positions), C.byref(bases), C.byref(count), per_round)
        if isinstance(seqs_or_store, UnitigStore):
            self._L.mtg_kmer_index_correct_store(self.index._h, seqs_or_store.handle, C.cast(params, C.c_void_p), *outs)
        else:
            self._L.mtg_kmer_index_correct(self.index._h, d, o, n, C.cast(params, C.c_void_p), *outs)
        del keep
        m = int(count.value)
        pos, letters = _taken(m, positions, np.uint64), _taken(m, bases, np.uint8)
        for p in (positions, bases):
            self._L.mtg_free(p)
        return CorrectionResult(self.index.info.k, off, kmers, valid, found, found_after, candidates, ambiguous, corrected, pos, letters,
                                np.array(list(per_round), np.uint64))


def last_kmer_correct_times() -> dict:
    """Phases of the last ReadCorrector.correct on this thread, in ms (HIP events around the kernels; upload, download and total by
    the host clock): query = every query pass, flag = the candidate bits and their compaction, evaluate = the search over the
    substitutions, apply = the compaction of the accepted ones and the patch of the packed text."""
    out = (C.c_double * 8)()
    _lib.load().mtg_last_kmer_correct_times(out)
    return dict(zip(("upload_ms", "pack_ms", "query_ms", "flag_ms", "evaluate_ms", "apply_ms", "download_ms", "total_ms"), list(out)))


def last_tig_locate_times() -> dict:
    """Phases of the last TigIndex.locate on this thread, in ms (HIP events around the kernels; the upload by the host clock): probe =
    the lookup of every window with its position and strand (with the fill of the hit array), runs = folding the hits into runs."""
    out = (C.c_double * 4)()
    _lib.load().mtg_last_tig_locate_times(out)
    return dict(zip(("upload_ms", "pack_ms", "probe_ms", "runs_ms"), list(out)))


def last_kmer_thread_times(tig: bool = False) -> dict:
    """Phases of the last KmerIndex.thread (tig=True: TigIndex.thread) on this thread, in ms (HIP events around the kernels; the upload
    by the host clock): probe and runs as locate() reports them, walks = the walk stage (flag, scans, emit, compaction)."""
    out = (C.c_double * 5)()
    L = _lib.load()
    (L.mtg_last_tig_thread_times if tig else L.mtg_last_kmer_thread_times)(out)
    return dict(zip(("upload_ms", "pack_ms", "probe_ms", "runs_ms", "walks_ms"), list(out)))


def last_tig_index_times() -> dict:
    """Phases of the last TigIndex build and the last query of one on this thread, in ms (HIP events around the kernels; uploads by
    the host clock)."""
    out = (C.c_double * 8)()
    _lib.load().mtg_last_tig_index_times(out)
    return dict(zip(("build_upload_ms", "build_pack_ms", "build_anchors_ms", "build_directory_ms", "build_heavy_ms", "query_upload_ms",
                     "query_pack_ms", "query_probe_ms"), list(out)))


def last_kmer_color_times() -> dict:
    """In ms: stats = the colour statistics kernel of the last compact_unitigs_colored on this thread (HIP events); the phases of the
    last KmerIndex.color_hits (HIP events around the kernels; upload and download by the host clock)."""
    out = (C.c_double * 5)()
    _lib.load().mtg_last_kmer_color_times(out)
    return dict(zip(("stats_ms", "upload_ms", "pack_ms", "probe_ms", "download_ms"), list(out)))


def last_kmer_query_times() -> dict:
    """Phases of the last KmerIndex build and the last query on this thread, in ms (HIP events around the kernels; uploads by the
    host clock)."""
    out = (C.c_double * 6)()
    _lib.load().mtg_last_kmer_query_times(out)
    return dict(zip(("build_upload_ms", "build_pack_ms", "build_insert_ms", "query_upload_ms", "query_pack_ms", "query_probe_ms"), list(out)))


def last_kmer_locate_times() -> dict:
    """Phases of the last KmerIndex.locate on this thread, in ms (HIP events around the kernels; the upload by the host clock):
    probe = the lookup of every window with its position and strand, runs = folding the hits into runs."""
    out = (C.c_double * 4)()
    _lib.load().mtg_last_kmer_locate_times(out)
    return dict(zip(("upload_ms", "pack_ms", "probe_ms", "runs_ms"), list(out)))


def last_kmer_abundance_times() -> dict:
    """Phases of the last KmerIndex.abundance on this thread, in ms (HIP events around the kernels; upload and download by the host
    clock)."""
    out = (C.c_double * 4)()
    _lib.load().mtg_last_kmer_abundance_times(out)
    return dict(zip(("upload_ms", "pack_ms", "probe_ms", "download_ms"), list(out)))


def kmer_at(seqs, record: int, pos: int, k: int) -> str:
    """The window a witness of a KmerComparison names, as text (upper case)."""
    if isinstance(seqs, UnitigStore):
        L = _lib.load()
        off = np.ctypeslib.as_array(C.cast(L.mtg_unitigs_offsets(seqs.handle), C.POINTER(C.c_uint64)), shape=(len(seqs) + 1,))
        return C.string_at(L.mtg_unitigs_data(seqs.handle) + int(off[record]) + pos, k).decode().upper()
    if isinstance(seqs, tuple):
        start = int(seqs[1][record]) + pos
        return np.asarray(seqs[0][start:start + k], np.uint8).tobytes().decode().upper()
    return seqs[record][pos:pos + k].upper()


def compute_tigs_to_fasta_file(graph: Bigraph, store: UnitigStore, algorithm: int, k: int, path: Optional[str],
                               compression_level: int = 6, device_id: int = 0, gfa_path: Optional[str] = None,
                               gfa_header: Optional[str] = None, duplication_bitvector_path: Optional[str] = None,
                               configuration: Optional[GreedytigAlgorithmConfiguration] = None, verify: bool = False,
                               verify_against=None) -> dict:
    """compute (3 = eulertigs, 5 = greedy matchtigs) + spell + write FASTA and/or GFA, all inside the library. verify: the result
    gains "verify", the KmerComparison of `store` with the FASTA file as written and read back (read_sequences) or, without a FASTA
    path, with the tigs spelled to FASTA in memory on the same GPU. verify_against: the sequences to compare with instead of `store`
    (the `--seq-in` route: the input as given, so that the check covers the compaction too)."""
    import time

    L = _lib.load()
    t0 = time.perf_counter()
    c = (configuration or GreedytigAlgorithmConfiguration(1, k, device_ids=(device_id,))).to_c()
    w = L.mtg_compute_tigs_cfg(graph.handle, algorithm, C.byref(c))
    t1 = time.perf_counter()
    n_tigs = int(L.mtg_walks_count(w))
    nbytes = gbytes = 0
    spell_dev = int(c.device_ids[0])  # spell where the tigs were computed (--device / cfg.device_ids)
    if path:
        nbytes = int(L.mtg_write_tigs_text_file_device(graph.handle, w, k, store.handle, 0, None, str(path).encode(), compression_level, spell_dev))
    if gfa_path:
        gbytes = int(L.mtg_write_tigs_text_file_device(graph.handle, w, k, store.handle, 1, gfa_header.encode() if gfa_header else None,
                                                       str(gfa_path).encode(), compression_level, spell_dev))
    if duplication_bitvector_path:
        L.mtg_write_tigs_duplication_bitvector_file(graph.handle, w, str(duplication_bitvector_path).encode())
    t2 = time.perf_counter()
    cmp = None
    if verify:
        if path:
            tigs = read_sequences(path)
        else:
            lim, ed, text = C.c_void_p(), C.c_void_p(), C.c_void_p()
            L.mtg_walks_data(w, C.byref(lim), C.byref(ed))
            n = L.mtg_write_walks_text_device(graph.handle, n_tigs, lim, ed, k, C.cast(L.mtg_unitigs_data(store.handle), C.c_char_p),
                                              L.mtg_unitigs_offsets(store.handle), 0, None, spell_dev, C.byref(text))
            fa = C.string_at(text, n)
            L.mtg_free(text)
            tigs = fa.decode().split("\n")[1::2]
        cmp = compare_kmer_sets(store if verify_against is None else verify_against, tigs, k, spell_dev)
    L.mtg_walks_free(w)
    r = {"tigs": n_tigs, "fasta_bytes": nbytes, "gfa_bytes": gbytes, "compute_s": t1 - t0, "write_s": t2 - t1}
    if verify:
        r["verify"], r["verify_tigs"], r["verify_s"] = cmp, tigs, time.perf_counter() - t2
    return r


def write_duplication_bitvector(graph: Bigraph, tigs) -> bytes:
    """implementation/mod.rs:668-702 through the C-ABI: per tig a line of '1' (original k-mer) / '0' (duplicate) characters."""
    L = _lib.load()
    if isinstance(tigs, tuple):
        lim, ed = np.ascontiguousarray(tigs[0], np.uint64), np.ascontiguousarray(tigs[1], np.uint32)
    else:
        ed = np.fromiter((e for t in tigs for e in t), dtype=np.uint32)
        lim = np.cumsum([len(t) for t in tigs], dtype=np.uint64) if len(tigs) else np.zeros(0, np.uint64)
    out = C.c_void_p()
    n = L.mtg_write_duplication_bitvector(graph.handle, len(lim), _ptr(lim) if len(lim) else None, _ptr(ed) if len(ed) else None,
                                          C.byref(out))
    data = C.string_at(out, n)
    L.mtg_free(out)
    return data


def write_walks_gfa(graph: Bigraph, tigs, unitigs: Sequence[str], k: int, header: Optional[str] = None) -> bytes:
    """bin.rs:667-818 through the C-ABI: GFA1 text (header line, then one S record per tig)."""
    return write_walks_fasta(graph, tigs, unitigs, k, _gfa=True, _header=header)


def write_walks_text_device(graph: Bigraph, tigs, unitigs, k: int, gfa: bool = False, header: Optional[str] = None,
                            device_id: int = 0) -> bytes:
    """The same text spelled on the GPU (mtg_write_walks_text_device). unitigs: list of str, or (uint8 array, offsets)."""
    L = _lib.load()
    if isinstance(tigs, tuple):
        lim, ed = np.ascontiguousarray(tigs[0], np.uint64), np.ascontiguousarray(tigs[1], np.uint32)
    else:
        ed = np.fromiter((e for t in tigs for e in t), dtype=np.uint32)
        lim = np.cumsum([len(t) for t in tigs], dtype=np.uint64) if len(tigs) else np.zeros(0, np.uint64)
    if isinstance(unitigs, tuple):
        cat = np.ascontiguousarray(unitigs[0], np.uint8).tobytes()
        off = np.ascontiguousarray(unitigs[1], np.uint64)
    else:
        cat = "".join(unitigs).encode()
        off = np.zeros(len(unitigs) + 1, np.uint64)
        off[1:] = np.cumsum([len(u) for u in unitigs])
    out = C.c_void_p()
    n = L.mtg_write_walks_text_device(graph.handle, len(lim), _ptr(lim) if len(lim) else None, _ptr(ed) if len(ed) else None, k, cat,
                                      _ptr(off), 1 if gfa else 0, header.encode() if header else None, device_id, C.byref(out))
    data = C.string_at(out, n)
    L.mtg_free(out)
    return data


def unitig_links(graph: Bigraph, device_id: int = 0):
    """The links of the unitig graph, made on the GPU (mtg_unitig_links) -> (link_off, link_to). Oriented unitig o --
    (u,+) is 2u, (u,-) is 2u + 1, the edge ids of every graph -- links to the edges link_to[link_off[o]:link_off[o + 1]], ascending:
    o' is among them iff from(edge o') == to(edge o). link_off: uint64[2U + 1], link_to: uint32[links]. Only the original edges
    count, so dummy edges a tig computation left in the graph change nothing."""
    L = _lib.load()
    off, to = C.c_void_p(), C.c_void_p()
    n = int(L.mtg_unitig_links(graph.handle, device_id, C.byref(off), C.byref(to)))
    n_off = graph.original_edge_count() + 1
    link_off = np.ctypeslib.as_array(C.cast(off, C.POINTER(C.c_uint64)), shape=(n_off,)).copy()
    link_to = np.ctypeslib.as_array(C.cast(to, C.POINTER(C.c_uint32)), shape=(n,)).copy() if n else np.zeros(0, np.uint32)
    L.mtg_free(off)
    L.mtg_free(to)
    return link_off, link_to


def write_unitig_graph(graph: Bigraph, store, k: int, path: Optional[str] = None, gfa: bool = False, kc=None,
                       compression_level: int = 6, device_id: int = 0):
    """The unitigs with their links as BCALM2/GGCAT FASTA (`>u LN:i: KC:i: km:f: L:+:v:-`) or, with gfa, as GFA1 (`S` and `L`
    lines), the whole text made on the GPU (mtg_write_unitig_graph_text / _file). store: the unitigs of `graph` as a
    UnitigStore, a list of str, or (uint8 array, offsets). kc: the abundance sum of every unitig (Abundance.unitig_sums), or None for
    its number of k-mers. Without a path the bytes are returned; with one the file is written (`.gz`: gzip at compression_level) and
    {"unitigs", "links", "bytes"} returned."""
    L = _lib.load()
    data, off, n, keep = _sequence_arrays(store)
    if kc is not None:
        kc = np.ascontiguousarray(kc, dtype=np.uint64)
        if len(kc) != n:
            raise ValueError(f"{len(kc)} abundance sums for {n} unitigs")
    if path is None:
        out = C.c_void_p()
        nbytes = int(L.mtg_write_unitig_graph_text(graph.handle, data, off, n, k, _ptr(kc) if kc is not None and n else None,
                                                   1 if gfa else 0, device_id, C.byref(out)))
        text = C.string_at(out, nbytes)
        L.mtg_free(out)
        del keep
        return text
    nbytes = int(L.mtg_write_unitig_graph_file(graph.handle, data, off, n, k, _ptr(kc) if kc is not None and n else None,
                                               1 if gfa else 0, device_id, str(path).encode(), compression_level))
    del keep
    return {"unitigs": n, "links": int(last_unitig_graph_times()["links"]), "bytes": nbytes}


def last_unitig_graph_times() -> dict:
    """Of the last unitig_links / write_unitig_graph on this thread: the uploads and the download by the host clock, the link kernels,
    the scans of the text and the text kernel by HIP events (ms); the links, the bytes of the text, the bytes the text kernel must
    move at the least and the peak of the device arena's live bytes."""
    out = (C.c_double * 9)()
    _lib.load().mtg_last_unitig_graph_times(out)
    names = ("upload_ms", "link_ms", "text_prepare_ms", "text_ms", "download_ms", "links", "bytes", "text_min_bytes", "peak_arena_bytes")
    return {name: (float(v) if name.endswith("_ms") else int(v)) for name, v in zip(names, out)}


@dataclass(frozen=True, eq=False)
class Components:
    """The connected components of a unitig graph over its links (mtg_unitig_components), in exact integers.
    component_of[u]: the component of unitig u; components are numbered by their smallest unitig, ascending. Per component:
    first_unitig, unitigs, kmers, abundance (the sum of the caller's per-unitig sums, or of the k-mers), links (the link entries whose
    source orientation lies in it), dead_ends (orientations without a link), irregular (orientations whose number of links is not 1)."""

    component_of: np.ndarray  # uint32[unitigs]
    first_unitig: np.ndarray  # uint32[components]
    unitigs: np.ndarray       # uint32[components]
    kmers: np.ndarray         # uint64[components]
    abundance: np.ndarray     # uint64[components]
    links: np.ndarray         # uint64[components]
    dead_ends: np.ndarray     # uint32[components]
    irregular: np.ndarray     # uint32[components]

    def __len__(self) -> int:
        return len(self.first_unitig)

    @property
    def circular(self) -> np.ndarray:
        """bool[components]: every orientation has exactly one link, so the component is a closed ring of unitigs."""
        return self.irregular == 0

    def describe(self) -> str:
        if len(self) == 0:
            return "0 components"
        big = int(np.argmax(self.kmers))  # (ties: the first)
        total = int(self.kmers.sum())
        share = 100.0 * int(self.kmers[big]) / total if total else 0.0
        return (f"{len(self)} components, largest {int(self.unitigs[big])} unitigs / {int(self.kmers[big])} k-mers ({share:.1f} % of the k-mers), "
                f"{int((self.unitigs == 1).sum())} of one unitig, {int(self.circular.sum())} circular")


def _unitig_kmers(store, k: int) -> np.ndarray:
    """The number of k-mers of every record of a UnitigStore, a list of str or (uint8 array, offsets)."""
    if isinstance(store, UnitigStore):
        lengths = np.diff(store.arrays()[1])
    elif isinstance(store, tuple):
        lengths = np.diff(np.asarray(store[1], np.uint64))
    else:
        lengths = np.array([len(s) for s in store], np.uint64)
    if len(lengths) and int(lengths.min()) < k:
        raise ValueError(f"a unitig is shorter than k = {k}")
    return (lengths.astype(np.uint64) - np.uint64(k - 1)).astype(np.uint64)


def unitig_components(graph: Bigraph, store_or_kmers, k: Optional[int] = None, kc=None, device_id: int = 0) -> Components:
    """The connected components of the unitig graph over its links, labelled and measured on the GPU (mtg_unitig_components,
    DESIGN.md 27). store_or_kmers: with k, the unitigs of `graph` as a UnitigStore, a list of str or (uint8 array, offsets); without
    k, the number of k-mers of every unitig as a plain array (graphs built from links, without sequences). kc: the abundance sum of
    every unitig (Abundance.unitig_sums), or None for its number of k-mers. Only the original edges count, so dummy edges a tig
    computation left in the graph change nothing."""
    L = _lib.load()
    U = graph.original_edge_count() // 2
    kmers = np.ascontiguousarray(store_or_kmers, dtype=np.uint64) if k is None else _unitig_kmers(store_or_kmers, k)
    if kmers.ndim != 1 or len(kmers) != U:
        raise ValueError(f"{len(kmers)} k-mer counts for a graph of {U} unitigs")
    if kc is not None:
        kc = np.ascontiguousarray(kc, dtype=np.uint64)
        if len(kc) != U:
            raise ValueError(f"{len(kc)} abundance sums for {U} unitigs")
    of, arrays = C.c_void_p(), _lib.MtgComponentArrays()
    n = int(L.mtg_unitig_components(graph.handle, _ptr(kmers) if U else None, _ptr(kc) if kc is not None and U else None, device_id,
                                    C.byref(of), C.byref(arrays)))

    def take(p, ctype, dtype, count):
        a = np.ctypeslib.as_array(C.cast(p, C.POINTER(ctype)), shape=(count,)).copy() if count else np.zeros(0, dtype)
        L.mtg_free(p)
        return a

    component_of = take(of, C.c_uint32, np.uint32, U)
    fields = {name: take(getattr(arrays, name), C.c_uint64 if name in ("kmers", "abundance", "links") else C.c_uint32,
                         np.uint64 if name in ("kmers", "abundance", "links") else np.uint32, n) for name, _ in arrays._fields_}
    return Components(component_of=component_of, **fields)


def select_components(graph: Bigraph, store, k: int, min_kmers: int, kc=None, device_id: int = 0):
    """The unitigs of the components that have at least min_kmers k-mers -> (store of the kept records in their order, keep (bool per
    unitig), Components of the graph as it was). A UnitigStore gives a UnitigStore (mtg_unitigs_select); a list of str gives a list,
    (uint8 array, offsets) gives such a pair. Links exist only inside a component, so the kept unitigs stay maximal, and the
    components of the graph of the kept store (Bigraph.from_sequences) are the kept ones, renumbered in their order."""
    if min_kmers < 1:
        raise ValueError("min_kmers must be >= 1")
    comps = unitig_components(graph, store, k, kc, device_id)
    keep = (comps.kmers >= np.uint64(min_kmers))[comps.component_of] if len(comps) else np.zeros(0, bool)
    if isinstance(store, UnitigStore):
        out = C.c_void_p()
        flags = np.ascontiguousarray(keep, dtype=np.uint8)
        _lib.load().mtg_unitigs_select(store.handle, _ptr(flags) if len(flags) else None, C.byref(out))
        kept = UnitigStore(out.value)
    elif isinstance(store, tuple):
        data, off = np.asarray(store[0], np.uint8), np.asarray(store[1], np.uint64)
        lengths = np.diff(off)
        new_off = np.zeros(int(keep.sum()) + 1, np.uint64)
        new_off[1:] = np.cumsum(lengths[keep])
        kept = (data[np.repeat(keep, lengths.astype(np.int64))], new_off)
    else:
        kept = [s for s, f in zip(store, keep.tolist()) if f]
    return kept, keep, comps


def last_unitig_components_times() -> dict:
    """Of the last unitig_components / select_components on this thread: the uploads and the download by the host clock, the label
    kernels and the statistics kernel by HIP events (ms); the components, the unitigs and the peak of the device arena's live bytes;
    and the parts of label_ms: rep / degree, the unions, flatten + scan + numbers."""
    out = (C.c_double * 10)()
    _lib.load().mtg_last_unitig_components_times(out)
    names = ("upload_ms", "label_ms", "stats_ms", "download_ms", "components", "unitigs", "peak_arena_bytes", "rep_ms", "union_ms", "flatten_ms")
    return {name: (float(v) if name.endswith("_ms") else int(v)) for name, v in zip(names, out)}


_BUBBLE_KINDS = ("snp", "mnp", "ins", "del", "complex", "identical")
_COMPLEMENT = str.maketrans("ACGTacgt", "TGCATGCA")


def _record_reader(store):
    """record(u) -> the upper-case string of record u of a UnitigStore, a list of str or (uint8 array, offsets)."""
    if isinstance(store, UnitigStore):
        store = store.arrays()
    if isinstance(store, tuple):
        data, off = np.asarray(store[0], np.uint8), np.asarray(store[1], np.uint64)
        return lambda u: data[int(off[u]):int(off[u + 1])].tobytes().decode().upper()
    return lambda u: store[u].upper()


@dataclass(frozen=True, eq=False)
class UnitigBubbles:
    """The bubbles of a unitig graph as variant calls (mtg_unitig_bubbles). The arms of bubble b are the entries
    arm_off[b] .. arm_off[b + 1] - 1: the reference arm (the largest mean abundance, then the smallest unitig) first, the others
    ascending by unitig; bubbles are numbered by their smallest unitig. arm_strand: 0 (+) where the arm runs the way the reference
    arm's record is written, 1 (-) where its reverse complement does. prefix / suffix / differences describe an arm's allele against
    the reference arm's record R: ref = R[prefix : len(R) - suffix], alt the same slice of the arm as oriented; all 0 for arm 0.
    carried[arm, c]: the arm's k-mers that colour c carries (None without masks)."""

    arm_off: np.ndarray        # uint64[bubbles + 1]
    arm_unitig: np.ndarray     # uint32[arms]
    arm_strand: np.ndarray     # uint8[arms]
    arm_kmers: np.ndarray      # uint32[arms]
    arm_abundance: np.ndarray  # uint64[arms]
    prefix: np.ndarray         # uint32[arms]
    suffix: np.ndarray         # uint32[arms]
    differences: np.ndarray    # uint32[arms]
    k: int                     # the k-mer length of the call: an arm has arm_kmers + k - 1 bases
    carried: Optional[np.ndarray] = None  # uint32[arms, n_colors]

    def __len__(self) -> int:
        return len(self.arm_off) - 1

    def _ref_arm(self) -> np.ndarray:
        """The index of arm 0 of every arm's bubble."""
        return np.repeat(self.arm_off[:-1], np.diff(self.arm_off).astype(np.int64)).astype(np.int64)

    def allele_lengths(self):
        """(len(ref), len(alt)) of every arm as int64 arrays; both 0 for arm 0."""
        first = self._ref_arm()
        cut = self.prefix.astype(np.int64) + self.suffix.astype(np.int64) - (self.k - 1)
        n_ref, n_alt = self.arm_kmers[first].astype(np.int64) - cut, self.arm_kmers.astype(np.int64) - cut
        is_ref = first == np.arange(len(first))
        n_ref[is_ref] = 0
        n_alt[is_ref] = 0
        return n_ref, n_alt

    def kinds(self) -> list:
        """The kind of every arm: "ref" for arm 0, else snp (both alleles one base), mnp (equal lengths above 1), del (alt empty),
        ins (ref empty), complex (anything else), or identical (both empty: a repeated record)."""
        first = self._ref_arm()
        n_ref, n_alt = self.allele_lengths()
        out = []
        for a, (r, v) in enumerate(zip(n_ref.tolist(), n_alt.tolist())):
            if a == first[a]:
                out.append("ref")
            elif r == 0 and v == 0:
                out.append("identical")
            elif v == 0:
                out.append("del")
            elif r == 0:
                out.append("ins")
            elif r == v:
                out.append("snp" if r == 1 else "mnp")
            else:
                out.append("complex")
        return out

    def alleles(self, store) -> list:
        """(ref, alt) of every arm as strings, read from the unitigs the call was made on (a UnitigStore, a list of str or (uint8
        array, offsets)); an empty allele is "", arm 0 gets (".", ".")."""
        record = _record_reader(store)
        first = self._ref_arm()
        out = []
        for a in range(len(self.arm_unitig)):
            if a == first[a]:
                out.append((".", "."))
                continue
            ref, arm = record(int(self.arm_unitig[first[a]])), record(int(self.arm_unitig[a]))
            if self.arm_strand[a]:
                arm = arm.translate(_COMPLEMENT)[::-1]
            p, s = int(self.prefix[a]), int(self.suffix[a])
            out.append((ref[p:len(ref) - s], arm[p:len(arm) - s]))
        return out

    def tsv(self, store, k: int, names=None) -> str:
        """`--bubbles-out`: one row per arm -- bubble, arm, unitig, strand, kmers, abundance, mean (abundance / kmers with one
        decimal, rounded half up in integers), type, pos (0-based in the reference arm's record), ref, alt, differences -- and one
        column per colour with `carried` (headed by names, or c0, c1, ...). Arm 0 has `ref . . . 0`; an empty allele is `-`."""
        if k != self.k:
            raise ValueError(f"k = {k}, but the bubbles were called with k = {self.k}")
        n_colors = 0 if self.carried is None else self.carried.shape[1]
        if names is not None and len(names) != n_colors:
            raise ValueError(f"{len(names)} names for {n_colors} colours")
        head = ["bubble", "arm", "unitig", "strand", "kmers", "abundance", "mean", "type", "pos", "ref", "alt", "differences"]
        head += list(names) if names is not None else [f"c{c}" for c in range(n_colors)]
        rows = ["\t".join(head) + "\n"]
        kinds, alleles = self.kinds(), self.alleles(store)
        bubble_of = np.repeat(np.arange(len(self)), np.diff(self.arm_off).astype(np.int64))
        first = self._ref_arm()
        for a in range(len(self.arm_unitig)):
            n, kc = int(self.arm_kmers[a]), int(self.arm_abundance[a])
            t = (10 * kc + n // 2) // n
            ref, alt = alleles[a]
            pos = "." if kinds[a] == "ref" else str(int(self.prefix[a]))
            row = [int(bubble_of[a]), a - int(first[a]), int(self.arm_unitig[a]), "-" if self.arm_strand[a] else "+", n, kc, f"{t // 10}.{t % 10}",
                   kinds[a], pos, ref or "-", alt or "-", int(self.differences[a])]
            row += self.carried[a].tolist() if n_colors else []
            rows.append("\t".join(str(x) for x in row) + "\n")
        return "".join(rows)

    def describe(self) -> str:
        kinds = self.kinds()
        n = {name: kinds.count(name) for name in _BUBBLE_KINDS}
        largest = int(np.diff(self.arm_off).max()) if len(self) else 0
        return (f"{len(self)} bubbles, {len(self.arm_unitig)} arms: {n['snp']} snp, {n['mnp']} mnp, {n['ins']} ins, {n['del']} del, "
                f"{n['complex']} complex; the largest has {largest} arms")


def unitig_bubbles(graph: Bigraph, store, k: int, max_arm_kmers: int, kc=None, kmer_colors=None, n_colors: int = 0,
                   device_id: int = 0) -> UnitigBubbles:
    """The bubbles of the unitig graph -- two or more unitigs of fewer than max_arm_kmers k-mers between the same two nodes -- with
    their alleles, found and described on the GPU (mtg_unitig_bubbles). store: the unitigs of `graph` as a UnitigStore,
    a list of str or (uint8 array, offsets). kc: the abundance sum of every unitig (Abundance.unitig_sums), or None for its number of
    k-mers. kmer_colors: the mask of every k-mer in window order of the store (Colors.kmer_colors) with n_colors in 1..64, or None.
    Only the original edges count, so dummy edges a tig computation left in the graph change nothing."""
    L = _lib.load()
    data, off, n, keep = _sequence_arrays(store)
    U = graph.original_edge_count() // 2
    if n != U:
        raise ValueError(f"{n} sequences for a graph of {U} unitigs")
    kmers = _unitig_kmers(store, k)
    if max_arm_kmers < 0:
        raise ValueError("max_arm_kmers must be >= 0")
    if kc is not None:
        kc = np.ascontiguousarray(kc, dtype=np.uint64)
        if kc.ndim != 1 or len(kc) != U:
            raise ValueError(f"{len(kc)} abundance sums for {U} unitigs")
    if kmer_colors is not None:
        if not 1 <= n_colors <= MAX_COLORS:
            raise ValueError(f"n_colors must be in 1..{MAX_COLORS}")
        kmer_colors = np.ascontiguousarray(kmer_colors, dtype=np.uint64)
        if kmer_colors.ndim != 1 or len(kmer_colors) != int(kmers.sum()):
            raise ValueError(f"{len(kmer_colors)} colour masks for {int(kmers.sum())} k-mers")
    arrays = _lib.MtgUnitigBubbleArrays()
    B = int(L.mtg_unitig_bubbles(graph.handle, data, off, n, k, max_arm_kmers, _ptr(kc) if kc is not None and U else None,
                                 _ptr(kmer_colors) if kmer_colors is not None and len(kmer_colors) else None,
                                 n_colors if kmer_colors is not None else 0, device_id, C.byref(arrays)))
    del keep

    def take(p, ctype, dtype, count):
        a = np.ctypeslib.as_array(C.cast(p, C.POINTER(ctype)), shape=(count,)).copy() if count else np.zeros(0, dtype)
        L.mtg_free(p)
        return a

    arm_off = take(arrays.arm_off, C.c_uint64, np.uint64, B + 1)
    A = int(arm_off[B])
    u32 = {name: take(getattr(arrays, name), C.c_uint32, np.uint32, A) for name in ("arm_unitig", "arm_kmers", "prefix", "suffix", "differences")}
    carried = None
    if kmer_colors is not None:
        carried = take(arrays.carried, C.c_uint32, np.uint32, A * n_colors).reshape(A, n_colors)
    return UnitigBubbles(arm_off=arm_off, arm_strand=take(arrays.arm_strand, C.c_uint8, np.uint8, A),
                         arm_abundance=take(arrays.arm_abundance, C.c_uint64, np.uint64, A), k=k, carried=carried, **u32)


def last_unitig_bubbles_times() -> dict:
    """Of the last unitig_bubbles on this thread: the uploads (with the pack) and the download by the host clock, keys + group +
    number, the allele kernel and the carrier kernel by HIP events (ms); the bubbles, the arms and the peak of the device arena's
    live bytes."""
    out = (C.c_double * 8)()
    _lib.load().mtg_last_unitig_bubbles_times(out)
    names = ("upload_ms", "group_ms", "allele_ms", "carrier_ms", "download_ms", "bubbles", "arms", "peak_arena_bytes")
    return {name: (float(v) if name.endswith("_ms") else int(v)) for name, v in zip(names, out)}


def last_spell_kernel() -> dict:
    L = _lib.load()
    return {"ms": float(L.mtg_last_spell_kernel_ms()), "bytes": int(L.mtg_last_spell_bytes())}


def write_walks_fasta(graph: Bigraph, tigs, unitigs: Sequence[str], k: int, _gfa: bool = False,
                      _header: Optional[str] = None) -> bytes:
    """bin.rs:466-606 through the C-ABI: tigs = list of edge-id lists (or (limits, edges) numpy pair) -> FASTA bytes."""
    L = _lib.load()
    if isinstance(tigs, tuple):
        lim, ed = np.ascontiguousarray(tigs[0], np.uint64), np.ascontiguousarray(tigs[1], np.uint32)
    else:
        ed = np.fromiter((e for t in tigs for e in t), dtype=np.uint32)
        lim = np.cumsum([len(t) for t in tigs], dtype=np.uint64) if len(tigs) else np.zeros(0, np.uint64)
    cat = "".join(unitigs).encode()
    off = np.zeros(len(unitigs) + 1, np.uint64)
    off[1:] = np.cumsum([len(u) for u in unitigs])
    out = C.c_void_p()
    if _gfa:
        n = L.mtg_write_walks_gfa(graph.handle, len(lim), _ptr(lim) if len(lim) else None, _ptr(ed) if len(ed) else None, k,
                                  cat, _ptr(off), _header.encode() if _header else None, C.byref(out))
    else:
        n = L.mtg_write_walks_fasta(graph.handle, len(lim), _ptr(lim) if len(lim) else None, _ptr(ed) if len(ed) else None, k,
                                    cat, _ptr(off), C.byref(out))
    data = C.string_at(out, n)
    L.mtg_free(out)
    return data


def last_euler_kernel_ms() -> float:
    return float(_lib.load().mtg_last_euler_kernel_ms())


def last_phase_seconds() -> dict:
    L = _lib.load()
    a = (C.c_double * 8)()
    L.mtg_last_phase_seconds(a)
    names = ["device_build", "classify", "sssp", "download", "replay", "eulerise", "euler", "cut"]
    return {n: float(a[i]) for i, n in enumerate(names)}


# ---- the reference's C-ABI, driven from Python exactly like a C caller would (clib.rs) ----------
def clib_compute_tigs(unitig_weights, links, tig_algorithm: int, threads: int, k: int, matching_file_prefix: str = "",
                      matcher_path: str = ""):
    """matchtigs_initialise_graph -> merge_nodes* -> build_graph -> compute_tigs. Returns
    (n_tigs, tigs_edge_out, tigs_insert_out, tigs_out_limits) trimmed to their used lengths."""
    L = _lib.load()
    w = np.ascontiguousarray(unitig_weights, dtype=np.uint64)
    u = len(w)
    data = L.matchtigs_initialise_graph(u)
    for (ua, sa, ub, sb) in links:
        L.matchtigs_merge_nodes(data, int(ua), bool(sa), int(ub), bool(sb))
    L.matchtigs_build_graph(data, _ptr(w))
    edge_count = 2 * u  # clib.rs:332-348: outputs sized by the edge count before dummies
    eo = np.zeros(max(2 * edge_count, 1), np.int64)
    io = np.zeros(max(2 * edge_count, 1), np.uint64)
    lo = np.zeros(max(edge_count, 1), np.uint64)
    n = int(L.matchtigs_compute_tigs(data, tig_algorithm, threads, k, str(matching_file_prefix).encode(),
                                     str(matcher_path).encode(), _ptr(eo), _ptr(io), _ptr(lo)))
    total = int(lo[n - 1]) if n else 0
    return n, eo[:total].copy(), io[:total].copy(), lo[:n].copy()
