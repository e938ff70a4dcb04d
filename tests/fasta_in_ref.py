"""Independent restatements of the plain-FASTA (`--fa-in`) graph contract, for the tests of that input route.

Occurrence o = 2u is the first k-1 bases of record u, o = 2u + 1 its last k-1 bases. A class {x, rc(x)} takes ids in increasing
order of its creator (smallest o): two consecutive ids, the creator's orientation first, or one for a palindrome. Edge 2u runs
node(P_u) -> node(S_u), edge 2u + 1 mirror(node(S_u)) -> mirror(node(P_u)), weight len + 1 - k.
"""
from __future__ import annotations

import numpy as np

_COMP = str.maketrans("ACGT", "TGCA")


def revcomp(s: str) -> str:
    return s.translate(_COMP)[::-1]


def graph_dict(seqs: list[str], k: int) -> dict:
    """Rules 1-4 with a dict, any k: the arrays mtg_graph_export gives."""
    L = k - 1
    ids: dict[str, int] = {}
    mirror: list[int] = []

    def node(x: str) -> int:
        if x not in ids:
            r, base = revcomp(x), len(mirror)
            if x == r:
                ids[x] = base
                mirror.append(base)
            else:
                ids[x], ids[r] = base, base + 1
                mirror.extend([base + 1, base])
        return ids[x]

    U = len(seqs)
    ef, et = np.zeros(2 * U, np.uint32), np.zeros(2 * U, np.uint32)
    for u, s in enumerate(seqs):  # occurrences in o order: the first sight of a class is its creator
        s = s.upper()
        p, q = node(s[:L]), node(s[len(s) - L:])
        ef[2 * u], et[2 * u] = p, q
        ef[2 * u + 1], et[2 * u + 1] = mirror[q], mirror[p]
    w = np.repeat(np.array([len(s) + 1 - k for s in seqs], np.uint64), 2)
    return {"mirror": np.array(mirror, np.uint32), "edge_from": ef, "edge_to": et, "edge_weight": w,
            "edge_unitig": np.repeat(np.arange(U, dtype=np.uint64), 2),
            "edge_forwards": np.tile(np.array([1, 0], np.uint8), U)}


def graph_np(seq: np.ndarray, off: np.ndarray, k: int) -> dict:
    """The same for k - 1 <= 31, vectorised: (k-1)-mers as 2-bit codes, classes by np.unique (first occurrence = creator)."""
    L = k - 1
    assert 1 <= L <= 31
    lut = np.full(256, 255, np.uint8)
    for i, c in enumerate(b"ACGT"):
        lut[c] = i
    for i, c in enumerate(b"acgt"):
        lut[c] = i
    b = lut[seq]
    assert not (b == 255).any()
    o64 = off.astype(np.int64)
    U = len(o64) - 1
    starts = np.empty(2 * U, np.int64)
    starts[0::2], starts[1::2] = o64[:-1], o64[1:] - L
    fwd, rc = np.zeros(2 * U, np.uint64), np.zeros(2 * U, np.uint64)
    for j in range(L):
        c = b[starts + j].astype(np.uint64)
        fwd = (fwd << np.uint64(2)) | c
        rc |= (np.uint64(3) - c) << np.uint64(2 * j)
    flip, pal = rc < fwd, rc == fwd
    _, first, inv = np.unique(np.where(flip, rc, fwd), return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    order = np.argsort(first, kind="stable")            # classes in creator order
    cnt = np.where(pal[first[order]], 1, 2).astype(np.int64)
    base = np.empty(len(first), np.int64)
    base[order] = np.cumsum(cnt) - cnt
    creator = first[inv]
    same = flip == flip[creator]
    node = base[inv] + np.where(pal, 0, np.where(same, 0, 1))
    mir = base[inv] + np.where(pal, 0, np.where(same, 1, 0))
    mirror = np.zeros(int(cnt.sum()), np.uint32)
    cpal = pal[first]
    mirror[base] = np.where(cpal, base, base + 1)
    mirror[base[~cpal] + 1] = base[~cpal]
    ef, et = np.empty(2 * U, np.uint32), np.empty(2 * U, np.uint32)
    ef[0::2], et[0::2] = node[0::2], node[1::2]
    ef[1::2], et[1::2] = mir[1::2], mir[0::2]
    return {"mirror": mirror, "edge_from": ef, "edge_to": et,
            "edge_weight": np.repeat((np.diff(o64) + 1 - k).astype(np.uint64), 2),
            "edge_unitig": np.repeat(np.arange(U, dtype=np.uint64), 2),
            "edge_forwards": np.tile(np.array([1, 0], np.uint8), U)}


def fasta_text(seqs: list[str], width: int = 0, headers=None) -> str:
    """FASTA text of the records; width > 0 wraps the sequences over several lines."""
    out = []
    for i, s in enumerate(seqs):
        out.append(f">{headers[i] if headers else i}\n")
        if width:
            out.extend(s[j:j + width] + "\n" for j in range(0, len(s), width))
        else:
            out.append(s + "\n")
    return "".join(out)


def end_partitions_agree(link: dict, fa: dict) -> tuple[bool, int]:
    """Compares the node partition of unitig ends of the link route (`link`) with the --fa-in one (`fa`), both from
    mtg_graph_export. Returns (ok, predicted link-route node count): ok iff every pair of ends the link route joins is joined by
    fa too, and every fa node that holds ends of several link-route nodes holds only out-ends or only in-ends, one link-route node
    per end. The prediction counts, per fa node, 1 if it holds both kinds of end, else its number of ends."""
    E = len(fa["edge_from"])
    ln = np.concatenate([link["edge_from"][:E], link["edge_to"][:E]]).astype(np.int64)
    fn = np.concatenate([fa["edge_from"][:E], fa["edge_to"][:E]]).astype(np.int64)
    is_out = np.concatenate([np.ones(E, bool), np.zeros(E, bool)])
    # refinement: one fa node per link node
    Vl, Vf = len(link["mirror"]), len(fa["mirror"])
    f_of_l = np.full(Vl, -1, np.int64)
    f_of_l[ln] = fn
    if not np.array_equal(f_of_l[ln], fn):
        return False, -1
    ends = np.bincount(fn, minlength=Vf)
    outs = np.bincount(fn, weights=is_out, minlength=Vf).astype(np.int64)
    mixed = (outs > 0) & (outs < ends)
    # self-mirror fa nodes: an out-end there is the in-end of the mirror edge at the same node
    predicted = np.where(mixed, 1, ends)
    pairs = np.unique(np.stack([fn, ln], 1), axis=0)
    l_per_f = np.bincount(pairs[:, 0], minlength=Vf)
    ok = bool(np.array_equal(l_per_f[ends > 0], predicted[ends > 0]))
    return ok, int(predicted.sum())
