"""Independent restatement of the unitig graph output contract, with strings and dicts, for the tests of
`--unitigs-bcalm-out` / `--unitigs-gfa-out`, api.unitig_links and api.write_unitig_graph.

Unitig u has two orientations: (u,+) is edge 2u, (u,-) is edge 2u + 1. Oriented unitig o links to o' iff
from(edge o') == to(edge o); on the graphs made from sequences that is "the last k-1 bases of o are the first k-1 bases of o'". The
links of o are listed ascending by o'; a record lists those of (u,+), then those of (u,-). KC is the sum of the abundances of the
unitig's k-mers (their number where nothing was counted), km = KC / k-mers with one decimal, rounded half up in integers.
"""
from __future__ import annotations

_COMP = str.maketrans("ACGT", "TGCA")


def revcomp(s: str) -> str:
    return s.translate(_COMP)[::-1]


def oriented(seqs, o: int) -> str:
    s = seqs[o >> 1].upper()
    return revcomp(s) if o & 1 else s


def links_of_sequences(seqs, k: int):
    """-> (link_off, link_to) by the string rule: 2U + 1 offsets and the target edge ids, as lists of int."""
    starts: dict[str, list[int]] = {}
    for o in range(2 * len(seqs)):
        starts.setdefault(oriented(seqs, o)[:k - 1], []).append(o)  # (o ascends: every list is sorted)
    off, to = [0], []
    for o in range(2 * len(seqs)):
        s = oriented(seqs, o)
        to.extend(starts.get(s[len(s) - (k - 1):], []))
        off.append(len(to))
    return off, to


def links_of_graph(edge_from, edge_to, n_original_edges: int):
    """-> (link_off, link_to) by the graph rule over the original edges of an exported graph."""
    by_from: dict[int, list[int]] = {}
    for e in range(n_original_edges):
        by_from.setdefault(int(edge_from[e]), []).append(e)
    off, to = [0], []
    for o in range(n_original_edges):
        to.extend(by_from.get(int(edge_to[o]), []))
        off.append(len(to))
    return off, to


def link_tuples(link_off, link_to):
    """The links as g_seq lists them: (unitig_a, strand_a, unitig_b, strand_b), a strand True for +; in the order of the arrays."""
    out = []
    for o in range(len(link_off) - 1):
        for j in range(int(link_off[o]), int(link_off[o + 1])):
            t = int(link_to[j])
            out.append((o >> 1, not o & 1, t >> 1, not t & 1))
    return out


def km_text(kc: int, kmers: int) -> str:
    """KC / kmers with one decimal, rounded half up, in integers."""
    t = (10 * kc + kmers // 2) // kmers
    return f"{t // 10}.{t % 10}"


def _tags(s: str, k: int, kc, u: int, sep: str) -> str:
    kmers = len(s) - k + 1
    c = kmers if kc is None else int(kc[u])
    return f"{sep}LN:i:{len(s)}{sep}KC:i:{c}{sep}km:f:{km_text(c, kmers)}"


def bcalm_text(seqs, k: int, link_off, link_to, kc=None) -> str:
    out = []
    for u, s in enumerate(seqs):
        s = s.upper()
        line = f">{u}" + _tags(s, k, kc, u, " ")
        for o in (2 * u, 2 * u + 1):
            for j in range(int(link_off[o]), int(link_off[o + 1])):
                t = int(link_to[j])
                line += f" L:{'-' if o & 1 else '+'}:{t >> 1}:{'-' if t & 1 else '+'}"
        out.append(line + "\n" + s + "\n")
    return "".join(out)


def gfa_text(seqs, k: int, link_off, link_to, kc=None) -> str:
    out = [f"H\tVN:Z:1.0\tKL:Z:{k}\n"]
    for u, s in enumerate(seqs):
        s = s.upper()
        out.append(f"S\t{u}\t{s}" + _tags(s, k, kc, u, "\t") + "\n")
        for o in (2 * u, 2 * u + 1):
            for j in range(int(link_off[o]), int(link_off[o + 1])):
                t = int(link_to[j])
                out.append(f"L\t{u}\t{'-' if o & 1 else '+'}\t{t >> 1}\t{'-' if t & 1 else '+'}\t{k - 1}M\n")
    return "".join(out)


def parse_bcalm(text: str):
    """The records of a BCALM2 file as dicts: id, LN, KC, km (text), links [(a, strand_a, b, strand_b) in file order], seq."""
    lines = text.splitlines()
    recs = []
    for head, seq in zip(lines[0::2], lines[1::2]):
        f = head.split(" ")
        assert f[0][0] == ">" and f[1].startswith("LN:i:") and f[2].startswith("KC:i:") and f[3].startswith("km:f:"), head
        u = int(f[0][1:])
        links = []
        for x in f[4:]:
            tag, a, v, b = x.split(":")
            assert tag == "L" and a in "+-" and b in "+-", head
            links.append((u, a == "+", int(v), b == "+"))
        recs.append({"id": u, "LN": int(f[1][5:]), "KC": int(f[2][5:]), "km": f[3][5:], "links": links, "seq": seq})
    return recs


# Hand-derived cases, k = 5 (the nodes are 4-mers): name -> (records, link_off, link_to), worked out on paper from the oriented
# strings (the reverse complement of record u is orientation 2u + 1).
K_HAND = 5
HAND = {
    # 0+ TTGACGCA ends in CGCA; 1+, 2+, 3+ start with it. Mirrors: 1-, 2-, 3- end in TGCG, 0- = TGCGTCAA starts with it.
    "fork": (["TTGACGCA", "CGCAATTC", "CGCACTTG", "CGCAGGTT"], [0, 3, 3, 3, 4, 4, 5, 5, 6], [2, 4, 6, 1, 1, 1]),
    # 0+ and 1+ end in ACCT, 2+ = ACCTGA starts with it. Mirror: 2- = TCAGGT ends in AGGT, 0- = AGGTTCC and 1- = AGGTGAA start with it.
    "merge": (["GGAACCT", "TTCACCT", "ACCTGA"], [0, 1, 1, 2, 2, 2, 4], [4, 4, 1, 3]),
    # first 4 = last 4 = ACCG: a closed walk spelled linearly. 0- = CGGTACGGT, first 4 = last 4 = CGGT.
    "closed": (["ACCGTACCG"], [0, 1, 2], [0, 1]),
    # 0+ ends in AATT, its own reverse complement; 0- = AATTGACC starts with it: (0,+) -> (0,-), once. 0- ends in GACC: nothing.
    "hairpin": (["GGTCAATT"], [0, 1, 1], [1]),
    # the node ACGT is its own mirror: 0+ = TTGACGT and 1- = GGACGT end in it, 0- = ACGTCAA and 1+ = ACGTCC start with it.
    "palindrome": (["TTGACGT", "ACGTCC"], [0, 2, 2, 2, 4], [1, 2, 1, 2]),
    # ACCGTTAGC / GCTAACGGT: ACCG, TAGC, GCTA, CGGT are four different 4-mers.
    "isolated": (["ACCGTTAGC"], [0, 0, 0], []),
}
HAND_BCALM = {
    "fork": (">0 LN:i:8 KC:i:4 km:f:1.0 L:+:1:+ L:+:2:+ L:+:3:+\nTTGACGCA\n>1 LN:i:8 KC:i:4 km:f:1.0 L:-:0:-\nCGCAATTC\n"
             ">2 LN:i:8 KC:i:4 km:f:1.0 L:-:0:-\nCGCACTTG\n>3 LN:i:8 KC:i:4 km:f:1.0 L:-:0:-\nCGCAGGTT\n"),
    "closed": ">0 LN:i:9 KC:i:5 km:f:1.0 L:+:0:+ L:-:0:-\nACCGTACCG\n",
    "hairpin": ">0 LN:i:8 KC:i:4 km:f:1.0 L:+:0:-\nGGTCAATT\n",
    "isolated": ">0 LN:i:9 KC:i:5 km:f:1.0\nACCGTTAGC\n",
}
HAND_GFA = {
    "palindrome": ("H\tVN:Z:1.0\tKL:Z:5\nS\t0\tTTGACGT\tLN:i:7\tKC:i:3\tkm:f:1.0\nL\t0\t+\t0\t-\t4M\nL\t0\t+\t1\t+\t4M\n"
                   "S\t1\tACGTCC\tLN:i:6\tKC:i:2\tkm:f:1.0\nL\t1\t-\t0\t-\t4M\nL\t1\t-\t1\t+\t4M\n"),
}
