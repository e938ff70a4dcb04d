"""Independent restatement of the unitig component contract, with dicts and lists, on top of the link lists of
unitig_links_ref.py, for the tests of api.unitig_components, api.select_components and `--components-out` /
`--unitig-components-out` / `--min-component-kmers`.

Unitigs u and v are adjacent iff some orientation of u links to some orientation of v (link rule of DESIGN.md 26); a component is a
class of the reflexive, symmetric, transitive closure: connectivity over LINKS, not over shared nodes. Components are numbered by
their smallest unitig, ascending. Per component: first_unitig, unitigs, kmers, abundance (the sum of kc, or of the k-mers), links
(the link entries whose source orientation lies in it), dead_ends (orientations with no link), irregular (orientations whose number
of links is not 1); circular iff irregular == 0.
"""
from __future__ import annotations

import unitig_links_ref as LR

FIELDS = ("first_unitig", "unitigs", "kmers", "abundance", "links", "dead_ends", "irregular")


def components_of_links(link_off, link_to, kmers, kc=None):
    """-> {"component_of": [...], field: [...] for every field of FIELDS}, from link lists over 2U oriented unitigs."""
    U = (len(link_off) - 1) // 2
    assert len(kmers) == U
    neighbours = [set() for _ in range(U)]
    for o in range(2 * U):
        for j in range(int(link_off[o]), int(link_off[o + 1])):
            v = int(link_to[j]) >> 1
            neighbours[o >> 1].add(v)
            neighbours[v].add(o >> 1)
    component_of = [-1] * U
    out = {f: [] for f in FIELDS}
    for u in range(U):  # ascending: the next unlabelled unitig is the smallest of a new component
        if component_of[u] >= 0:
            continue
        c = len(out["first_unitig"])
        component_of[u] = c
        todo, members = [u], []
        while todo:
            x = todo.pop()
            members.append(x)
            for v in neighbours[x]:
                if component_of[v] < 0:
                    component_of[v] = c
                    todo.append(v)
        degree = [int(link_off[o + 1]) - int(link_off[o]) for x in members for o in (2 * x, 2 * x + 1)]
        out["first_unitig"].append(u)
        out["unitigs"].append(len(members))
        out["kmers"].append(sum(int(kmers[x]) for x in members))
        out["abundance"].append(sum(int((kmers if kc is None else kc)[x]) for x in members))
        out["links"].append(sum(degree))
        out["dead_ends"].append(sum(1 for d in degree if d == 0))
        out["irregular"].append(sum(1 for d in degree if d != 1))
    out["component_of"] = component_of
    return out


def components_of_sequences(seqs, k: int, kc=None):
    off, to = LR.links_of_sequences(seqs, k)
    return components_of_links(off, to, [len(s) - k + 1 for s in seqs], kc)


def components_of_graph(edge_from, edge_to, n_original_edges: int, kmers, kc=None):
    off, to = LR.links_of_graph(edge_from, edge_to, n_original_edges)
    return components_of_links(off, to, kmers, kc)


def circular(comps):
    return [x == 0 for x in comps["irregular"]]


def keep_of(comps, min_kmers: int):
    """The filter: one bool per unitig, true for the unitigs of the components with at least min_kmers k-mers."""
    return [comps["kmers"][c] >= min_kmers for c in comps["component_of"]]


def filtered_sequences(seqs, k: int, min_kmers: int):
    """-> (kept records in their old order, keep). What is reported after a filter is what a call on these records returns."""
    keep = keep_of(components_of_sequences(seqs, k), min_kmers)
    return [s for s, f in zip(seqs, keep) if f], keep


def components_tsv(comps, k: int) -> str:
    """`--components-out`: bases = kmers + (k - 1) unitigs; mean = abundance / kmers with one decimal, rounded half up in integers."""
    rows = ["component\tfirst_unitig\tunitigs\tkmers\tbases\tabundance\tmean\tlinks\tdead_ends\tcircular\n"]
    for c in range(len(comps["first_unitig"])):
        n, m, a = comps["unitigs"][c], comps["kmers"][c], comps["abundance"][c]
        rows.append(f"{c}\t{comps['first_unitig'][c]}\t{n}\t{m}\t{m + (k - 1) * n}\t{a}\t{LR.km_text(a, m)}\t{comps['links'][c]}\t"
                    f"{comps['dead_ends'][c]}\t{1 if comps['irregular'][c] == 0 else 0}\n")
    return "".join(rows)


# Hand cases at k = 5: those of unitig_links_ref.HAND plus two that only the components tell apart.
HAND = {name: recs for name, (recs, _, _) in LR.HAND.items()}
# Both records start with ACCG and nothing ends in it; their mirrors end in CGGT and nothing starts with it: one shared node, no link.
HAND["siblings"] = ["ACCGTTA", "ACCGAGC"]
# fork's first three records (one component), a lone k-mer, and a ring with a tail: 4+ = ACCGTACCG links to itself and to 5+ = ACCGTTAGC.
HAND["mixed"] = ["TTGACGCA", "CGCAATTC", "CGCACTTG", "GGACC", "ACCGTACCG", "ACCGTTAGC"]
