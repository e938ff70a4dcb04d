"""Tig spelling restated: walks -> FASTA / GFA bytes, written from the reference's writers (bin.rs:466-606 write_walks_fasta,
:667-818 write_walks_gfa) and from nothing else -- no import from pyref.py, the oracle or the library, so that the speller kernel
(spell_device.hip) and the host speller (spell.cpp) are each held to a third reading of the same lines.

The graph is reduced to what the writers read of it: edge e < n_orig is ORIGINAL, its sequence is unitig e >> 1, forwards iff e is
even (clib.rs:239-248: biedge b is unitig b, the even edge the forwards one); edge e >= n_orig is a DUMMY of weight
dummy_weights[(e - n_orig) >> 1] (a dummy biedge and its mirror share the weight) and has no sequence.

The reference keeps its sequences in a 2-bit DnaAlphabet store: whatever case went in, upper-case ACGT comes out, and the
restatement does the same. Where the reference would panic (an empty walk :487, a dummy first edge :489, k - 1 - weight below zero
:536, a slice past the unitig :541 / :572) the restatement fails an assertion."""

_COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}


def spell_ref(k, seqs, n_orig, dummy_weights, walks, gfa=False, header=None) -> bytes:
    """k: k-mer length; seqs: the unitigs (str, any case of ACGT); n_orig: number of original edges (2 per unitig); dummy_weights:
    weight of dummy biedge i (edges n_orig + 2 i, n_orig + 2 i + 1); walks: iterable of sequences of edge ids (Python ints); gfa: GFA1 records
    behind a header line (`header`, or "H\\tKL:Z:{k}" :688-692) instead of FASTA records."""
    assert k >= 1 and n_orig == 2 * len(seqs)
    seqs = [s.upper() for s in seqs]
    texts = {}  # (edge, offset) -> what the edge adds, so that a million one-edge walks over few unitigs stay quick

    def text_of(edge, offset):
        seq = seqs[edge >> 1]
        assert 0 <= offset <= len(seq), f"offset {offset} outside unitig {edge >> 1} of length {len(seq)}"
        if edge % 2 == 0:
            return seq[offset:]                                                        # :539-566
        return "".join(_COMPLEMENT[c] for c in reversed(seq[:len(seq) - offset]))     # :567-596: revcomp(seq[0 .. len - offset])

    out = []
    if gfa:
        out.append((header if header is not None else f"H\tKL:Z:{k}") + "\n")  # :688-693
    for i, walk in enumerate(walks):
        assert len(walk) > 0, f"walk {i} is empty"                     # walk.first().unwrap(), :487
        previous = walk[0]
        assert previous < n_orig, f"walk {i} starts with a dummy edge"  # :489
        out.append(f"S\t{i + 1}\t" if gfa else f">{i + 1}\n")           # :704 / :492
        key = (previous, 0)                                             # :497-501: the first edge in full
        if key not in texts:
            texts[key] = text_of(*key)
        out.append(texts[key])
        for current in walk[1:]:
            if current >= n_orig:                                       # :519-531: a dummy edge writes nothing
                previous = current
                continue
            if previous < n_orig:
                key = (current, k - 1)                                  # :534
            else:
                key = (current, k - 1 - int(dummy_weights[(previous - n_orig) >> 1]))  # :536
            if key not in texts:
                texts[key] = text_of(*key)
            out.append(texts[key])
            previous = current
        out.append("\n")                                                # :601
    return "".join(out).encode()


def walks_of(limits, edges):
    """The (limits, edges) array form of a walk set (exclusive ends, flat edge ids) as a list of lists."""
    out, b = [], 0
    ed = [int(e) for e in edges]
    for lim in limits:
        out.append(ed[b:int(lim)])
        b = int(lim)
    return out
