"""KmerIndex's probes (api.py) without a GPU: query, locate, abundance and color_hits refuse a closed index first, and an open one
that was not built for them second, each with its own message -- before anything reaches the library."""
import types

import pytest

from matchtigs_amd import api

PROBES = {"query": None, "locate": "locate() needs an index built with locate=True",
          "abundance": "abundance() needs an index built with weights", "color_hits": "color_hits() needs an index built with colors"}


def _bare(handle, able):
    """An index object that never met the library: its handle is a stand-in that only close() may receive."""
    ix = api.KmerIndex.__new__(api.KmerIndex)
    ix._L = types.SimpleNamespace(mtg_kmer_index_free=lambda h: None)
    ix._h = handle
    ix.locating = ix.weighted = ix.colored = able
    ix.n_colors = 2 if able else 0
    return ix


@pytest.mark.parametrize("able", [False, True])
@pytest.mark.parametrize("probe", PROBES)
def test_a_closed_index_refuses(probe, able):
    with pytest.raises(ValueError) as e:
        getattr(_bare(None, able), probe)(["ACGT"])
    assert str(e.value) == "the index is closed"  # (also where the capability is missing: closed is checked first)


@pytest.mark.parametrize("probe", [p for p in PROBES if PROBES[p]])
def test_an_open_index_without_the_capability_keeps_its_own_message(probe):
    with pytest.raises(ValueError) as e:
        getattr(_bare(1, False), probe)(["ACGT"])
    assert str(e.value) == PROBES[probe]
