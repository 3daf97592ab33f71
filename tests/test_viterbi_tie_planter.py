"""The near-tie planter of tests/helpers.py (plant_viterbi_ties), checked against the oracle before any device sees its
batches: every planted decision comes out as constructed, moving the losing candidate's planted weight slightly ahead flips
it, and the two candidate paths of a separated tie run apart across a composed chunk entry."""
import numpy as np
import pytest

from tests.helpers import plant_viterbi_ties

TRANS2 = np.array([[2.669891070463728, -2.599571900486168], [-2.6019205422130995, 2.5683226020688488]])


def _flip(w, trans, case, cptr):
    """labels of the case's contig with the losing candidate moved ahead by 1e-9 of its magnitude"""
    from oracle import crf_oracle as orc

    g0, g1 = int(cptr[case["contig"]]), int(cptr[case["contig"] + 1])
    st = w[g0:g1].copy()
    row = st[case["planted"] - g0]
    row[case["loser"]] += 1e-9 * max(1.0, float(np.abs(row).max()) * (g1 - g0))
    y, _ = orc.viterbi_seq(st, trans)
    return y, g0


@pytest.mark.parametrize("L, lengths", [
    (2, [9, 0, 200, 1, 2049, 3, 50000, 0, 300000, 7]),
    (3, [9, 0, 200, 1, 2049, 3, 50000]),
    (5, [9, 200, 0, 2049, 1, 64]),
    (8, [9, 200, 2049, 0, 5000, 3]),
    (13, [9, 200, 0, 2049, 2, 66]),
    (32, [9, 200, 0, 2049, 1, 130]),
])
def test_planted_ties_decide_as_constructed(L, lengths):
    from oracle import crf_oracle as orc

    rng = np.random.default_rng(31 + L)
    trans = TRANS2 if L == 2 else rng.normal(0.0, 1.5, size=(L, L))
    w, cptr, gptr, attr, cases = plant_viterbi_ties(rng, lengths, L, trans)
    ey, _ = orc.viterbi(w, trans, cptr, gptr, attr)
    kinds = {(c["kind"], c["ulps"]) for c in cases}
    assert {("end", k) for k in (0, 1, -1, 2, -2)} <= kinds and {("interior", k) for k in (0, 1, -1, 2, -2)} <= kinds
    if L >= 3:
        assert any(abs(c["pair"][0] - c["pair"][1]) > 1 for c in cases)
    # every contig with genes has its end tie; long contigs have their block boundary more than 64 blocks in
    assert sum(c["kind"] == "end" for c in cases) == sum(1 for T in lengths if T)
    if 300000 in lengths:
        c = lengths.index(300000)
        assert any(x["contig"] == c and x["gene"] - cptr[c] > 64 * 2048 for x in cases if x["kind"] == "interior")
    # separated ties: at every chunk boundary t = 128 q of the longer contigs, the two candidates' paths split before the
    # entry of the 64-gene chunk that holds gene t - 1 (so the vector entering the chunk of gene t is composed from chunk
    # products over paths of their own), and the pair is sometimes non-adjacent
    sep = [c for c in cases if c["kind"] == "separated"]
    assert len(sep) >= 5 and {c["ulps"] for c in sep} == {0, 1, -1, 2, -2}
    for c in sep:
        rel = c["gene"] - cptr[c["contig"]]
        entry = (rel // 64) * 64
        assert entry >= 64 and c["merge"] - cptr[c["contig"]] < entry, c
    if 300000 in lengths:
        c = lengths.index(300000)
        assert any(x["contig"] == c and x["gene"] - cptr[c] > 64 * 2048 for x in sep)
    for case in cases:
        assert ey[case["gene"]] == case["winner"], case
        if case["kind"] != "end":
            assert ey[case["gene"] + 1] == case["j"], case
        y, g0 = _flip(w, trans, case, cptr)
        assert y[case["gene"] - g0] == case["loser"], case
