"""The quad-tree selection's case table (tests/octree_cases.py) on the CPU: its encoding against the oracle's detection order and the FAST kernel's cell rule,
the two CPU references -- the literal C list code of oracle/orb.c (sso_distribute_octtree) and pyref's port -- against each other on every case and every
level geometry tests/test_gpu_orb_octree.py uses, and, from pyref's trace, that the table reaches every path of the selection.  The conditions of the last
test are conditions on the INPUTS: the seeds in octree_cases.table were chosen until the references alone satisfy them."""
import numpy as np
import pytest

import octree_cases as K
import pyref

_cache = {}


def results(oracle):
    """per (context, level, case name): (level geometry, case, selection, trace), both references computed once and held to each other"""
    if not _cache:
        for ci, (w, h, nl, sc, nf, _) in enumerate(K.CONTEXTS):
            g = K.geometry(w, h, nl, sc, nf)
            for l in K.planted_levels(nl):
                L = g["levels"][l]
                for c in K.table(L):
                    tr = {}
                    a, b = K.reference(L, c, None, tr), K.reference(L, c, oracle)
                    assert np.array_equal(a, b), "context %d level %d case %s: pyref selects %d, oracle/orb.c %d; first difference at %s" % (
                        ci, l, c.name, len(a), len(b), next((i for i in range(min(len(a), len(b))) if tuple(a[i]) != tuple(b[i])), min(len(a), len(b))))
                    assert (ci, l, c.name) not in _cache
                    _cache[(ci, l, c.name)] = (L, c, a, tr)
    return _cache


def test_references_agree_on_every_case(oracle):
    r = results(oracle)
    assert len(r) >= 8 * 30
    for (ci, l, name), (L, c, sel, tr) in r.items():
        assert len(sel) == tr["final"] <= L.sel_cap, (ci, l, name)          # the kernel's slots (N + 3) hold every reference selection
        assert len({tuple(v) for v in sel.tolist()}) == len(sel)


def test_trace_does_not_change_the_result(oracle):
    L = K.geometry(*K.CONTEXTS[0][:3], K.CONTEXTS[0][3], K.CONTEXTS[0][4])["levels"][0]
    for c in K.table(L)[3:22]:
        s = [tuple(int(v) for v in row) for row in K.survivors(L, c)]
        assert pyref.distribute_octtree(s, *K.octree_args(L)) == pyref.distribute_octtree(s, *K.octree_args(L), trace={})


def test_encoding_is_the_oracles_detection_order_and_the_kernels_cell_rule(oracle):
    # the oracle lists a level's candidates cells row-major, raster inside a cell: the rank words of that list must rise strictly
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (480, 640), dtype=np.uint8)
    g = K.geometry(640, 480, 8, 1.2, 1000)
    _, _, stages = oracle.orb_extract(img, nfeatures=1000, want_stages=True)
    for L, st in zip(g["levels"], stages):
        c = st["cand"].astype(np.int64)
        assert len(c) > 100
        x, y = c[:, 0] - L.minB, c[:, 1] - L.minB
        assert x.min() >= 3 and x.max() < L.W - 3 and y.min() >= 3 and y.max() < L.H - 3
        rw = K.rank_word(L, x, y).astype(np.int64)
        assert (np.diff(rw) > 0).all()
        assert ((rw >> 14) < L.nCols * L.nRows).all() and ((rw & 127) >= 3).all() and ((rw & 127) < L.wCell + 3).all() and (((rw >> 7) & 127) < L.hCell + 3).all()
    # fast_tile takes the cell of a position by a reciprocal multiplication: __umulhi(xr - 3, ceil(2^32 / wCell))
    for (w, h, nl, sc, nf, _) in K.CONTEXTS:
        for L in K.geometry(w, h, nl, sc, nf)["levels"]:
            for n, cell in ((L.W, L.wCell), (L.H, L.hCell)):
                v = np.arange(0, n - 6, dtype=np.uint64)
                assert np.array_equal((v * np.uint64(((1 << 32) + cell - 1) // cell)) >> np.uint64(32), v // np.uint64(cell))


def test_expected_selections(oracle):
    r = results(oracle)
    for (ci, l, name), (L, c, sel, tr) in r.items():
        ns = len(K.survivors(L, c))
        if name == "cluster":
            assert ns == 100 and len(sel) == 1 and tr["finish1"] == "no growth" and tr["passes1"] == 1
        if name == "all_dropped":
            assert len(c.cands) == 300 and ns == 0 and len(sel) == 0
        if name in ("exact_n", "exact_n_uneven"):                   # list + 3 * expandable == N before the last pass: no mode switch, N nodes after it
            assert tr["finish1"] == ">= N" and tr["passes2"] == 0 and len(sel) == L.nfeat
            assert (name == "exact_n") == (ns == L.nfeat)
        if name in ("random(1)", "random(2)", "random(3)"):
            assert len(sel) == ns
        if name == "thresholds":                                    # both kinds of cell, and keys on both sides of each threshold
            S, cm = c.cands[:, 2] + 1, c.cellmax[K.cell_of(L, c.cands[:, 0], c.cands[:, 1])]
            assert (cm > K.INI).any() and (cm == K.INI).any() and ((cm < K.INI) & (cm > K.MIN)).any()
            for s in (K.MIN, K.MIN + 1, K.INI, K.INI + 1):
                assert (S == s).any()
            assert 0 < ns < len(c.cands)
    # the 10 x 10 corner block and the sparse case of the level with N = 217
    assert len(r[(0, 0, "sparse(100)")][2]) == 99 and r[(0, 0, "sparse(100)")][3]["finish1"] == "no growth"


def test_table_reaches_every_path(oracle):
    r = results(oracle)
    tr = [(k, v[0], v[3], len(K.survivors(v[0], v[1]))) for k, v in r.items()]

    def some(pred):
        return [k for k, L, t, ns in tr if pred(L, t, ns)]

    assert some(lambda L, t, ns: t["finish1"] == ">= N")
    assert some(lambda L, t, ns: t["finish1"] == "no growth" and 1 < t["final"] < ns)       # fewer nodes than keys, nothing left that grows
    assert some(lambda L, t, ns: t["finish1"] == "second phase" and t["passes2"] > 1)
    assert some(lambda L, t, ns: t["broke"] > 0)
    assert some(lambda L, t, ns: t["finish2"] == "no growth" and t["final"] < L.nfeat)
    assert some(lambda L, t, ns: t["finish2"] == ">= N" and t["broke"] == 0)                # ... and the second phase's stop at the very end of a pass
    for extra in (0, 1, 2):
        assert some(lambda L, t, ns: t["passes2"] > 0 and t["final"] == L.nfeat + extra), extra
    assert some(lambda L, t, ns: t["seq_decided"] > 0) and some(lambda L, t, ns: t["tied_best"] > 0)
    assert some(lambda L, t, ns: ns == 0) and some(lambda L, t, ns: ns == 1)
    assert some(lambda L, t, ns: 1 < ns <= K.OT_KCAP) and some(lambda L, t, ns: ns > K.OT_KCAP)
    # per context: both node-id storage paths on level 0 wherever the level holds that many candidates, roots that are empty or start as leaves where nIni >= 2
    for ci, (w, h, nl, sc, nf, _) in enumerate(K.CONTEXTS):
        L0 = K.geometry(w, h, nl, sc, nf)["levels"][0]
        counts = {len(v[1].cands) for k, v in r.items() if k[0] == ci and k[1] == 0}
        if L0.cand_cap > K.OT_KCAP:
            assert {2047, 2048, 2049} <= counts, ci
        assert ("roots_ends" in {k[2] for k in r if k[0] == ci and k[1] == 0}) == (L0.nIni >= 2)
    assert K.geometry(*K.CONTEXTS[1][:5])["levels"][0].nIni == 4 and K.geometry(*K.CONTEXTS[4][:5])["levels"][0].nIni == 1
    assert [K.geometry(*c[:5])["nodes"] for c in K.CONTEXTS[:3]] == [256, 512, 1024]
