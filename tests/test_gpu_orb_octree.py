"""The quad-tree selection of the ORB front end (octree_kernel, K4) ALONE on PLANTED candidate lists: ssm_debug_orb_octree against the case table of
tests/octree_cases.py, whose two CPU references tests/test_octree_cases.py holds to each other.  Exact equality everywhere: the counts, the selected words IN
ORDER, the untouched slots behind them, the status word.  Every case lies on level 0 and on a middle level, in rank order, reversed and shuffled (the order
FAST's atomics append in must not matter); batches put a different case on every (frame, level), with empty levels between full ones and two frames above the
LDS capacity on one level, and must equal the same frames run alone; the oracle's own candidate lists of real frames must come out as the oracle's keypoints;
every rule the hook checks is broken once.  Contexts: the three kernel instances (NODES 256 / 512 / 1024), four root nodes, a tiny and a tall frame."""
import numpy as np
import pytest

import octree_cases as K
import pyref
from conftest import CAM, SEED

pytestmark = pytest.mark.gpu

UNWRITTEN = 0xA5A5A5A5


class Rig:
    """one context of K.CONTEXTS + the Python-side geometry + the references of what is planted (computed once per case)"""

    def __init__(self, oracle, ci):
        import semantic_slam_mapping_amd as ssm
        self.ci, self.oracle = ci, oracle
        self.w, self.h, self.nl, self.scale, self.nfeat, self.batch = K.CONTEXTS[ci]
        self.g = K.geometry(self.w, self.h, self.nl, self.scale, self.nfeat)
        self.levels = self.g["levels"]
        self.c = ssm.Context(0, width=self.w, height=self.h, orb_levels=self.nl, orb_scale=self.scale, orb_features=self.nfeat, max_batch=self.batch,
                             voxel_capacity_log2=18, camera=CAM)
        self._tables, self._refs = {}, {}

    def table(self, l):
        if l not in self._tables:
            self._tables[l] = K.table(self.levels[l])
        return self._tables[l]

    def ref(self, l, case):
        """the reference selection's packed words (the literal C list code; tests/test_octree_cases.py holds pyref's port to it)"""
        key = (l, case.name, hash(case.cands.tobytes()), hash(case.cellmax.tobytes()))
        if key not in self._refs:
            self._refs[key] = K.sel_words(self.levels[l], K.reference(self.levels[l], case, self.oracle))
        return self._refs[key]

    def plant(self, frames, want_nodeof=False):
        """frames: per frame a dict level -> (case, index array: the buffer order).  One call of the hook; returns (nsel, sel, status[, nodeof])"""
        n = len(frames)
        ncand = np.zeros((n, self.nl), np.int32); cellmax = np.zeros((n, self.g["cells_total"]), np.int32); words = []
        for f, fr in enumerate(frames):
            for l in range(self.nl):
                if l in fr:
                    case, order = fr[l]; L = self.levels[l]
                    ncand[f, l] = len(case.cands)
                    words.append(K.encode(L, case.cands[order]))
                    cellmax[f, L.cell_off:L.cell_off + L.nCols * L.nRows] = case.cellmax
        cand = np.concatenate(words) if words else np.zeros((0, 2), np.uint32)
        return self.c.debug_orb_octree(ncand, cand, cellmax, want_nodeof)

    def check(self, frames, out, what):
        nsel, sel, status = out[:3]
        assert status == 0, "%s: status %d" % (what, status)
        for f, fr in enumerate(frames):
            for l, L in enumerate(self.levels):
                got = sel[f, L.sel_off:L.sel_off + L.sel_cap]
                ref = self.ref(l, fr[l][0]) if l in fr else np.zeros(0, np.uint32)
                at = "%s: context %d frame %d level %d%s" % (what, self.ci, f, l, " case " + fr[l][0].name if l in fr else "")
                assert int(nsel[f, l]) == len(ref), "%s: nsel %d, the reference selects %d" % (at, nsel[f, l], len(ref))
                if not np.array_equal(got[:len(ref)], ref):
                    i = int(np.flatnonzero(got[:len(ref)] != ref)[0])
                    raise AssertionError("%s: selected word %d of %d is (x %d, y %d, score %d), the reference has (x %d, y %d, score %d)" % (
                        at, i, len(ref), got[i] & 4095, got[i] >> 12 & 4095, got[i] >> 24, ref[i] & 4095, ref[i] >> 12 & 4095, ref[i] >> 24))
                assert (got[len(ref):] == UNWRITTEN).all(), "%s: a slot behind nsel = %d was written" % (at, len(ref))


_rigs = {}


@pytest.fixture(scope="module")
def rig(oracle):
    def get(ci):
        if ci not in _rigs:
            _rigs[ci] = Rig(oracle, ci)
        return _rigs[ci]
    yield get
    for r in _rigs.values():
        r.c.close()
    _rigs.clear()


CI = range(len(K.CONTEXTS))


@pytest.mark.parametrize("ci", CI)
def test_geometry_query_equals_the_python_side(rig, ci):
    r = rig(ci)
    g = r.c.debug_orb_octree_geometry()
    assert len(g["levels"]) == r.nl
    for l, L in enumerate(r.levels):
        assert g["levels"][l] == {k: getattr(L, k) for k in K.GEOM_FIELDS}, l
    assert {k: g[k] for k in ("cells_total", "cand_total", "sel_total", "nodes")} == {k: r.g[k] for k in ("cells_total", "cand_total", "sel_total", "nodes")}
    assert g["nodes"] == (256, 512, 1024, 1024, 512)[ci]
    assert r.c.cap == g["sel_total"]


@pytest.mark.parametrize("ci", CI)
def test_every_case_on_level_0_and_a_middle_level_in_three_buffer_orders(rig, ci):
    r = rig(ci)
    lv = K.planted_levels(r.nl)
    names = []
    for l in lv:
        names += [c.name for c in r.table(l) if c.name not in names]
    assert len(names) >= 30
    for i, name in enumerate(names):
        first = None
        for oname in ("rank", "reversed", "shuffled"):
            fr = {}
            for l in lv:
                case = next((c for c in r.table(l) if c.name == name), None)
                if case is not None:
                    fr[l] = (case, K.orders(case, i)[oname])
            out = r.plant([fr])
            r.check([fr], out, "%s, %s order" % (name, oname))
            if first is None:
                first = out
            assert out[0].tobytes() == first[0].tobytes() and out[1].tobytes() == first[1].tobytes(), "%s: %s order differs from rank order" % (name, oname)


def _batch_frames(r):
    """a different case on every (frame, level): level 0 above the LDS capacity in every frame (5000 or 2049 candidates, other seeds than the table's), every
    third (frame, level) empty, the table's cases dealt over the rest; buffers shuffled"""
    frames = []
    for f in range(r.batch):
        fr = {}
        for l, L in enumerate(r.levels):
            if l == 0:
                case = K.random(L, 4000 + f, 5000 if f < 2 else 2049, "batch random #%d" % f)
            elif (f + l) % 3 == 1:
                continue
            else:
                t = r.table(l)
                case = t[(7 * f + 5 * l) % len(t)]
            fr[l] = (case, K.orders(case, 10 * f + l)["shuffled"])
        frames.append(fr)
    return frames


@pytest.mark.parametrize("ci", CI)
def test_batch_of_different_cases_equals_references_and_single_frames(rig, ci):
    r = rig(ci)
    frames = _batch_frames(r)
    if r.batch >= 2:                                                 # two frames above the LDS capacity on the same level: the global node ids are per frame
        assert all(len(K.survivors(r.levels[0], fr[0][0])) > K.OT_KCAP for fr in frames[:2]) and frames[0][0][0].cands.tobytes() != frames[1][0][0].cands.tobytes()
    if r.nl >= 3:
        assert any(l - 1 in fr and l not in fr and l + 1 in fr for fr in frames for l in range(1, r.nl - 1))       # an empty level between full ones
    out = r.plant(frames, want_nodeof=True)
    r.check(frames, out, "batch")
    # the global node ids: written for exactly the candidates of the (frame, level) pairs above the LDS capacity, in THAT frame's part of the scratch -- every
    # one a final node of its level or 0xFFFF (dropped) -- and nowhere else
    for f, fr in enumerate(frames):
        for l, L in enumerate(r.levels):
            ids = out[3][f, L.cand_off:L.cand_off + L.cand_cap]
            nc = len(fr[l][0].cands) if l in fr else 0
            used = nc if nc > K.OT_KCAP else 0
            assert (ids[used:] == 0xA5A5).all(), "frame %d level %d: node ids written outside the level's %d candidates" % (f, l, used)
            if used:
                case, order = fr[l]
                kept = np.isin(K.encode(L, case.cands[order])[:, 0], K.encode(L, K.survivors(L, case))[:, 0])
                assert (ids[:used][~kept] == 0xFFFF).all() and (ids[:used][kept] < int(out[0][f, l])).all(), "frame %d level %d: node ids of the global path" % (f, l)
                best = np.zeros(int(out[0][f, l]), np.int64)
                np.maximum.at(best, ids[:used][kept].astype(np.int64), case.cands[order][kept][:, 2])
                assert np.array_equal(best, out[1][f, L.sel_off:L.sel_off + len(best)].astype(np.int64) >> 24)      # every node's selected response is its keys' maximum
    for f, fr in enumerate(frames):
        one = r.plant([fr])
        r.check([fr], one, "frame %d alone" % f)
        assert one[0][0].tobytes() == out[0][f].tobytes() and one[1][0].tobytes() == out[1][f].tobytes(), "frame %d alone differs from the batch" % f


@pytest.mark.parametrize("ci", CI)
def test_oracle_candidates_of_real_frames_come_out_as_the_oracles_keypoints(rig, oracle, ci):
    r = rig(ci)
    sf = pyref.level_params(r.nfeat, r.scale, r.nl)[0]
    imgs = [("synthetic", oracle.bgr2gray(oracle.synth_frame(SEED, 2, r.w, r.h)[0])),
            ("noise", np.random.default_rng(77 + ci).integers(0, 256, (r.h, r.w), dtype=np.uint8))]
    for name, img in imgs:
        kps, _, stages = oracle.orb_extract(img, nfeatures=r.nfeat, scale=r.scale, nlevels=r.nl, want_stages=True)
        assert len(kps) > 0
        fr = {}
        for l, L in enumerate(r.levels):
            c = stages[l]["cand"].astype(np.int64)
            assert stages[l]["nfeat"] == L.nfeat
            if len(c):
                case = K.make(L, "%s level %d" % (name, l), np.column_stack([c[:, 0] - L.minB, c[:, 1] - L.minB, c[:, 2]]))
                assert np.array_equal(case.cands[:, :2] + L.minB, c[:, :2])              # the oracle's order is rank order
                assert len(K.survivors(L, case)) == len(c)                               # what the oracle lists has passed the ini / min rule already
                fr[l] = (case, K.orders(case, l)["shuffled"])
        nsel, sel, status = r.plant([fr])
        assert status == 0
        for l, L in enumerate(r.levels):
            k = kps[kps["octave"] == l]
            got = sel[0, L.sel_off:L.sel_off + int(nsel[0, l])].astype(np.int64)
            assert len(got) == len(k), "%s level %d: %d selected, the oracle has %d keypoints" % (name, l, len(got), len(k))
            x, y = (got & 4095).astype(np.float32), (got >> 12 & 4095).astype(np.float32)
            if l:
                x, y = x * sf[l], y * sf[l]
            assert np.array_equal(x, k["x"]) and np.array_equal(y, k["y"]) and np.array_equal((got >> 24).astype(np.float32), k["response"]), "%s level %d" % (name, l)


def test_hook_refuses_what_the_kernel_relies_on_and_leaves_the_context_clean(rig, oracle):
    import semantic_slam_mapping_amd as ssm
    r = rig(0)
    L, L1 = r.levels[0], r.levels[1]
    cells = r.g["cells_total"]
    good = K.random(L, 1, 50)
    words = K.encode(L, good.cands)

    def call(ncand, cand, cellmax=None, n=1):
        nc = np.zeros((n, r.nl), np.int32); nc[0, :len(ncand)] = ncand
        return r.c.debug_orb_octree(nc, cand, np.zeros((n, cells), np.int32) if cellmax is None else cellmax)

    def lo(x, y, s=50):
        return x | y << 12 | s << 24

    def hi(cell, yin, xin):
        return cell << 14 | yin << 7 | xin

    ok = (lo(10, 10), hi(0, 10, 10))
    assert call([1], np.array([ok], np.uint32))[0][0, 0] == 1                    # the candidate every refusal below is a variation of is accepted and selected
    cm_bad_hi, cm_bad_lo = np.zeros((1, cells), np.int32), np.zeros((1, cells), np.int32)
    cm_bad_hi[0, cells - 1] = 256; cm_bad_lo[0, 0] = -1
    bad = [
        ("count below 0", lambda: call([-1], np.zeros((0, 2), np.uint32))),
        ("count above the capacity", lambda: call([L.cand_cap + 1], np.tile(np.array([ok], np.uint32), (L.cand_cap + 1, 1)))),
        ("count above a higher level's capacity", lambda: call([0, L1.cand_cap + 1], np.tile(np.array([ok], np.uint32), (L1.cand_cap + 1, 1)))),
        ("x left of the window", lambda: call([1], np.array([(lo(2, 10), hi(0, 10, 2))], np.uint32))),
        ("x right of the window", lambda: call([1], np.array([(lo(L.W - 3, 10), hi(L.nCols - 1, 10, L.W - 3 - (L.nCols - 1) * L.wCell))], np.uint32))),
        ("y above the window", lambda: call([1], np.array([(lo(10, 2), hi(0, 2, 10))], np.uint32))),
        ("y below the window", lambda: call([1], np.array([(lo(10, L.H - 3), hi((L.nRows - 1) * L.nCols, L.H - 3 - (L.nRows - 1) * L.hCell, 10))], np.uint32))),
        ("cell id outside the level", lambda: call([1], np.array([(lo(10, 10), hi(L.nCols * L.nRows, 10, 10))], np.uint32))),
        ("cell id of another cell", lambda: call([1], np.array([(lo(10, 10), hi(1, 10, 10))], np.uint32))),
        ("x offset off by one", lambda: call([1], np.array([(lo(10, 10), hi(0, 10, 11))], np.uint32))),
        ("y offset off by one", lambda: call([1], np.array([(lo(10, 10), hi(0, 9, 10))], np.uint32))),
        ("cell maximum above 255", lambda: call([len(words)], words, cm_bad_hi)),
        ("cell maximum below 0", lambda: call([len(words)], words, cm_bad_lo)),
        ("no frame", lambda: r.c._chk(r.c.lib.ssm_debug_orb_octree(r.c.h, 0, words.ctypes.data, words.ctypes.data, words.ctypes.data, None, words.ctypes.data, words.ctypes.data, words.ctypes.data, None))),
        ("more frames than max_batch", lambda: call([0], np.zeros((0, 2), np.uint32), n=r.batch + 1)),
    ]
    # (the last valid column and row are accepted: the refusals above are exactly one past them)
    edge = K.make(L, "edge", np.array([[L.W - 4, L.H - 4, 50]]))
    r.check([{0: (edge, np.arange(1))}], r.plant([{0: (edge, np.arange(1))}]), "last valid position")
    for what, fn in bad:
        with pytest.raises(ssm.SsmError) as e:
            fn()
        assert e.value.code == -1, what                                          # SSM_E_INVAL
        assert r.c.last_error(), what
    # after the refusals and a large planted case an ordinary extraction on the same context equals the oracle: no status word and nothing planted is left behind
    big = r.table(0)[10]
    r.check([{0: (big, np.arange(len(big.cands)))}], r.plant([{0: (big, np.arange(len(big.cands)))}]), "largest case")
    img = oracle.bgr2gray(oracle.synth_frame(SEED, 3)[0])
    ok_k, ok_d = oracle.orb_extract(img, nfeatures=r.nfeat)
    gk, gd, _ = r.c.detect_features(img)
    assert len(gk) == len(ok_k) and gk.tobytes() == ok_k.tobytes() and np.array_equal(gd, ok_d)
