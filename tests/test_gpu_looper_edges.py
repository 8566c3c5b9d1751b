"""The device looper (csrc/kernels_bow.hip, csrc/ssm_looper.hip) where tests/test_gpu_looper.py does not go: every LDS sort size P from 128 to 4096 with frames
of 0, 1, 2, cap - 1 and cap features, sibling groups wider than the 16 lanes that share a descriptor (the tie rule across lanes and across trips), both descent
kernels (SSM_BOW_VARIANT), ragged bulk adds with garbage behind every frame's descriptors, long runs and dropped words, and the edges of query().
Sources of truth: a bag of words and a score row are the bytes of the library's host path (Vocabulary.transform / Vocabulary.score: the arithmetic of
include/ssm/looper_core.h, itself checked on the CPU against tests/looper_ref.py and exact rationals in tests/test_looper.py); a candidate list is exactly the
list of tests/looper_ref.py, in pairs and in order, under the condition -- asserted -- that no reference score lies within 1e-9 of the threshold; candidate
scores are within 8 cap 2^-53 of the restatement's (cap = the context's features per frame: a sum of at most cap terms whose magnitudes total at most 4)."""
import ctypes as C
import functools
import os
import sys
import types
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import looper_ref as R  # noqa: E402
from conftest import CAM  # noqa: E402

pytestmark = pytest.mark.gpu
VARIANTS = (None, "1")                                        # SSM_BOW_VARIANT: unset = 16 lanes per descriptor, 1 = one lane per descriptor
TINY = {"tiny": (), "tiny_zero1": (1,), "tiny_zero_all": (0, 1, 2)}


def _ssm():
    import semantic_slam_mapping_amd as ssm
    return ssm


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def _looper(ctx, v, monkeypatch=None, variant=None):
    """the variable is read when the looper is created"""
    if monkeypatch is not None:
        if variant is None:
            monkeypatch.delenv("SSM_BOW_VARIANT", raising=False)
        else:
            monkeypatch.setenv("SSM_BOW_VARIANT", variant)
    return _ssm().Looper(ctx, v)


def _host_rows(v, vecs, full=False):
    """Vocabulary.score for row q against the entries 0 .. q (full: against all), through the library call itself with the pointers taken once"""
    lib, out = v.lib, C.c_double(0)
    ref = C.byref(out)
    arg = [(i.ctypes.data, x.ctypes.data, len(i)) for i, x in vecs]
    rows = []
    for q in range(len(vecs)):
        row = np.zeros(len(vecs) if full else q + 1)
        for e in range(len(row)):
            assert lib.ssm_bow_score_host(*arg[q], *arg[e], ref) == 0
            row[e] = out.value
        rows.append(row)
    return rows


# ---- 1. descent: wide sibling groups and leaves above level L, both kernels -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _descent_case(name):
    """-> (the vocabulary's arrays, [(descriptors of a frame, the word each of them must get or None)])"""
    rng = np.random.default_rng(51)
    if name == "irregular":
        arrays = R.make_irregular_vocab(13)
        return arrays, [(R.rand_desc(rng, n), None) for n in (0, 1, 63, 64, 65, 1000, 1024)]
    arrays, queries, want = R.make_wide_vocab(14)
    frames = [(queries, want)]
    big = R.rand_desc(rng, 4096)
    frames += [(big[i:i + 1024], None) for i in range(0, 4096, 1024)]
    # every root child's own descriptor.  A leaf child: itself, or the earlier copy where the descriptor is duplicated
    first = np.arange(300); first[[b for _, b in R.WIDE_ROOT_PAIRS]] = [a for a, _ in R.WIDE_ROOT_PAIRS]
    frames.append((arrays[4][20:300], (first[20:300] - 20).astype(np.int32)))
    frames.append((arrays[4][:20], None))                    # an inner child: some word of its own group (checked in the test)
    return arrays, frames


def _descent_run(ctx, monkeypatch, name, variant):
    arrays, frames = _descent_case(name)
    v = _ssm().Vocabulary.from_arrays(*arrays)
    lp = _looper(ctx, v, monkeypatch, variant)
    for e, (d, _) in enumerate(frames):
        lp.add(d, e)
    got = [lp.bow(e) for e in range(len(frames))]
    lp.close()
    return v, frames, got


@pytest.mark.parametrize("variant", VARIANTS, ids=["subgroup", "lane"])
@pytest.mark.parametrize("name", ["wide", "irregular"])
def test_descent_equals_host(ctx, monkeypatch, name, variant):
    assert ctx.cap == 1024
    v, frames, got = _descent_run(ctx, monkeypatch, name, variant)
    weight = np.asarray(_descent_case(name)[0][5])[np.asarray(_descent_case(name)[0][3]) > 0]
    for e, (d, want) in enumerate(frames):
        wof, ids, vals = v.transform(d)
        if want is not None:
            assert np.array_equal(wof, want), e                # the host path's word list, stated directly
        assert _same(got[e], (ids, vals)), (name, variant, e)
        kept = np.unique(wof[weight[wof] > 0])
        assert np.array_equal(got[e][0], kept), e                  # and the device's ids are those words
    if name == "wide":
        rv = R.RefVocab(*_descent_case(name)[0])
        wof = v.transform(frames[-1][0])[0]                        # root child c < 20 is inner: its descriptor goes down into c's own group
        for c in range(20):
            group = rv.word_of_id[rv.kids[rv.start[c + 1]:rv.start[c + 1] + rv.cnt[c + 1]]]
            assert wof[c] in group, c
        assert np.array_equal(got[-1][0], np.unique(wof))


@pytest.mark.parametrize("name", ["wide", "irregular"])
def test_descent_variants_identical(ctx, monkeypatch, name):
    a = _descent_run(ctx, monkeypatch, name, None)[2]
    b = _descent_run(ctx, monkeypatch, name, "1")[2]
    assert len(a) == len(b) > 4 and all(_same(x, y) for x, y in zip(a, b))
    assert sum(len(x[0]) for x in a) > 100


# ---- 2. every LDS sort size ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("features,levels,cap,P", [(100, 1, 103, 128), (232, 8, 256, 256), (233, 8, 257, 512), (1000, 8, 1024, 1024), (4072, 8, 4096, 4096)])
def test_sort_sizes(features, levels, cap, P):
    """one context per cap; frames of 0, 1, 2, cap - 1 and cap features (cap == P: no padding key in the sort) of three kinds: random descriptors on 1000 words,
    random descriptors on three words (runs of about n / 3 that span many threads' chunks; one word or all words of weight 0), n copies of one descriptor"""
    ssm = _ssm()
    c = ssm.Context(0, orb_features=features, orb_levels=levels, max_batch=1, voxel_capacity_log2=16, camera=CAM)
    try:
        assert c.cap == cap and P >= cap > P // 2
        sizes = (0, 1, 2, cap - 1, cap)
        rng = np.random.default_rng(61)
        vocabs = {"k10L3": R.make_vocab(10, 3, 11)}
        vocabs.update({k: R.make_tiny_vocab(15, zero=z) for k, z in TINY.items()})
        for name, arrays in vocabs.items():
            v = ssm.Vocabulary.from_arrays(*arrays)
            lp = ssm.Looper(c, v)
            host = []
            for e, n in enumerate(sizes):
                q = R.rand_desc(rng, n)
                lp.add(q, e)
                wof, ids, vals = v.transform(q)
                host.append((ids, vals))
                assert _same(lp.bow(e), host[-1]), (cap, name, n)
                if name == "tiny_zero_all":
                    assert len(lp.bow(e)[0]) == 0                 # a non-empty frame, an empty vector
                elif name == "tiny" and n >= 100:
                    assert len(ids) == 3 and np.bincount(wof).min() > n // 6
            one = R.rand_desc(rng, 1)
            w = int(v.transform(one)[0][0])
            for n in sizes:                                        # a single run of length n: the word's weight added n times, divided by itself
                lp.add(np.repeat(one, n, axis=0), 100 + n)
                ids, vals = lp.bow(len(lp) - 1)
                if n == 0 or arrays[5][arrays[3] > 0][w] <= 0:
                    assert len(ids) == 0, (cap, name, n)
                else:
                    assert ids.tolist() == [w] and vals.tolist() == [1.0], (cap, name, n)
                assert _same((ids, vals), v.transform(np.repeat(one, n, axis=0))[1:])
                host.append((ids, vals))
            if name == "k10L3":                                    # the score kernel holds a query of up to cap entries in LDS
                q = len(sizes) - 1
                rows = _host_rows(v, host[:q + 1])
                assert lp.scores(q).tobytes() == rows[q].tobytes() and rows[q][q] > 0.99
            lp.close()
    finally:
        c.close()


def test_more_than_4096_features_is_refused():
    ssm = _ssm()
    c = ssm.Context(0, orb_features=4073, orb_levels=8, max_batch=1, voxel_capacity_log2=16, camera=CAM)
    try:
        assert c.cap == 4097
        v = ssm.Vocabulary.from_arrays(*R.make_tiny_vocab(15))
        before = ssm.live_allocations()
        with pytest.raises(ssm.SsmError) as e:
            ssm.Looper(c, v)
        assert e.value.code == -1 and "looper: at most 4096 features per frame (ssm_orb_capacity)" in str(e.value)
        assert ssm.live_allocations() == before
        data = np.arange(1000, dtype=np.int32)                     # the context still works
        p = c.dev_alloc(data.nbytes)
        c.h2d(p, data)
        assert np.array_equal(c.d2h(p, data.shape, np.int32), data)
        c.dev_free(p)
        assert ssm.live_allocations() == before
    finally:
        c.close()


# ---- 3. ragged bulk add ----------------------------------------------------------------------------------------------------------------------------------
def test_ragged_bulk_add(ctx):
    """300 frames whose counts cycle through 0, 1, 17, 63, 64, 65, cap, cap + 5 (clamped), -3 (clamped to 0), 500, every unused descriptor slot random bytes;
    one bulk call of 200 (the value arrays grow from nothing: 200 x 1024 > 65536), one of 100 (crosses the 256-entry growth), then all 300 once more in one
    call (the value arrays grow with entries in them)"""
    ssm = _ssm()
    cap, F = ctx.cap, 300
    assert cap == 1024
    v = ssm.Vocabulary.from_arrays(*R.make_vocab(10, 3, 11))
    rng = np.random.default_rng(71)
    desc = rng.integers(0, 256, size=(F, cap, 32), dtype=np.uint8)     # nothing is zero behind a frame's count
    cycle = [0, 1, 17, 63, 64, 65, cap, cap + 5, -3, 500]
    nkp = np.array([cycle[f % len(cycle)] for f in range(F)], np.int32)
    clamped = np.clip(nkp, 0, cap)
    d_desc, d_nkp = ctx.dev_alloc(desc.nbytes), ctx.dev_alloc(nkp.nbytes)
    ctx.h2d(d_desc, desc); ctx.h2d(d_nkp, nkp)
    ids = np.arange(F) * 3
    bulk, single = ssm.Looper(ctx, v), ssm.Looper(ctx, v)
    try:
        for f0, n in ((0, 200), (200, 100)):
            bulk.add_dev(types.SimpleNamespace(desc=d_desc + f0 * cap * 32, nkp=d_nkp + f0 * 4, cap=cap), n, ids[f0:f0 + n])
        assert len(bulk) == F
        host = [v.transform(desc[f, :clamped[f]])[1:] for f in range(F)]
        for f in range(F):                                          # the entries written before each growth included
            assert _same(bulk.bow(f), host[f]), (f, int(nkp[f]))
            single.add(desc[f, :clamped[f]], ids[f])
        assert [len(host[f][0]) for f in (0, 8)] == [0, 0] and len(host[1][0]) == 1
        for q in (0, 1, 6, 7, 8, 199, 200, 255, 256, 299):
            assert bulk.scores(q).tobytes() == single.scores(q).tobytes(), q
        assert bulk.scores(299, against=300).tobytes() == single.scores(299, against=300).tobytes()
        a, b = bulk.query(0, F, 0.0, 3), single.query(0, F, 0.0, 3)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and len(a[0]) > 1000
        bulk.add_dev(types.SimpleNamespace(desc=d_desc, nkp=d_nkp, cap=cap), F, ids + 5000)
        assert len(bulk) == 2 * F
        for f in range(F):
            assert _same(bulk.bow(f), host[f]) and _same(bulk.bow(F + f), host[f]), f
    finally:
        bulk.close(); single.close()
        ctx.dev_free(d_desc); ctx.dev_free(d_nkp)


# ---- 4. query edges --------------------------------------------------------------------------------------------------------------------------------------
QF, THR, INTERVAL = 600, 0.3, 10
EMPTY = (0, 5, 300, 599)


def _score_tol(ctx):
    return 8 * ctx.cap * 2.0 ** -53


@pytest.fixture(scope="module")
def qdb(ctx):
    """600 frames of 20 .. 80 random descriptors on 100 words; frames 0, 5, 300, 599 empty, frame 7 a single descriptor; frame ids 0 .. 599.  Computed once:
    the restatement's vectors and score matrix, the host path's vectors and score rows, the device's score rows"""
    ssm = _ssm()
    arrays = R.make_vocab(10, 2, 21)
    rv = R.RefVocab(*arrays)
    v = ssm.Vocabulary.from_arrays(*arrays)
    rng = np.random.default_rng(77)
    sets = [R.rand_desc(rng, int(rng.integers(20, 81))) for _ in range(QF)]
    for f in EMPTY:
        sets[f] = R.rand_desc(rng, 0)
    sets[7] = R.rand_desc(rng, 1)
    ref = [rv.transform(d)[1:] for d in sets]
    host = [v.transform(d)[1:] for d in sets]
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(ref, host))
    S = R.score_matrix(ref, rv.words)
    lp = ssm.Looper(ctx, v)
    for f, d in enumerate(sets):
        lp.add(d, f)
    db = types.SimpleNamespace(v=v, sets=sets, ref=ref, host=host, S=S, lp=lp, ids=np.arange(QF), gap=float(np.abs(S - THR).min()))
    db.dev = [lp.scores(q) for q in range(QF)]
    yield db
    lp.close()


def _pairs(p):
    return [tuple(x) for x in p.tolist()]


def _check(db, ctx, got, want):
    pairs, sc = got
    assert len(pairs) == len(sc) == len(want)                     # the returned count is exact
    assert _pairs(pairs) == [(q, e) for q, e, _ in want]
    if len(want):
        assert np.abs(sc - np.array([s for _, _, s in want])).max() <= _score_tol(ctx)


def test_query_scores_equal_host(qdb, ctx):
    host = _host_rows(qdb.v, qdb.host)
    for q in range(QF):
        assert qdb.dev[q].tobytes() == host[q].tobytes(), q
    zero = np.zeros(1).tobytes()                                   # +0.0, not -0.0
    for f in EMPTY:
        assert all(x.tobytes() == zero for x in qdb.dev[f])                                   # an empty query
        assert all(qdb.dev[q][f:f + 1].tobytes() == zero for q in range(f, QF))               # an empty stored entry
        full = qdb.lp.scores(f, against=QF)
        assert full.tobytes() == np.zeros(QF).tobytes()
    assert np.abs(np.concatenate(qdb.dev) - qdb.S[np.tril_indices(QF)]).max() <= _score_tol(ctx)
    assert all(abs(qdb.dev[q][q] - 1.0) <= _score_tol(ctx) for q in range(QF) if q not in EMPTY)


def test_query_full_list(qdb, ctx):
    """83 707 candidates; 113 queries have more than 256 each (the emit kernel's 256-wide scan and its running base), the largest 415"""
    want = R.candidates_range(qdb.ref, qdb.ids, 0, QF, -1, THR, INTERVAL, scores=qdb.S)
    per = np.bincount([q for q, _, _ in want], minlength=QF)
    print(f"{len(want)} candidates, {(per > 256).sum()} queries above 256, largest {per.max()}, nearest score {qdb.gap:.3g} from the threshold")
    assert qdb.gap > 1e-9                                           # the condition: no score so close that a last-bit difference could move a candidate
    assert (len(want), int((per > 256).sum()), int(per.max())) == (83707, 113, 415)
    _check(qdb, ctx, qdb.lp.query(0, QF, THR, INTERVAL), want)


@pytest.mark.parametrize("first,n,against", [(400, 150, 0), (400, 150, 600), (400, 150, 500), (599, 1, -1), (300, 0, -1), (0, 600, 600), (0, 1, -1)],
                         ids=["against0", "against_len", "against_mid_self_and_later", "last_entry", "n0", "full_square", "first_entry"])
def test_query_sub_ranges(qdb, ctx, first, n, against):
    assert qdb.gap > 1e-9
    want = R.candidates_range(qdb.ref, qdb.ids, first, n, against, THR, INTERVAL, scores=qdb.S)
    got = qdb.lp.query(first, n, THR, INTERVAL, against=against)
    _check(qdb, ctx, got, want)
    if against == 0 or n == 0 or (first, n) in ((599, 1), (0, 1)):    # (599 and 0 are empty frames)
        assert len(got[0]) == 0
    if against == 500:
        later = [(q, e) for q, e in _pairs(got[0]) if e > q]
        assert len(later) > 256                                           # entries behind the query are in range
    if against == 600 and n == 600:
        assert len(want) == 2 * 83707                                     # the score is symmetric


def test_query_negative_interval_and_score(qdb, ctx):
    assert qdb.gap > 1e-9
    want = R.candidates_range(qdb.ref, qdb.ids, 0, QF, -1, THR, -1, scores=qdb.S)
    got = qdb.lp.query(0, QF, THR, -1)
    _check(qdb, ctx, got, want)
    selfs = [q for q, e in _pairs(got[0]) if q == e]
    assert selfs == [q for q in range(QF) if q not in EMPTY]         # |0| > -1: every non-empty entry pairs with itself
    # 0 > -1: empty entries are candidates too, like in the restatement.  No score is within 1e-9 of -1 (all are >= 0)
    want = R.candidates_range(qdb.ref, qdb.ids, 0, QF, -1, -1.0, INTERVAL, scores=qdb.S)
    assert len(want) == sum(max(0, q - INTERVAL) for q in range(QF)) and qdb.S.min() >= 0.0
    got = qdb.lp.query(0, QF, -1.0, INTERVAL)
    _check(qdb, ctx, got, want)
    assert (599, 0) in _pairs(got[0][-600:])


def test_query_comparisons_are_strict(qdb, ctx):
    """exact: the expected lists come from the device's own score rows"""
    pairs, sc = qdb.lp.query(0, QF, THR, INTERVAL)
    k = len(sc) // 2
    q0, e0 = (int(x) for x in pairs[k])
    s = float(sc[k])
    assert qdb.dev[q0][e0] == s
    want = [(q, e) for q in range(QF) for e in np.nonzero(qdb.dev[q] > s)[0].tolist() if abs(e - q) > INTERVAL]
    got = qdb.lp.query(0, QF, s, INTERVAL)
    assert _pairs(got[0]) == want and (q0, e0) not in want and 0 < len(want) < len(sc)
    assert all(qdb.dev[q][e] == x for (q, e), x in zip(want, got[1].tolist()))
    d = abs(e0 - q0)                                                  # the same for the interval: |id difference| == min_interval is no candidate
    want = [(q, e) for q in range(QF) for e in np.nonzero(qdb.dev[q] > THR)[0].tolist() if abs(e - q) > d]
    got = qdb.lp.query(0, QF, THR, d)
    assert _pairs(got[0]) == want and (q0, e0) not in want and d > INTERVAL
    assert any(abs(e - q) == d + 1 for q, e in want)


def test_query_capacity(qdb, ctx):
    ssm = _ssm()
    want = R.candidates_range(qdb.ref, qdb.ids, 0, QF, -1, THR, INTERVAL, scores=qdb.S)
    count = len(want)
    _check(qdb, ctx, qdb.lp.query(0, QF, THR, INTERVAL, cap=count), want)
    for cap in (count - 1, 0):
        with pytest.raises(ssm.SsmError) as e:
            qdb.lp.query(0, QF, THR, INTERVAL, cap=cap)
        assert e.value.code == -4 and e.value.needed == count
        sub = R.candidates_range(qdb.ref, qdb.ids, 500, 40, -1, THR, INTERVAL, scores=qdb.S)      # and answers the next query
        _check(qdb, ctx, qdb.lp.query(500, 40, THR, INTERVAL), sub)
        assert len(sub) > 256
    _check(qdb, ctx, qdb.lp.query(0, QF, THR, INTERVAL, cap=count), want)


def test_query_permuted_negative_frame_ids(qdb, ctx):
    """the same frames under frame ids that are a shuffle of -1000 .. -401"""
    ids = np.random.default_rng(79).permutation(QF) - 1000
    assert ids.max() < 0 and np.any(np.diff(ids) < 0)
    lp = _ssm().Looper(ctx, qdb.v)
    try:
        for f, d in enumerate(qdb.sets):
            lp.add(d, int(ids[f]))
        want = R.candidates_range(qdb.ref, ids, 0, QF, -1, THR, INTERVAL, scores=qdb.S)
        assert 80000 < len(want) != 83707 and qdb.gap > 1e-9
        _check(qdb, ctx, lp.query(0, QF, THR, INTERVAL), want)
        want = R.candidates_range(qdb.ref, ids, 400, 150, 500, THR, INTERVAL, scores=qdb.S)
        _check(qdb, ctx, lp.query(400, 150, THR, INTERVAL, against=500), want)
        want = R.candidates_range(qdb.ref, ids, 0, QF, -1, THR, -1, scores=qdb.S)
        _check(qdb, ctx, lp.query(0, QF, THR, -1), want)
    finally:
        lp.close()
