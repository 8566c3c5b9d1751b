"""The matrix-core matcher's keys (kernels_match.hip): key = 2^(e+1) H + trainIdx built in the accumulator, ONE running pair of floats per
accumulator shifted by 32 from tile to tile, two values per update, split at bit e + 1 in the epilogue.  Every case is compared exactly with the oracle's strict
'<' scan and with the VALU matcher (a context created under SSM_MATCH_VARIANT=0); where the case plants its winners they are asserted by name as well.
nq = 70: both accumulators and both lane halves of a wave write results."""
import numpy as np
import pytest

from conftest import CAM, SEED, rand_desc

pytestmark = pytest.mark.gpu
NQ = 70


@pytest.fixture(scope="module")
def valu_ctx():
    """the same entry points on the VALU matcher (the variant is read when a context is created)"""
    import semantic_slam_mapping_amd as ssm
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("SSM_MATCH_VARIANT", "0")
        c = ssm.Context(0, orb_features=1000, max_batch=4, voxel_capacity_log2=12, camera=CAM)
    yield c
    c.close()


def flip(d, bits):
    """a copy of descriptor d with these bit positions (0 .. 255) inverted"""
    o = d.copy()
    for b in bits:
        o[b >> 3] ^= np.uint8(1 << (b & 7))
    return o


def at_distance(rng, d, h, lo=64):
    """a descriptor at Hamming distance h from d; the inverted bits are drawn from positions lo .. 255"""
    return flip(d, lo + rng.choice(256 - lo, size=h, replace=False))


def queries(rng, q0, nq=NQ):
    """nq variations of q0: query i differs from it in i % 5 of the bits 0 .. 63, so that a train descriptor made by at_distance(q0, h) is at h + i % 5 from query i --
    every lane sees other distances, and the planted order holds for all of them"""
    return np.stack([flip(q0, rng.choice(64, size=i % 5, replace=False)) for i in range(nq)])


def far(rng, q0, n):
    """n descriptors at H >= 200 from q0 (>= 196 from every query)"""
    return np.stack([at_distance(rng, q0, int(h), lo=0) for h in rng.integers(200, 257, size=n)])


def check(ctx, valu_ctx, oracle, q, t, first=None):
    """knn2 and the ratio-tested list of both matchers against the oracle; first = (i0, i1): the planted winners of every query"""
    oi, od = oracle.knn2(q, t)
    gi, gd = ctx.knn2(q, t)
    assert np.array_equal(gi, oi) and np.array_equal(gd, od), (gi[:4], oi[:4], gd[:4], od[:4])
    vi, vd = valu_ctx.knn2(q, t)
    assert np.array_equal(gi, vi) and np.array_equal(gd, vd)
    om = oracle.match(q, t, 0.97)
    assert ctx.match(q, t, 0.97).tobytes() == om.tobytes() and valu_ctx.match(q, t, 0.97).tobytes() == om.tobytes()
    if first is not None:
        assert (gi[:, 0] == first[0]).all() and (gi[:, 1] == first[1]).all(), gi[:4]
    return gi, gd


@pytest.mark.parametrize("nt", [2, 3, 31, 32, 33, 63, 64, 65, 95, 97])
def test_tile_edges(ctx, valu_ctx, oracle, nt):
    """the padded rows of a last tile, a last tile of one valid row, and one tile alone (only the start value is ever shifted)"""
    rng = np.random.default_rng(1000 + nt)
    check(ctx, valu_ctx, oracle, rand_desc(rng, NQ), rand_desc(rng, nt))


@pytest.mark.parametrize("nt,rows", [(1024, (0, 1)), (1000, (999, 998))])
def test_running_pair_through_every_tile(ctx, valu_ctx, oracle, nt, rows):
    """the two nearest (H = 0 and H = 1 from the base query) in the first two rows -- the pair is shifted 31 times and goes negative -- or in the last two valid rows
    of the last tile; every other descriptor at H >= 200"""
    rng = np.random.default_rng(nt)
    q0 = rand_desc(rng, 1)[0]
    t = far(rng, q0, nt)
    t[rows[0]] = q0
    t[rows[1]] = flip(q0, [255])
    gi, gd = check(ctx, valu_ctx, oracle, queries(rng, q0), t, first=rows)
    assert gd[0, 0] == 0 and gd[0, 1] == 1


def test_ties_everywhere(ctx, valu_ctx, oracle):
    """all train descriptors equal: every distance of a query is the same, the winners are trainIdx 0 and 1"""
    rng = np.random.default_rng(5)
    q0 = rand_desc(rng, 1)[0]
    gi, gd = check(ctx, valu_ctx, oracle, queries(rng, q0), np.tile(q0, (100, 1)), first=(0, 1))
    assert gd[0, 0] == 0 and gd[0, 1] == 0


@pytest.mark.parametrize("a", [31, 3, 7])
def test_equal_best_distance_across_a_border(ctx, valu_ctx, oracle, a):
    """the same best distance in rows a | a + 1: the tile border (31 | 32) and the lane-half and register-group borders of the accumulator layout
    (row = (i & 3) + 8 (i >> 2) + 4 h: 3 | 4 and 7 | 8).  The lower trainIdx is first"""
    rng = np.random.default_rng(50 + a)
    q0 = rand_desc(rng, 1)[0]
    t = far(rng, q0, 70)
    t[a] = at_distance(rng, q0, 3)
    t[a + 1] = at_distance(rng, q0, 3)
    gi, gd = check(ctx, valu_ctx, oracle, queries(rng, q0), t, first=(a, a + 1))
    assert gd[0, 0] == 3 and gd[0, 1] == 3


def test_extremes(ctx, valu_ctx, oracle):
    """H = 256 everywhere (the largest key), then one train at H = 255 in the last tile's only valid row: it must be first"""
    rng = np.random.default_rng(9)
    q = rand_desc(rng, NQ)[:1].repeat(NQ, axis=0)
    t = np.tile(~q[0], (33, 1))
    gi, gd = check(ctx, valu_ctx, oracle, q, t, first=(0, 1))
    assert (gd == 256).all()
    t[32] = flip(t[32], [17])
    gi, gd = check(ctx, valu_ctx, oracle, q, t, first=(32, 0))
    assert (gd[:, 0] == 255).all() and (gd[:, 1] == 256).all()


@pytest.mark.parametrize("nt", [1025, 1500, 2100, 4099])
@pytest.mark.parametrize("where", ["from_1024", "last"])
def test_key_width(ctx, valu_ctx, oracle, nt, where):
    """rows of more than 1024 descriptors: e = 10, 10, 11, 12.  The two nearest are planted at trainIdx >= 1024 (with 1025 rows only one such index exists: the
    second nearest then sits at 1023), or in the last two rows; the rest is random (H around 128)"""
    rng = np.random.default_rng(nt)
    q0 = rand_desc(rng, 1)[0]
    t = rand_desc(rng, nt)
    i0, i1 = (nt - 1, nt - 2) if where == "last" else (1024, 1024 + (nt - 1025) // 2 if nt > 1026 else 1023)
    t[i0] = q0
    t[i1] = flip(q0, [255])
    check(ctx, valu_ctx, oracle, queries(rng, q0), t, first=(i0, i1))


def test_rows_too_long_for_the_key(ctx, valu_ctx, oracle):
    """33000 train descriptors: no exact key (capT > 32768), the call takes the VALU matcher and still equals the oracle"""
    rng = np.random.default_rng(33000)
    q = rand_desc(rng, 5)
    t = rand_desc(rng, 33000)
    t[32999] = q[0]
    t[32800] = flip(q[0], [3])
    gi, gd = check(ctx, valu_ctx, oracle, q, t)
    assert tuple(gi[0]) == (32999, 32800) and tuple(gd[0]) == (0, 1)


def test_sequence_tables_equal_the_valu_matcher(oracle, monkeypatch):
    """seq_process of 7 frames (320 x 240, 300 features, 5 reference frames, stages ORB | MATCH), then a second call with continue_sequence=True whose history rows
    are the first call's last frames: nmatch and every valid match record equal those of a SSM_MATCH_VARIANT=0 context byte for byte"""
    import semantic_slam_mapping_amd as ssm
    W, H, NF, n, R = 320, 240, 300, 7, 5
    fr = [oracle.synth_frame(SEED, 40 + i, W, H) for i in range(n)]
    bgr = np.stack([f[0] for f in fr]); dep = np.stack([f[1] for f in fr])

    def run():
        c = ssm.Context(0, width=W, height=H, orb_features=NF, orb_levels=4, max_batch=4, tracker_ref_frames=R, voxel_capacity_log2=12, camera=CAM)
        bufs = [c.dev_alloc(n * W * H * 3), c.dev_alloc(n * W * H * 2)]
        try:
            assert c.R == R
            c.h2d(bufs[0], bgr); c.h2d(bufs[1], dep)
            res = []
            for cnt, cont in ((n, False), (3, True)):
                out = c.seq_process(bufs[0], bufs[1], None, None, cnt, continue_sequence=cont, stages=3)
                c.sync()
                res.append(c.seq_fetch(out, cnt))
            return res
        finally:
            for p in bufs:
                c.dev_free(p)
            c.close()

    got = run()
    monkeypatch.setenv("SSM_MATCH_VARIANT", "0")
    want = run()
    pairs = 0
    for g, w in zip(got, want):
        assert g["nkp"].tobytes() == w["nkp"].tobytes() and g["nmatch"].tobytes() == w["nmatch"].tobytes()
        for i in range(len(g["nmatch"])):
            for r in range(R):
                k = int(g["nmatch"][i, r])
                if k > 0:
                    assert g["matches"][i, r, :k].tobytes() == w["matches"][i, r, :k].tobytes(), (i, r)
                    pairs += 1
    assert (got[0]["nmatch"][0] == -1).all() and (got[1]["nmatch"] >= 0).all() and pairs >= 20      # no history in the first call, a full one in the second
