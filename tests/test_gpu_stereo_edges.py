"""Edge paths of two parallel forms of sequential algorithms on the stereo path, GPU vs the CPU oracle bit for bit, on inputs built to reach them
(tests/stereo_ref.py builds the inputs; tests/test_stereo_ref.py checks there, without a GPU, that each input has the property it exists for):

* goodFeaturesToTrack's minDistance selection (kernels_quad.hip): dependency chains far longer than the 1 + 12 launched rounds, more stronger
  neighbours than the 32-entry dependency list, windows wider than the bit-image scan, exact distance boundaries, exact ties and max_corners cuts
  inside them, and plateaus of equal eigenvalues with more candidates than the w*h/4 + 1024 list (selected on the pixel grid) -- through ssm_gftt,
  ssm_quad_track and a batch of ssm_stereo_seq_process;
* the SGBM post stages (sgbm_post.inc) through ssm_debug_sgbm_post: the int16 3x3 median and the two-level union-find of filterSpeckles on combs,
  spirals, serpentines, components of exactly maxSize, maxDiff boundaries, int16 extremes and dense random maps, every map as several frames of one
  launch (all frames must agree), and stacked frames that would join if their forests leaked into each other;
* the per-call functions that carve one scratch / pinned buffer into regions, interleaved on one context so that every layout is built small, large and
  small again and each buffer grows under one function and is carved again by the next."""
import numpy as np
import pytest
import stereo_ref as R
from test_gpu_stereo_seq import stereo_sequence, reference_walk, check_against_walk, run_seq
from conftest import rand_desc
from test_gpu_quad import stereo_pair as quad_images
from test_gpu_pnp import KCAM, _check as check_pnp
from test_pnp import _case as pnp_case
from test_sgbm import stereo_pair as sgbm_pair
from test_vo import scene as vo_scene, F, CU, CV, BASE

pytestmark = pytest.mark.gpu

GFTT = R.gftt_cases()
SPECKLE = R.speckle_cases()


@pytest.fixture(scope="module")
def gctx():
    """a context of its own: the candidate list of a geometry is max(w*h/4 + 1024, the largest max_corners seen at it), so the GFTT cases, whose
    max_corners stay below w*h/4 + 1024 where the list must overflow, see the list length they were built for"""
    import semantic_slam_mapping_amd as ssm
    c = ssm.Context(0, width=640, height=480, max_batch=4)
    yield c
    c.close()


@pytest.mark.parametrize("name", sorted(GFTT))
def test_gftt_edge_cases(gctx, oracle, name):
    img, mc, q, md, _ = GFTT[name]
    mc = mc if mc > 0 else 30000
    g = gctx.gftt(img, mc, q, md)
    o = oracle.gftt(img, mc, q, md)
    assert len(o) > 0 and len(g) == len(o) and g.tobytes() == o.tobytes()


@pytest.mark.parametrize("h,w,box", [(48, 64, None), (480, 640, None), (480, 640, (40, 440, 100, 600)), (376, 1241, None), (376, 1241, (60, 300, 200, 1000))])
def test_gftt_plateaus(gctx, oracle, h, w, box):
    """2 x 2-pixel checkerboard cells: ~ one candidate per pixel, more than the list holds (the pixel-grid selection); minDistance 1 keeps more corners
    than the list too (the strongest `cap` of them go to the output)"""
    img = R.checker(h, w, box=box)
    cap = w * h // 4 + 1024
    assert len(R.gftt_candidates(oracle.min_eigen_map(img), 0.04)[0]) > cap
    for mc, q, md in ((1000, 0.04, 8.0), (min(30000, cap), 0.01, 1.0), (min(5000, cap), 0.01, 1.5), (300, 0.01, 20.0)):
        g = gctx.gftt(img, mc, q, md)
        o = oracle.gftt(img, mc, q, md)
        assert len(g) == len(o) > 0 and g.tobytes() == o.tobytes(), (mc, q, md)
    # the context goes on as before: a textured image right after
    tex = R.checker(h, w, box=(0, 0, 0, 0))
    assert gctx.gftt(tex, 1000, 0.04, 8.0).tobytes() == oracle.gftt(tex, 1000, 0.04, 8.0).tobytes()


@pytest.mark.parametrize("w,h", [(640, 480), (1241, 376)])
def test_quad_track_on_plateaus(ctx, oracle, w, h):
    """the current left image and the previous one carry a plateau patch (both GFTT frames of the call take the pixel-grid selection)"""
    big = R.checker(h, w, box=(h // 8, h - h // 8, w // 6, w - w // 6))
    sh = lambda im, dx, dy=0: np.roll(np.roll(im, dx, axis=1), dy, axis=0).copy()
    lc = big; rc = sh(big, -9); lp = sh(big, 2, 1); rp = sh(lp, -9)
    g = ctx.quad_track(lc, rc, lp, rp)
    o = oracle.quad_track(lc, rc, lp, rp)
    assert len(o) > 0 and g.tobytes() == o.tobytes()


def test_sequence_batch_with_a_plateau_frame(oracle):
    """one frame of a batched sequence is a plateau: the batch's other frames keep the list path, that frame the pixel-grid path, in one launch"""
    import semantic_slam_mapping_amd as ssm
    from semantic_slam_mapping_amd.api import GlibcRand
    c = ssm.Context(0, width=640, height=480, max_batch=2, stereo_batch=4)
    try:
        n, w, h, iters = 6, 480, 200, 60
        L, R_ = stereo_sequence(oracle, n, w, h, disp=9, flow=(2, 1))
        L[2] = R.checker(h, w, box=(20, 180, 40, 440)); R_[2] = np.roll(L[2], -9, axis=1)
        assert len(R.gftt_candidates(oracle.min_eigen_map(L[2]), 0.04)[0]) > h * w // 4 + 1024
        walk, _ = reference_walk(oracle, L, R_, iters, None, depth=False)
        res = run_seq(c, L, R_, GlibcRand(0), iters, stages=1 | 4)
        check_against_walk(res, walk, depth=False)
        for f in range(n):
            gc = oracle.gftt(L[f], 1000)
            assert res["ncorners"][f] == len(gc) > 0 and np.array_equal(res["corners"][f, :len(gc)], gc), f
    finally:
        c.close()


def _post_expected(oracle, m, op, nv, ms, md):
    a = oracle.median3_s16(m) if op & 1 else m
    return oracle.filter_speckles(a, nv, ms, md) if op & 2 else a


@pytest.mark.parametrize("name", sorted(SPECKLE))
def test_sgbm_post_edge_cases(ctx, oracle, name):
    maps, nv, ms, md, _ = SPECKLE[name]
    k = len(maps)
    batch = np.concatenate([maps] * 3)                                  # >= 3 copies of every map in one launch
    for op in (1, 2, 3):
        out = ctx.debug_sgbm_post(batch, op, nv, ms, md)
        for i, m in enumerate(maps):
            exp = _post_expected(oracle, m, op, nv, ms, md)
            for r in range(3):
                assert np.array_equal(out[r * k + i], exp), (op, i, r)


@pytest.mark.parametrize("w", [1, 63, 64, 65, 127, 1241])
@pytest.mark.parametrize("h", [1, 15, 16, 17, 376])
def test_sgbm_post_sizes(ctx, oracle, w, h):
    """dense random maps over a few values at tile-edge sizes: four frames per launch, two speckle settings"""
    rng = np.random.default_rng(w * 1000 + h)
    vals = np.array([R.NV, 100, 101, 103, 110, -32768, 32767], np.int16)
    maps = rng.choice(vals, size=(4, h, w), p=[0.1, 0.3, 0.25, 0.15, 0.1, 0.05, 0.05])
    for ms, md in ((5, 1), (40, 3)):
        out = ctx.debug_sgbm_post(maps, 3, R.NV, ms, md)
        for i, m in enumerate(maps):
            assert np.array_equal(out[i], _post_expected(oracle, m, 3, R.NV, ms, md)), (ms, md, i)


def test_per_call_layouts_small_large_small(oracle):
    """window_match, vo_estimate, pnp_solve, debug_sgbm_post, sgbm and quad_track take their regions from the context's one scratch buffer and one pinned area
    (and the pair calls from one device staging buffer).  Three rounds on a fresh context -- small, large, small again -- so that each buffer is allocated by one
    function, grown by another and carved again by every one of them at a size below what it holds; every result is the oracle's, bit for bit."""
    import semantic_slam_mapping_amd as ssm
    rng = np.random.default_rng(77)
    vals = np.array([R.NV, 100, 101, 103, 110, -32768, 32767], np.int16)

    def window(c, n1, n2):
        k1 = rng.uniform(0, 100, (n1, 2)).astype(np.float32); k2 = rng.uniform(0, 100, (n2, 2)).astype(np.float32)
        d1 = rand_desc(rng, n1); d2 = (d1[rng.integers(0, n1, n2)] ^ (rng.random((n2, 32)) < 0.02).astype(np.uint8)) if n2 else np.zeros((0, 32), np.uint8)
        g = c.window_match(k1, d1, k2, d2, 20, 20, 80.0)
        assert len(g) == n1 and g.tobytes() == oracle.window_match(k1, d1, k2, d2, 20, 20, 80.0).tobytes(), (n1, n2)

    def vo(c, n, iters):
        m = vo_scene(n, n // 5, 300 + n, noise=0.2 if n > 6 else 0.0)
        smp = oracle.vo_samples(oracle.rand_state(0), n, iters)
        ok, tr, inl = oracle.vo_estimate(m, oracle.vo_params(F, CU, CV, BASE, 2.0, True), smp)
        gok, gtr, ginl = c.vo_estimate(m, F, CU, CV, BASE, smp, 2.0, True)
        assert gok == ok and np.array_equal(ginl, inl) and gtr.tobytes() == tr.tobytes(), (n, iters)

    def pnp(c, n):
        img, obj, _ = pnp_case(40 + n % 7, n, 6, 7, 0.5)
        check_pnp(c, oracle, img, obj, np.eye(4))

    def post(c, n, h, w):
        maps = rng.choice(vals, size=(n, h, w), p=[0.1, 0.3, 0.25, 0.15, 0.1, 0.05, 0.05])
        out = c.debug_sgbm_post(maps, 3, R.NV, 5, 1)
        for i, m in enumerate(maps):
            assert np.array_equal(out[i], _post_expected(oracle, m, 3, R.NV, 5, 1)), (n, h, w, i)

    def sgbm(c, h, w, nd, sad, seed):
        l, r, _ = sgbm_pair(h, w, seed, planes=((nd // 4, None), (nd // 2 + 3, (0.3, 0.75, 0.3, 0.7))), noise=3)
        assert np.array_equal(c.sgbm(l, r, c.sgbm_params(numberOfDisparities=nd, SADWindowSize=sad)), oracle.sgbm(l, r, oracle.sgbm_params(num_disp=nd, sad=sad))), (h, w)

    def quad(c):
        ims = quad_images(oracle, 64, 48, 5, (2, 1))
        g = c.quad_track(*ims); o = oracle.quad_track(*ims)
        assert len(o) > 0 and len(g) == len(o) and g.tobytes() == o.tobytes()

    c = ssm.Context(0, width=640, height=480, max_batch=1)
    try:
        for wm, von, pn, pm, sg in (((1, 0), (6, 1), 0, (1, 7, 5), (40, 120, 16, 5, 6)),
                                    ((700, 650), (900, 50), 3000, (3, 40, 120), (61, 333, 80, 11, 9)),
                                    ((3, 5), (6, 1), 1, (1, 7, 5), (40, 120, 16, 5, 6))):
            window(c, *wm); vo(c, *von); pnp(c, pn); post(c, *pm); sgbm(c, *sg); quad(c)
    finally:
        c.close()
