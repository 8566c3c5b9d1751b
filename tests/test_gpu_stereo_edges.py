"""Edge paths of two parallel forms of sequential algorithms on the stereo path, GPU vs the CPU oracle bit for bit, on inputs built to reach them
(tests/stereo_ref.py builds the inputs; tests/test_stereo_ref.py checks there, without a GPU, that each input has the property it exists for):

* goodFeaturesToTrack's minDistance selection (kernels_quad.hip): dependency chains far longer than the 1 + 12 launched rounds, more stronger
  neighbours than the 32-entry dependency list, windows wider than the bit-image scan, exact distance boundaries, exact ties and max_corners cuts
  inside them, and plateaus of equal eigenvalues with more candidates than the w*h/4 + 1024 list (selected on the pixel grid) -- through ssm_gftt,
  ssm_quad_track and a batch of ssm_stereo_seq_process;
* the SGBM post stages (sgbm_post.inc) through ssm_debug_sgbm_post: the int16 3x3 median and the two-level union-find of filterSpeckles on combs,
  spirals, serpentines, components of exactly maxSize, maxDiff boundaries, int16 extremes and dense random maps, every map as several frames of one
  launch (all frames must agree), and stacked frames that would join if their forests leaked into each other."""
import numpy as np
import pytest
import stereo_ref as R
from test_gpu_stereo_seq import stereo_sequence, reference_walk, check_against_walk, run_seq

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
