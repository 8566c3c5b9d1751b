"""CPU tests of the contract the device LK is held to (tests/test_gpu_lk_edges.py compares the kernels with oracle/quad.c bit for bit): the C oracle's
pyramidal LK against the independent Python restatement tests/golden/pyref.py, computed live at the edges the golden file's 16 points do not reach, and
against ground truth the restatement cannot give: sub-pixel translations of analytic images.  Inputs: tests/lk_cases.py."""
import os
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import lk_cases as L          # noqa: E402
import pyref                  # noqa: E402

f32 = np.float32

# (w, h) -> top levels 4 x 4, 5 x 6 and 6 x 5; point counts 4k + 1, 4k + 2, 4k + 3 (a block of the device kernel tracks four points)
GRIDS = (((32, 32), 21), ((33, 47), 22), ((45, 37), 23))
# (max_count, epsilon, min_eig_threshold): the two of the issue and one with ten iterations at the defaults' epsilon
PARAMS = ((3, 0.3, 1e-3), (1, 0.0, 0.0), (10, 0.01, 1e-4))


def grid_case(w, h, n):
    prev = L.noise_image(w, h, 7 + w)
    return prev, L.shifted(prev, 1, -1, seed=3, amp=6), L.frac_grid(w, h, n, seed=w)


@pytest.mark.parametrize("size,n", GRIDS)
@pytest.mark.parametrize("params", PARAMS)
def test_oracle_lk_equals_restatement_at_the_edges(oracle, size, n, params):
    """points, status and err byte for byte, on grids of fractional points from 13 px outside the image (no window pixel inside) to 3 px past the far border:
    border reflection of the image taps, zeroed derivatives outside, the status-0 exits before and inside the iteration loop, small top levels"""
    prev, nxt, pts = grid_case(*size, n)
    assert len(pts) == n and (np.modf(pts)[0] != 0).any()
    o, os_, oe = oracle.lk_track(prev, nxt, pts, *params)
    assert (os_ == 1).sum() * 4 >= n and (os_ == 0).sum() >= 5, (int((os_ == 1).sum()), n)          # not vacuous: both outcomes occur
    p, ps, pe = pyref.lk_track(prev, nxt, pts, *params)
    assert np.array_equal(os_, ps) and o.tobytes() == p.tobytes() and oe.tobytes() == pe.tobytes()


def test_oracle_recovers_subpixel_translations(oracle):
    """Ground truth for the fractional weights: analytic band-limited images (lk_cases.Analytic, seed 11: 24 sinusoids, |frequency| <= 0.35 rad / px, 8 bits)
    moved by (0.37, -0.81), (3.25, 1.6), (-6.5, 2.75) and (11.3, -4.4) px at 131 x 96 and 203 x 70, tracked from fractional start points >= 24 px inside.
    Measured with oracle/quad.c (defaults: 200 iterations, epsilon 0.01): worst error 0.1653 px (203 x 70, (11.3, -4.4)), median of a case at most 0.024 px,
    every point status 1.  Asserted: 1.5 x the worst = 0.248 px (the margin covers another seed: seeds 12 and 13 give 0.215 and 0.123), median 0.05 px."""
    A = L.Analytic(11)
    worst = 0.0
    for (w, h) in L.ANALYTIC_SIZES:
        assert w % 4
        prev = A.sample(w, h); pts = L.interior_points(w, h, 24, 9, 11)
        assert len(pts) >= 50
        for (tx, ty) in L.TRANSLATIONS:
            out, st, _ = oracle.lk_track(prev, A.sample(w, h, tx, ty), pts)
            e = np.hypot(*(out.astype(np.float64) - pts - np.array([tx, ty])).T)
            print(f"{w} x {h} ({tx}, {ty}): worst {e.max():.4f} median {np.median(e):.4f}")
            assert (st == 1).all()
            assert e.max() <= L.SUBPIXEL_BOUND and np.median(e) <= 0.05, (w, h, tx, ty, e.max(), np.median(e))
            worst = max(worst, e.max())
    assert worst >= 0.5 * L.SUBPIXEL_WORST          # the recorded figure is this construction's (a stale one would loosen every bound derived from it)


def test_restatement_recovers_subpixel_translation():
    """the same truth for the Python restatement, on a handful of points of the smaller image (it is slow): it is the oracle's twin, not only on noise"""
    A = L.Analytic(11); w, h = L.ANALYTIC_SIZES[0]
    pts = L.interior_points(w, h, 40, 25, 3)[:5]
    tx, ty = L.TRANSLATIONS[1]
    out, st, _ = pyref.lk_track(A.sample(w, h), A.sample(w, h, tx, ty), pts, 30, 0.01, 1e-6)
    assert (st == 1).all() and np.hypot(*(out - pts - np.array([tx, ty])).T).max() <= L.SUBPIXEL_BOUND


def test_stripe_sums_reach_the_32_bit_limits(oracle):
    """Period-4 stripes (0, 0, 255, 255; rows pulled towards grey by 0 or 1 so that Iy is not zero): with integer arithmetic in Python integers, the window's
    sum of Ix^2 is 2.004e9 (93 % of 2^31; 2,014,214,400 without the row modulation) and, tracked into the stripes moved by one column, the full sum of
    (J - I) Ix is -2.185e9 for the windows that start on an even column: beyond 32 bits.  That sum is what the oracle computes: one iteration from the sums
    (float32 steps as in LKTrackerInvoker) gives the oracle's max_count = 1 result bit for bit at such points."""
    s, s1, pts = L.stripe_case()
    der = pyref.scharr(s)
    assert np.abs(der[2:-2, 2:-2, 0]).min() >= 16 * 253 and np.abs(der[..., 1]).max() > 0
    sums = [L.level0_sums(s, s1, p, der) for p in pts]
    print("max sum Ix^2 %d, max |sum (J - I) Ix| %d" % (max(v[0] for v in sums), max(abs(v[3]) for v in sums)))
    assert max(v[0] for v in sums) > 1.9e9 and max(v[0] for v in sums) < 2 ** 31
    out, st, _ = oracle.lk_track(s, s1, pts, 1, 0.0, 0.0)
    SC, half, proven = f32(1.0 / (1 << 20)), f32(5), 0
    for i, (p, (a, b, c, d, e)) in enumerate(zip(pts, sums)):
        if st[i] != 1 or abs(d) <= 2 ** 31:
            continue
        A11, A12, A22, b1, b2 = f32(f32(a) * SC), f32(f32(b) * SC), f32(f32(c) * SC), f32(f32(d) * SC), f32(f32(e) * SC)
        Dt = f32(f32(1) / f32(f32(A11 * A22) - f32(A12 * A12)))
        ddx = f32(f32(f32(A12 * b2) - f32(A22 * b1)) * Dt); ddy = f32(f32(f32(A12 * b1) - f32(A11 * b2)) * Dt)
        ex = np.array([f32(f32(f32(p[0] - half) + ddx) + half), f32(f32(f32(p[1] - half) + ddy) + half)], np.float32)
        proven += ex.tobytes() == out[i].tobytes()          # (a point the levels above moved before level 0 does not start at p: not counted)
    assert proven >= 5
    # and the whole track is the restatement's, at a few of those points (30 iterations)
    sel = [i for i, v in enumerate(sums) if abs(v[3]) > 2 ** 31][:3] + [0]
    o = oracle.lk_track(s, s1, pts[sel], 30, 0.01, 1e-6); p = pyref.lk_track(s, s1, pts[sel], 30, 0.01, 1e-6)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(o, p)) and np.isfinite(o[0]).all()


def test_diverging_tracks_stay_finite_and_equal(oracle):
    """binary noise tracked into its inverse: tracks run tens of pixels and leave the image in mid-iteration (the status-0 break inside the loop)"""
    w, h = 45, 37
    a = L.binary_noise(w, h, 3); pts = L.frac_grid(w, h, 13, 1)
    o = oracle.lk_track(a, 255 - a, pts, 10, 0.01, 1e-6); p = pyref.lk_track(a, 255 - a, pts, 10, 0.01, 1e-6)
    assert np.isfinite(o[0]).all() and np.hypot(*(o[0] - pts).T).max() > 20
    inside = (pts[:, 0] > 6) & (pts[:, 0] < w - 7) & (pts[:, 1] > 6) & (pts[:, 1] < h - 7)
    assert (inside & (o[1] == 0)).any()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(o, p))
