"""Inputs shared by tests/test_lk_ref.py (CPU: oracle/quad.c against tests/golden/pyref.py) and tests/test_gpu_lk_edges.py (device against oracle/quad.c):
images and point sets that reach the parts of pyramidal LK a GFTT corner list on a rolled image never does -- fractional bilinear weights at every level,
windows that start outside the image or leave it in mid-iteration, 4 x 4 top levels, window sums at the 32-bit limit.  numpy only."""
import numpy as np

LKW = 11

# the translations of the sub-pixel tests (x, y), and the sizes (w, h): widths that are no multiple of 4
TRANSLATIONS = ((0.37, -0.81), (3.25, 1.6), (-6.5, 2.75), (11.3, -4.4))
ANALYTIC_SIZES = ((131, 96), (203, 70))
# what oracle/quad.c's LK recovers of those translations at interior points (tests/test_lk_ref.py::test_oracle_recovers_subpixel_translations measures and
# asserts it): worst error over every point, size and translation, in pixels.  The bound of every sub-pixel assertion is 1.5 x this
SUBPIXEL_WORST = 0.1653         # median of a case: at most 0.024
SUBPIXEL_BOUND = 1.5 * SUBPIXEL_WORST


def noise_image(w, h, seed, smooth=True):
    """uniform noise over the full 8-bit range (every border reflection carries information); smooth: 3 x 3 box mean, stretched back to 0 .. 255, so that LK
    converges on it"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w)).astype(np.float64)
    if smooth:
        p = np.pad(a, 1, mode="reflect")
        a = sum(p[j:j + h, i:i + w] for j in range(3) for i in range(3)) / 9.0
        a = (a - a.min()) * (255.0 / (a.max() - a.min()))
    return np.rint(a).astype(np.uint8)


def shifted(img, dx, dy, seed=None, amp=0):
    """img moved by (dx, dy) whole pixels (np.roll), plus uniform noise of +-amp"""
    out = np.roll(np.roll(img, dx, axis=1), dy, axis=0).astype(np.int64)
    if amp:
        out = out + np.random.default_rng(seed).integers(-amp, amp + 1, img.shape)
    return np.clip(out, 0, 255).astype(np.uint8)


def frac_grid(w, h, n, seed=0):
    """n points with fractional coordinates on a jittered grid that reaches from 13 px outside the image (no window pixel inside: 13 > 11 / 2 + 5 + 1) to 3 px
    past the far border, the corners of that range included.  n is hit by thinning a grid of at least n points evenly"""
    rng = np.random.default_rng(seed)
    aspect = (w + 16.0) / (h + 16.0)
    gy = max(2, int(np.ceil(np.sqrt(n / aspect)))); gx = max(2, int(np.ceil(n / gy)))
    xs, ys = np.linspace(-13.0, w + 3.0, gx), np.linspace(-13.0, h + 3.0, gy)
    g = np.stack(np.meshgrid(xs, ys), 2).reshape(-1, 2)
    jit = rng.uniform(-0.49, 0.49, g.shape); jit[0] = jit[-1] = 0.0
    g = g + jit
    if n <= 5:                                      # a handful: along the diagonal, from a window that straddles the near corner to one at the far corner
        t = (np.arange(n) + 0.5) / n
        return np.ascontiguousarray(np.stack([-6.3 + t * (w + 8.0), -5.6 + t * (h + 9.0)], 1), np.float32)
    keep = np.unique(np.rint(np.linspace(0, len(g) - 1, n)).astype(int))
    assert len(keep) == n
    return np.ascontiguousarray(g[keep], np.float32)


class Analytic:
    """A band-limited image known at every real coordinate: 24 sinusoids with |frequency| <= 0.35 rad / px (wavelength >= 18 px, far below the 8-bit
    pyramid's aliasing), quantised to 8 bits only at the end.  sample(w, h, tx, ty) is the image moved by (tx, ty): a point p of sample(w, h) lies at
    p + (tx, ty) in it, whatever the fraction."""

    def __init__(self, seed, n=24, fmax=0.35):
        rng = np.random.default_rng(seed)
        r = fmax * np.sqrt(rng.uniform(0.15, 1.0, n)); th = rng.uniform(0, 2 * np.pi, n)
        self.fx, self.fy = r * np.cos(th), r * np.sin(th)
        self.ph = rng.uniform(0, 2 * np.pi, n); self.amp = rng.uniform(0.5, 1.0, n)
        self.norm = 110.0 / self.amp.sum()

    def sample(self, w, h, tx=0.0, ty=0.0):
        x = np.arange(w, dtype=np.float64)[None, :, None] - tx; y = np.arange(h, dtype=np.float64)[:, None, None] - ty
        v = (self.amp * np.sin(self.fx * x + self.fy * y + self.ph)).sum(2)
        return np.clip(np.rint(128.0 + self.norm * v), 0, 255).astype(np.uint8)


def interior_points(w, h, margin, step, seed):
    """fractional start points at least `margin` px from every border"""
    rng = np.random.default_rng(seed)
    xs, ys = np.arange(margin, w - margin + 1e-9, step), np.arange(margin, h - margin + 1e-9, step)
    g = np.stack(np.meshgrid(xs, ys), 2).reshape(-1, 2)
    return np.ascontiguousarray(g + rng.uniform(0.0, 0.999, g.shape), np.float32)


def stripes(w, h, seed, depth=1):
    """Vertical stripes of period 4 (0, 0, 255, 255): |Ix| = 16 * 255 at every interior pixel, the largest a Scharr derivative gets.  Each row is pulled
    towards grey by m(y) in 0 .. depth (dark columns m, bright ones 255 - m) so that Iy is not zero everywhere and the 2 x 2 matrix is regular."""
    m = np.random.default_rng(seed).integers(0, depth + 1, h)[:, None]
    bright = ((np.arange(w) >> 1) & 1).astype(bool)[None, :]
    return np.where(bright, 255 - m, m).astype(np.uint8)


def level0_sums(prev, nxt, pt, der):
    """The integer sums of LK's FIRST level-0 iteration for an integer point pt = (x, y) whose window lies inside the image, started at pt itself (bilinear
    weights 16384, 0, 0, 0: I = 32 p, Ix, Iy = the Scharr derivatives `der` of prev, h x w x 2), in Python integers: sum Ix^2, sum Ix Iy, sum Iy^2, sum (J - I) Ix, sum (J - I) Iy"""
    x0, y0 = int(pt[0]) - LKW // 2, int(pt[1]) - LKW // 2
    h, w = prev.shape
    assert float(pt[0]) == int(pt[0]) and float(pt[1]) == int(pt[1]) and x0 >= 0 and y0 >= 0 and x0 + LKW < w and y0 + LKW < h
    d = der[y0:y0 + LKW, x0:x0 + LKW].astype(np.int64)
    ix, iy = [int(v) for v in d[:, :, 0].ravel()], [int(v) for v in d[:, :, 1].ravel()]
    diff = [32 * (int(b) - int(a)) for a, b in zip(prev[y0:y0 + LKW, x0:x0 + LKW].ravel(), nxt[y0:y0 + LKW, x0:x0 + LKW].ravel())]
    return (sum(a * a for a in ix), sum(a * b for a, b in zip(ix, iy)), sum(b * b for b in iy),
            sum(e * a for e, a in zip(diff, ix)), sum(e * b for e, b in zip(diff, iy)))


def binary_noise(w, h, seed):
    return (np.random.default_rng(seed).integers(0, 2, (h, w)) * 255).astype(np.uint8)


def checker2(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return ((((x >> 1) + (y >> 1)) & 1) * 255).astype(np.uint8)


def stripe_case(w=64, h=48, seed=5):
    """(stripes, stripes moved one column to the right, integer points whose windows lie inside the image, on every phase of the stripes)"""
    s = stripes(w, h, seed)
    pts = np.array([[x, y] for y in (8, 17, 24, h - 8) for x in range(7, w - 7, 3)], np.float32)
    return s, np.roll(s, 1, axis=1), pts
