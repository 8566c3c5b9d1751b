"""SegNet layers on REAL-VALUED data against float64 (the per-op tests of test_gpu_segnet.py use small integers, on which fp16 storage, fp32
accumulation and the fp32 -> fp16 conversion are all exact: they check indexing, not arithmetic).

Contract (include/ssm_hip.h, DESIGN.md s.2 "SegNet numerics"): fp16 operands (weights rounded to fp16 with RNE), fp32 accumulation, one fp32 FMA for the
folded BN scale / shift, IEEE fp16 round-to-nearest-even of the result with subnormals kept and overflow to +-inf, ReLU (-inf -> 0) on every layer but 25.
Checked per element against y64 = scale * conv_float64(x16, w16) + shift with the bound of segnet_ref.check_layer, and -- because that bound must hold for
every summation order and is loose -- by the fraction of non-zero outputs equal to float16(y64), which round-toward-zero or a narrower accumulator
(tests/test_segnet_checker.py) would take to about one half.  SSM_CONV_WINOGRAD=1 (test_gpu_segnet.py::test_winograd_conv_kernel_passes_the_same_tests)
runs the plain conv layers 1 .. 24 through the Winograd kernel, with the bound widened by one fp16 rounding of U = G g and of V = B^T d."""
import numpy as np
import pytest

import segnet_ref as S

pytestmark = pytest.mark.gpu

# Fraction of the non-zero outputs that must equal float16(y64), and the mean signed error in half-ulps (check_layer's "bias").  Measured on the MI355X
# (every test prints both): direct kernel, lowest fraction 0.99776 (layer 10, 512 channels: fp32 accumulation misrounds 0.22 %), |bias| <= 0.005.  Thresholds:
# 0.995 (twice the measured misround share) and |bias| <= 0.05; round-toward-zero output gives about 0.5 and -1.  The Winograd variant measured 0.440 .. 0.537
# (layers 1 .. 24) with a bias of +0.17 .. +1.0 half-ulps: its U = G g is rounded from the fp32 weights, not from the fp16 ones the reference (and the direct
# kernel) multiply with, and each fp16 V = B^T d adds about half an ulp of noise; threshold 0.40, no bias check (its own bound still holds, at <= 0.04 of it).
EXACT_MIN = 0.995
BIAS_MAX = 0.05
EXACT_MIN_WINO = 0.40

def exact_min(wino):
    return EXACT_MIN_WINO if wino else EXACT_MIN


@pytest.fixture(scope="module")
def seeded(ctx):
    w = S.make_weights(1234)
    for l, (wt, sc, sh) in enumerate(w):
        ctx.segnet_set_layer(l, wt, sc, sh)
    yield w
    for l, (wt, sc, sh) in enumerate(w):                    # the tests below load scaled copies: leave the seeded net behind
        ctx.segnet_set_layer(l, wt, sc, sh)


def activations(rng, h, w, c, layer):
    """the domain of a layer's input: post-ReLU |N(0,1)|-like values with about half zeros, fp16; layer 0 gets its real 0..255 integers"""
    if layer == 0:
        return rng.integers(0, 256, (h, w, c)).astype(np.float16)
    return np.maximum(rng.standard_normal((h, w, c)), 0).astype(np.float16)


def conv_padded(ctx, layer, x):
    """debug op 0 with every stored output channel (segnet_debug_conv drops the padding ones); the output buffer starts as NaN"""
    from semantic_slam_mapping_amd.api import _ptr
    cin, cout, _, _ = ctx.segnet_layers()[layer]
    h, w = x.shape[:2]
    xin = np.zeros((h, w, (cin + 15) // 16 * 16), np.float16); xin[:, :, :cin] = x
    out = np.full((h, w, (cout + 15) // 16 * 16), np.nan, np.float16)
    ctx._chk(ctx.lib.ssm_segnet_debug_op(ctx.h, 0, layer, _ptr(xin), h, w, _ptr(out), None))
    return out


def run_layer(ctx, layer, x, wt, sc, sh, what):
    """one layer through debug op 0 against float64; returns the check_layer dict"""
    cin, cout, _, _ = ctx.segnet_layers()[layer]
    wino = S.wino_active(cin, cout)
    ctx.segnet_set_layer(layer, wt, sc, sh)
    out = conv_padded(ctx, layer, x)
    y64, d = S.layer_ref(x, wt, sc, sh, relu=layer != 25, wino=wino)
    r = S.check_layer(out[:, :, :cout], y64, d)
    print(f"segnet precision {what} layer {layer:2d} {x.shape[0]}x{x.shape[1]}{' wino' if wino else ''}: exact {r['exact']:.5f} margin {r['margin']:.3f} bias {r['bias']:+.3f} "
          f"inf {r['n_inf']} bad {int(r['bad'].sum())}")
    assert not r["bad"].any(), f"{int(r['bad'].sum())} outputs outside the bound, first at {np.argwhere(r['bad'])[0]}"
    assert (out[:, :, cout:] == 0).all(), "padding output channels must be 0"
    assert r["exact"] >= exact_min(wino), f"only {r['exact']:.5f} of the outputs are correctly rounded"
    assert wino or abs(r["bias"]) <= BIAS_MAX, f"mean signed error {r['bias']:+.3f} half-ulps: not round-to-nearest"
    return r, out[:, :, :cout], y64


@pytest.mark.parametrize("layer", range(26))
def test_layer_against_float64(ctx, seeded, layer):
    """every layer at its production size with the seeded weights, on inputs shaped like its real ones"""
    cin, _, h, w = ctx.segnet_layers()[layer]
    x = activations(np.random.default_rng(7000 + layer), h, w, cin, layer)
    try:
        run_layer(ctx, layer, x, *seeded[layer], "seeded")
    finally:
        ctx.segnet_set_layer(layer, *seeded[layer])


@pytest.mark.parametrize("layer", [1, 3, 6, 9, 12])
def test_conv_pool_fused_against_float64(ctx, seeded, layer):
    """debug op 3 (conv + BN + ReLU + 2x2 max-pool in one kernel, always the direct conv): each pooled value within the bound of its window's maximum of
    y64, each arg-max code on an element whose y64 is within twice the bound of that maximum, and the fused result bit-equal to conv -> pool"""
    cin, cout, h, w = ctx.segnet_layers()[layer]
    x = activations(np.random.default_rng(7100 + layer), h, w, cin, layer)
    wt, sc, sh = seeded[layer]
    p, code = ctx.segnet_debug_conv_pool(layer, x)
    y64, d = S.layer_ref(x, wt, sc, sh, relu=True)
    tol = S.half_ulp16(np.abs(y64) + d) + d
    PH, PW = (h + 1) // 2, (w + 1) // 2
    win = np.full((PH, PW, 4, cout), -np.inf); wtol = np.zeros((PH, PW, 4, cout))
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        ys, xs = slice(dy, h, 2), slice(dx, w, 2)
        win[:y64[ys, xs].shape[0], :y64[ys, xs].shape[1], k] = y64[ys, xs]            # clipped windows at odd sizes keep -inf
        wtol[:y64[ys, xs].shape[0], :y64[ys, xs].shape[1], k] = tol[ys, xs]
    m = win.max(axis=2)
    dmax = wtol.max(axis=2)                                                             # the widest bound in the window (max is monotonic)
    err = np.abs(p.astype(np.float64) - m)
    print(f"segnet precision conv+pool layer {layer:2d}: max |pooled - max y64| / bound {float((err / dmax).max()):.3f}")
    assert (err <= dmax).all()
    assert code.max() <= 3
    picked = np.take_along_axis(win, code[:, :, None, :].astype(np.int64), axis=2)[:, :, 0]
    assert np.isfinite(picked).all(), "a code points outside a clipped window"
    assert (m - picked <= 2 * dmax).all()
    if not S.wino_active(cin, cout):                     # op 0 runs the Winograd kernel under SSM_CONV_WINOGRAD=1, op 3 the direct one
        p_ref, c_ref = ctx.segnet_debug_pool(ctx.segnet_debug_conv(layer, x))
        assert np.array_equal(p, p_ref) and np.array_equal(code, c_ref)


@pytest.mark.parametrize("layer", [13, 16, 19, 22, 24])
def test_unpool_conv_fused_against_float64(ctx, seeded, layer):
    """debug op 4 (un-pool on load + conv + BN + ReLU, always the direct conv) against float64 applied to the un-pooled tensor; codes drawn per element
    and clipped to the image at odd sizes, as a real pooling leaves them"""
    cin, cout, h, w = ctx.segnet_layers()[layer]
    rng = np.random.default_rng(7200 + layer)
    PH, PW = (h + 1) // 2, (w + 1) // 2
    pooled = activations(rng, PH, PW, cin, layer)
    dy = rng.integers(0, 2, (PH, PW, cin)); dx = rng.integers(0, 2, (PH, PW, cin))
    yy, xx = np.meshgrid(np.arange(PH), np.arange(PW), indexing="ij")
    dy = np.where(2 * yy[:, :, None] + 1 < h, dy, 0); dx = np.where(2 * xx[:, :, None] + 1 < w, dx, 0)
    code = (2 * dy + dx).astype(np.uint8)
    up = np.zeros((h, w, cin), np.float16)
    for a in range(2):
        for b in range(2):
            sub = up[a::2, b::2]
            sub[...] = np.where(code[:sub.shape[0], :sub.shape[1]] == 2 * a + b, pooled[:sub.shape[0], :sub.shape[1]], 0)
    wt, sc, sh = seeded[layer]
    out = ctx.segnet_debug_unpool_conv(layer, pooled, code, h, w)
    y64, d = S.layer_ref(up, wt, sc, sh, relu=True)
    r = S.check_layer(out, y64, d)
    print(f"segnet precision unpool+conv layer {layer:2d} {h}x{w}: exact {r['exact']:.5f} margin {r['margin']:.3f} bias {r['bias']:+.3f}")
    assert not r["bad"].any()
    assert r["exact"] >= EXACT_MIN and abs(r["bias"]) <= BIAS_MAX


@pytest.mark.parametrize("layer", [2, 18, 25])
def test_subnormal_outputs(ctx, seeded, layer):
    """scale and shift times 2^-20: most outputs fall in the fp16 subnormal range (half an ulp = 2^-25 there); a kernel that flushes them, or converts
    with a different rounding, is off by a whole subnormal step"""
    cin, _, h, w = ctx.segnet_layers()[layer]
    h, w = min(h, 45), min(w, 61)
    wt, sc, sh = seeded[layer]
    x = activations(np.random.default_rng(7300 + layer), h, w, cin, layer)
    try:
        r, out, y64 = run_layer(ctx, layer, x, wt, sc * np.float32(2.0 ** -20), sh * np.float32(2.0 ** -20), "subnormal-out")
    finally:
        ctx.segnet_set_layer(layer, wt, sc, sh)
    sub = (out != 0) & (np.abs(out.astype(np.float64)) < 2.0 ** -14)
    assert sub.mean() > 0.3, f"only {sub.mean():.3f} of the outputs are subnormal: the case does not test what it says"


@pytest.mark.parametrize("layer", [1, 25])
def test_subnormal_inputs(ctx, seeded, layer):
    """inputs in the fp16 subnormal range (|N(0,1)| x 2^-17), scale x 2^14 so that the outputs are normal again: subnormal operands must not be flushed"""
    cin, _, h, w = ctx.segnet_layers()[layer]
    h, w = min(h, 45), min(w, 61)
    wt, sc, sh = seeded[layer]
    x = (np.maximum(np.random.default_rng(7400 + layer).standard_normal((h, w, cin)), 0) * 2.0 ** -17).astype(np.float16)
    nz = x[x != 0]
    assert (np.abs(nz.astype(np.float32)) < 2.0 ** -14).mean() > 0.95
    try:
        r, out, _ = run_layer(ctx, layer, x, wt, sc * np.float32(2.0 ** 14), sh, "subnormal-in")
    finally:
        ctx.segnet_set_layer(layer, wt, sc, sh)
    assert np.abs(out.astype(np.float32)).max() > 2.0 ** -10


@pytest.mark.parametrize("layer", [2, 25])
def test_overflow_to_inf(ctx, seeded, layer):
    """scale x 2^15: part of the outputs pass 65504.  RNE takes |y| >= 65520 to +-inf; after the ReLU -inf becomes 0 (layer 2); layer 25 has no ReLU and
    must give both signs of inf"""
    cin, _, h, w = ctx.segnet_layers()[layer]
    h, w = min(h, 45), min(w, 61)
    wt, sc, sh = seeded[layer]
    x = activations(np.random.default_rng(7500 + layer), h, w, cin, layer)
    try:
        r, out, y64 = run_layer(ctx, layer, x, wt, sc * np.float32(2.0 ** 15), sh, "overflow")
    finally:
        ctx.segnet_set_layer(layer, wt, sc, sh)
    assert (out == np.inf).sum() > 10 and (np.isfinite(out) & (out != 0)).sum() > 10
    if layer == 25:
        assert (out == -np.inf).sum() > 10
    else:
        assert not (out == -np.inf).any() and (y64 == 0).sum() > 10


def test_fused_argmax_rounds_like_the_stored_logits(ctx, seeded):
    """debug op 5 (the last layer's conv + scale / shift + class ArgMax in one epilogue: the labels of ssm_segnet_forward_dev) on logits built to sit on
    fp16 midpoints: the only weight is the centre tap of input channel 0 (acc = x exactly), class 0 has scale 1 + 2^-11 and shift +2^-30, class 1
    scale 1 + 2^-10, the others one of those or 1.  The fp32 FMA rounds x (1 + 2^-11) + 2^-30 back onto the midpoint x (1 + 2^-11), which RNE takes to
    the even neighbour; rounding the FMA straight to fp16 (v_fma_mixlo_f16) takes it up instead, a tie with class 1 that the first maximum gives to
    class 0.  The labels must be the first maximum of the stored fp16 logits (debug op 0, the argmax_kernel path) and of the contract's model"""
    layer, (h, w) = 25, (37, 45)
    cin, cout, _, _ = ctx.segnet_layers()[layer]
    rng = np.random.default_rng(7600)
    wt = np.zeros((cout, cin, 3, 3), np.float32); wt[:, 0, 1, 1] = 1.0
    sc = np.ones(cout, np.float32); sh = np.zeros(cout, np.float32)
    sc[0], sh[0], sc[1] = 1 + 2.0 ** -11, 2.0 ** -30, 1 + 2.0 ** -10
    for c in range(2, cout):
        sc[c], sh[c] = [(1 + 2.0 ** -11, 2.0 ** -30), (1 + 2.0 ** -11, -2.0 ** -30), (1 + 2.0 ** -10, 0.0), (1.0, 0.0)][rng.integers(0, 4)]
    x = rng.standard_normal((h, w, cin)).astype(np.float16)
    x[:, :, 0] = rng.choice(np.array([0.5, 1, 2, 3, 4, 5, 8, 16, 24, 64, 96, 256], np.float16), (h, w))
    exact = x[:, :, :1].astype(np.float64) * sc.astype(np.float64) + sh.astype(np.float64)      # exact in float64: 12 + 11 bits and the 2^-30
    contract = exact.astype(np.float32).astype(np.float16)                                      # fp32 FMA, then RNE to fp16
    once = exact.astype(np.float16)                                                             # rounded once, straight to fp16
    assert (contract.argmax(2) != once.argmax(2)).sum() > 100, "the case must tell the two roundings apart"
    try:
        ctx.segnet_set_layer(layer, wt, sc, sh)
        logits = ctx.segnet_debug_conv(layer, x)
        labels = ctx.segnet_debug_conv_argmax(layer, x)
    finally:
        ctx.segnet_set_layer(layer, *seeded[layer])
    assert np.array_equal(logits, contract), "stored logits"
    diff = labels != contract.argmax(2)
    assert not diff.any(), f"{int(diff.sum())} fused labels differ from the first maximum of the stored logits, e.g. at {np.argwhere(diff)[0].tolist()}"
