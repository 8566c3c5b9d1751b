"""The checker of tests/test_gpu_segnet_precision.py checked on the CPU: a numpy emulation of one conv3x3 + scale / shift + ReLU layer must PASS it when it
does what the contract says (fp32 accumulation in a shuffled order, one FMA, RNE to fp16) and FAIL it when it rounds toward zero, accumulates in fp16 or
stores bf16-precision outputs -- the bound and the correctly-rounded fraction can both go red.  The Winograd F(2, 3) emulation (fp16 U = G g from the fp32
weights, fp16 V = B^T d, fp32 sums) must pass with its widened bound and fail without it."""
import numpy as np
import pytest

import segnet_ref as S
from test_gpu_segnet_precision import EXACT_MIN, EXACT_MIN_WINO

H, W, CIN, COUT = 11, 13, 64, 32          # odd sizes: the Winograd pairs and the borders both clip


def case(seed=5):
    rng = np.random.default_rng(seed)
    x = np.maximum(rng.standard_normal((H, W, CIN)), 0).astype(np.float16)
    wt = (rng.standard_normal((COUT, CIN, 3, 3)) * np.sqrt(2.0 / (9 * CIN))).astype(np.float32)
    sc = (1.0 + 0.05 * rng.standard_normal(COUT)).astype(np.float32)
    sh = (0.05 * rng.standard_normal(COUT)).astype(np.float32)
    return x, wt, sc, sh


def taps(x):
    xp = np.zeros((H + 2, W + 2, CIN), np.float16); xp[1:-1, 1:-1] = x
    return xp


def epilogue(acc, sc, sh, out):
    """one FMA (acc x scale is exact in float64; the sum rounds once more on the way to fp32), the output conversion, ReLU"""
    y32 = (acc.astype(np.float64) * sc.astype(np.float64) + sh.astype(np.float64)).astype(np.float32)
    if out == "rne":
        h = y32.astype(np.float16)
    elif out == "rtz":
        h = y32.astype(np.float16)
        h = np.where(np.abs(h.astype(np.float32)) > np.abs(y32), np.nextafter(h, np.float16(0)), h)
    else:                                                     # bf16: RNE to 8 fraction bits
        b = y32.view(np.uint32)
        h = ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32).astype(np.float16)
    return np.maximum(h, np.float16(0))


def emulate_direct(x, wt, sc, sh, acc_dtype=np.float32, out="rne", seed=1):
    w16 = wt.astype(np.float16)
    xp = taps(x)
    terms = [(dy, dx, c) for dy in range(3) for dx in range(3) for c in range(CIN)]
    acc = np.zeros((H, W, COUT), acc_dtype)
    for t in np.random.default_rng(seed).permutation(len(terms)):      # fp16 x fp16 products are exact in fp32
        dy, dx, c = terms[t]
        p = xp[dy:dy + H, dx:dx + W, c, None].astype(np.float32) * w16[:, c, dy, dx].astype(np.float32)
        acc = (acc.astype(np.float32) + p).astype(acc_dtype)
    return epilogue(acc, sc, sh, out)


def emulate_wino(x, wt, sc, sh, seed=1):
    """conv3x3_wino_kernel's arithmetic: per dy, U0 = g0, U1 = (g0 + g1 + g2) / 2, U2 = (g0 - g1 + g2) / 2, U3 = g2 in fp32 -> fp16 (ssm_segnet_set_layer);
    V0 = d0 - d2, V1 = d1 + d2, V2 = d2 - d1, V3 = d1 - d3 in fp16; M_k summed in fp32; y[2j] = (M0 + M1) + M2, y[2j+1] = (M1 - M2) - M3"""
    g = wt.astype(np.float32)
    U = np.stack([g[..., 0], (g[..., 0] + g[..., 1] + g[..., 2]) * np.float32(0.5), (g[..., 0] - g[..., 1] + g[..., 2]) * np.float32(0.5), g[..., 2]]).astype(np.float16)
    Wp = W + (W & 1)
    xp = np.zeros((H + 2, Wp + 2, CIN), np.float16); xp[1:H + 1, 1:W + 1] = x
    d = [xp[:, k:k + Wp - 1:2] for k in range(4)]                 # d_k of pair j = column 2j - 1 + k (padded index 2j + k)
    V = [d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]]      # fp16 arithmetic in numpy rounds each result to fp16
    M = np.zeros((4, H, Wp // 2, COUT), np.float32)
    terms = [(dy, c) for dy in range(3) for c in range(CIN)]
    for t in np.random.default_rng(seed).permutation(len(terms)):
        dy, c = terms[t]
        for k in range(4):
            M[k] = M[k] + V[k][dy:dy + H, :, c, None].astype(np.float32) * U[k][:, c, dy].astype(np.float32)
    y = np.empty((H, Wp, COUT), np.float32)
    y[:, 0::2] = (M[0] + M[1]) + M[2]
    y[:, 1::2] = (M[1] - M[2]) - M[3]
    return epilogue(y[:, :W], sc, sh, "rne")


def verdict(got, x, wt, sc, sh, wino=False, exact_min=EXACT_MIN):
    y64, d = S.layer_ref(x, wt, sc, sh, relu=True, wino=wino)
    r = S.check_layer(got, y64, d)
    return (not r["bad"].any()) and r["exact"] >= exact_min, r


def test_checker_passes_fp32_accumulation_in_any_order():
    x, wt, sc, sh = case()
    for seed in (1, 2):
        ok, r = verdict(emulate_direct(x, wt, sc, sh, seed=seed), x, wt, sc, sh)
        assert ok, r
        assert r["margin"] < 0.75 and r["exact"] > 0.995


@pytest.mark.parametrize("kind", ["rtz", "fp16_acc", "bf16"])
def test_checker_fails_wrong_arithmetic(kind):
    x, wt, sc, sh = case()
    got = emulate_direct(x, wt, sc, sh, acc_dtype=np.float16 if kind == "fp16_acc" else np.float32, out="rne" if kind == "fp16_acc" else kind)
    ok, r = verdict(got, x, wt, sc, sh)
    assert not ok, r
    assert r["exact"] < 0.9, r                               # the sharper check alone already catches each of them


def test_checker_winograd_bound():
    x, wt, sc, sh = case()
    got = emulate_wino(x, wt, sc, sh)
    ok, r = verdict(got, x, wt, sc, sh, wino=True, exact_min=EXACT_MIN_WINO)
    assert ok, r
    ok_direct, r_direct = verdict(got, x, wt, sc, sh)
    assert not ok_direct, r_direct                           # the extra fp16 roundings do not fit the direct kernel's contract


def test_half_ulp16_and_overflow():
    assert S.half_ulp16(1.0) == 2.0 ** -11 and S.half_ulp16(1.999) == 2.0 ** -11 and S.half_ulp16(2.0) == 2.0 ** -10
    assert S.half_ulp16(0.0) == 2.0 ** -25 and S.half_ulp16(2.0 ** -20) == 2.0 ** -25 and S.half_ulp16(65504.0) == 16.0
    y = np.array([70000.0, -70000.0, 65519.0, 3.0])
    d = np.zeros(4)
    good = np.array([np.inf, -np.inf, 65504, 3.0], np.float16)
    assert not S.check_layer(good, y, d)["bad"].any()
    for wrong in ([65504, -np.inf, 65504, 3], [np.inf, -65504, 65504, 3], [np.inf, -np.inf, np.inf, 3], [np.inf, -np.inf, 65504, np.nan]):
        assert S.check_layer(np.array(wrong, np.float16), y, d)["bad"].any(), wrong
