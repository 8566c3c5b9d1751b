"""Depth from stereo (oracle/sgbm.c, kernels_sgbm.hip): cv::StereoSGBM as /root/reference/src/stereo.cpp:11-30 configures it +
FrameReader's disparity -> depth conversion (/root/reference/src/rgbdframe.cpp:81-116).  CPU: properties of the oracle on
synthetic rectified pairs with known disparity.  GPU: every stage against the oracle, bit for bit."""
import numpy as np
import pytest

KITTI = dict(baseline=0.532331858, cu=607.1928, cv=185.2157, f=718.856, roix=20.0, roiy=5.0, roiz=40.0, scale=1000.0)   # parameters.txt:37-63


def stereo_pair(h, w, seed, planes=((20, None), (45, (0.3, 0.75, 0.3, 0.7))), noise=0):
    """textured right image; the left image shows the same texture shifted by the disparity of fronto-parallel planes"""
    rng = np.random.default_rng(seed)
    tex = rng.integers(0, 256, (h, w + 160)).astype(np.float32)
    k = np.array([1, 4, 6, 4, 1], np.float32); k /= k.sum()
    for ax in (0, 1):
        tex = np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), ax, tex)
    tex = ((tex - tex.min()) / (tex.max() - tex.min()) * 255).astype(np.uint8)
    dmap = np.zeros((h, w), np.int32)
    for d, box in planes:
        if box is None:
            dmap[:] = d
        else:
            y0, y1, x0, x1 = int(box[0] * h), int(box[1] * h), int(box[2] * w), int(box[3] * w)
            dmap[y0:y1, x0:x1] = d
    right = tex[:, 80:80 + w].copy()
    xs = np.arange(w)[None, :] - dmap + 80
    left = np.take_along_axis(tex, xs, axis=1)
    if noise:
        left = np.clip(left.astype(np.int32) + rng.integers(-noise, noise + 1, left.shape), 0, 255).astype(np.uint8)
    return left, right, dmap


def test_oracle_recovers_plane_disparities(oracle):
    left, right, dmap = stereo_pair(96, 320, 0)
    d = oracle.sgbm(left, right, oracle.sgbm_params())
    assert d.dtype == np.int16 and (d[:, :80] == -16).all()                     # columns < numberOfDisparities are never matched
    bg = d[5:25, 120:300]; fg = d[35:65, 130:210]
    assert np.median(bg) == 20 * 16 and np.median(fg) == 45 * 16
    assert (np.abs(bg[bg != -16] - 320) <= 8).mean() > 0.99
    raw = oracle.sgbm(left, right, oracle.sgbm_params(), raw=True)
    assert np.array_equal(oracle.filter_speckles(oracle.median3_s16(raw), -16, 100, 512), d)
    # too few columns for any disparity: everything invalid
    assert (oracle.sgbm(left[:, :60], right[:, :60], oracle.sgbm_params()) == -16).all()
    with pytest.raises(ValueError):
        oracle.sgbm(left, right, oracle.sgbm_params(num_disp=40))                # not a multiple of 16


def test_oracle_speckle_and_median(oracle):
    img = np.full((40, 50), -16, np.int16)
    img[5:8, 5:8] = 300                      # 9-pixel blob: removed at maxSpeckleSize 10
    img[20:30, 10:40] = 500                  # 300-pixel region: kept
    img[22, 12] = 500 + 600                  # differs by more than maxDiff from its neighbours: a 1-pixel component
    out = oracle.filter_speckles(img, -16, 10, 512)
    assert (out[5:8, 5:8] == -16).all() and out[22, 12] == -16 and (out[20:30, 10:40] == 500).sum() == 299
    r = np.random.default_rng(1).integers(-16, 1000, (17, 23)).astype(np.int16)
    m = oracle.median3_s16(r)
    p = np.pad(r, 1, mode="edge")
    ref = np.median(np.stack([p[i:i + 17, j:j + 23] for i in range(3) for j in range(3)]), axis=0).astype(np.int16)
    assert np.array_equal(m, ref)


def test_oracle_depth_conversion(oracle):
    disp = np.full((20, 40), -16, np.int16)
    disp[5, 10] = 320; disp[6, 11] = 0; disp[7, 12] = 16 * 2                     # 20 px -> 19.1 m; zero; 2 px -> 191 m (outside roiz)
    depth = oracle.disparity_to_depth(disp, **KITTI)
    z = KITTI["f"] * KITTI["baseline"] / 320.0 * 16.0
    assert depth[5, 10] == int(z * 1000.0) and depth[6, 11] == 0 and depth[7, 12] == 0
    assert (depth[disp == -16] == 0).all()                                        # the minimum value of the image is "no measurement"


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,num_disp,sad,seed,noise", [(96, 320, 80, 11, 0, 0), (64, 200, 64, 5, 1, 6), (50, 150, 32, 3, 2, 0),
                                                          (120, 400, 80, 11, 3, 10), (37, 181, 48, 7, 4, 3), (30, 140, 128, 9, 5, 2),
                                                          (40, 120, 16, 5, 6, 0), (44, 230, 96, 7, 7, 4)])
def test_gpu_sgbm_bit_exact(ctx, oracle, h, w, num_disp, sad, seed, noise):
    left, right, _ = stereo_pair(h, w, seed, planes=((num_disp // 4, None), (num_disp // 2 + 3, (0.3, 0.75, 0.3, 0.7))), noise=noise)
    po = oracle.sgbm_params(num_disp=num_disp, sad=sad)
    pg = ctx.sgbm_params(numberOfDisparities=num_disp, SADWindowSize=sad)
    assert np.array_equal(po, pg)
    raw_o = oracle.sgbm(left, right, po, raw=True); raw_g = ctx.sgbm(left, right, pg, raw=True)
    assert np.array_equal(raw_g, raw_o), f"{(raw_g != raw_o).sum()} of {raw_o.size} raw disparities differ"
    assert np.array_equal(ctx.sgbm(left, right, pg), oracle.sgbm(left, right, po))
    assert (raw_o != (-16)).any()


@pytest.mark.gpu
def test_gpu_sgbm_options_and_depth(ctx, oracle):
    left, right, _ = stereo_pair(80, 300, 7, noise=4)
    for kw_o, kw_g in ((dict(uniqueness=0, disp12=2), dict(uniquenessRatio=0, disp12MaxDiff=2)),
                       (dict(speckle_window=0), dict(speckleWindowSize=0)),
                       (dict(prefilter_cap=10, p1=50, p2=800, speckle_window=30, speckle_range=2), dict(preFilterCap=10, P1=50, P2=800, speckleWindowSize=30, speckleRange=2))):
        assert np.array_equal(ctx.sgbm(left, right, ctx.sgbm_params(**kw_g)), oracle.sgbm(left, right, oracle.sgbm_params(**kw_o)))
    depth, disp = ctx.stereo_depth(left, right, **KITTI)
    ref_disp = oracle.sgbm(left, right, oracle.sgbm_params())
    assert np.array_equal(disp, ref_disp)
    assert np.array_equal(depth, oracle.disparity_to_depth(ref_disp, **KITTI))
    assert (depth > 0).sum() > 1000
    from semantic_slam_mapping_amd.api import SsmError
    with pytest.raises(SsmError):
        ctx.sgbm(left, right, ctx.sgbm_params(numberOfDisparities=40))
    assert (ctx.sgbm(left[:, :70], right[:, :70]) == -16).all()                  # fewer columns than disparities


@pytest.mark.gpu
def test_gpu_sgbm_kitti_size(ctx, oracle):
    """configs[3] geometry: 1241 x 376, 80 disparities"""
    left, right, _ = stereo_pair(376, 1241, 11, planes=((12, None), (30, (0.4, 0.9, 0.2, 0.5)), (60, (0.5, 0.95, 0.6, 0.8))), noise=5)
    g = ctx.sgbm(left, right)
    assert np.array_equal(g, oracle.sgbm(left, right, oracle.sgbm_params()))


def _sgbm_in_subprocess(tmp_path, env, cases):
    """the SGBM form / strip width are read once per process: run the library in a child with the given environment"""
    import os, subprocess, sys
    np.savez(tmp_path / "in.npz", **{f"{k}{i}": v for i, (l, r, _, _) in enumerate(cases) for k, v in (("l", l), ("r", r))})
    code = ("import numpy as np, semantic_slam_mapping_amd as ssm\n"
            f"g = np.load(r'{tmp_path / 'in.npz'}')\n"
            "c = ssm.Context(0, width=640, height=480, max_batch=1)\n"
            f"P = {[(nd, sad) for _, _, nd, sad in cases]!r}\n"
            "out = {}\n"
            "for i, (nd, sad) in enumerate(P):\n"
            "    out[f'd{i}'] = c.sgbm(g[f'l{i}'], g[f'r{i}'], c.sgbm_params(numberOfDisparities=nd, SADWindowSize=sad))\n"
            "    out[f'raw{i}'] = c.sgbm(g[f'l{i}'], g[f'r{i}'], c.sgbm_params(numberOfDisparities=nd, SADWindowSize=sad), raw=True)\n"
            "c.sync()\n"
            f"np.savez(r'{tmp_path / 'out.npz'}', **out); c.close()\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=root, **env), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(tmp_path / "out.npz")


@pytest.mark.gpu
@pytest.mark.parametrize("env", [dict(SSM_SGBM_FORM="0"), dict(SSM_SGBM_FORM="1"), dict(SSM_SGBM_FORM="2", SSM_SGBM_STRIP="8"), dict(SSM_SGBM_FORM="2", SSM_SGBM_STRIP="34")])
def test_gpu_sgbm_forms_stay_equal(oracle, tmp_path, env):
    """Three formulations of the five scan directions live in the library (kernels_sgbm.hip, SSM_SGBM_FORM): 0 = five L volumes + sgbm_wta,
    1 = four L volumes + the column direction with the winner pass inside (round 3), 2 = the default:
    sgbm_rows (both row directions -> one summed volume) + sgbm_sweep (three directions + winner pass, strips of columns handing their diagonal states
    on through mailboxes).  All must produce the oracle's bits; SSM_SGBM_STRIP narrows the sweep's strips so that small images have many seams
    (8 columns: every wave holds both strip edges; 34: strips that do not divide the width).  The sweep has two kernels: eight lanes per pixel and sixteen
    (what D = 128 uses: the 8-lane kernel's exchange buffers do not fit there -- case 4 below); the row kernel is sgbm_rows8 (eight disparities per lane, one aligned
    16-byte word; checkpoints every 12 columns).  The env-selected variants of both (16-lane rows, 16-lane sweep at every D, 8- / 16-column checkpoints) were
    measured slower in rounds 4 - 5 and removed in round 6."""
    cases = []
    for (h, w, nd, sad, seed, noise) in [(72, 260, 64, 7, 5, 4), (50, 150, 32, 3, 2, 0), (61, 333, 80, 11, 9, 6), (40, 120, 16, 5, 6, 0), (44, 300, 128, 9, 8, 3), (33, 170, 48, 5, 3, 2)]:
        l, r, _ = stereo_pair(h, w, seed, planes=((nd // 4, None), (nd // 2 + 3, (0.3, 0.75, 0.3, 0.7))), noise=noise)
        cases.append((l, r, nd, sad))
    got = _sgbm_in_subprocess(tmp_path, env, cases)
    for i, (l, r, nd, sad) in enumerate(cases):
        po = oracle.sgbm_params(num_disp=nd, sad=sad)
        raw_o = oracle.sgbm(l, r, po, raw=True)
        assert np.array_equal(got[f"raw{i}"], raw_o), f"case {i} ({env}): {(got[f'raw{i}'] != raw_o).sum()} of {raw_o.size} raw disparities differ"
        assert np.array_equal(got[f"d{i}"], oracle.sgbm(l, r, po)), f"case {i} ({env})"


@pytest.mark.gpu
def test_gpu_sgbm_form_is_a_context_setting(oracle):
    """ssm_config.sgbm_form: three contexts of ONE process run the three formulations (1: four path volumes, 2: rows + sweep, 3: five path volumes) and agree with the
    oracle -- the maintainer-facing knob is configuration, not environment"""
    import semantic_slam_mapping_amd as ssm
    cases = []
    for (h, w, nd, sad, seed, noise) in [(72, 260, 64, 7, 5, 4), (61, 333, 80, 11, 9, 6), (44, 300, 128, 9, 8, 3)]:
        l, r, _ = stereo_pair(h, w, seed, planes=((nd // 4, None), (nd // 2 + 3, (0.3, 0.75, 0.3, 0.7))), noise=noise)
        cases.append((l, r, nd, sad))
    ctxs = [ssm.Context(0, width=640, height=480, max_batch=1, sgbm_form=f) for f in (1, 2, 3)]
    try:
        for l, r, nd, sad in cases:
            ref = oracle.sgbm(l, r, oracle.sgbm_params(num_disp=nd, sad=sad))
            for c in ctxs:
                assert np.array_equal(c.sgbm(l, r, c.sgbm_params(numberOfDisparities=nd, SADWindowSize=sad)), ref), c.cfg.sgbm_form
        with pytest.raises(ssm.SsmError):
            ssm.Context(0, width=640, height=480, max_batch=1, sgbm_form=4)
    finally:
        for c in ctxs:
            c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("hook", ["1", "2"])
def test_gpu_sgbm_sweep_timeout_falls_back_to_form_1(oracle, tmp_path, hook):
    """cv::StereoSGBM cannot fail (src/stereo.cpp:11-30).  The sweep of form 2 can time out in a strip hand-off: SSM_SGBM_TEST_TIMEOUT=1 makes every sweep report one, =2
    makes the occupancy check in front of the sweep say that its strips cannot all be resident.  Either way the call must return the oracle's disparities (repeated / run
    in form 1) -- both per-pair entry points (ssm_sgbm and ssm_stereo_depth share one repeat loop, sgbm_pair) and the batched path (whose failure is only known
    at ssm_sync), there with a note in ssm_last_error"""
    import os, subprocess, sys
    h, w, n = 61, 333, 5
    pairs = [stereo_pair(h, w, 20 + k, planes=((20, None), (43, (0.3, 0.75, 0.3, 0.7))), noise=3) for k in range(n)]
    L = np.stack([p[0] for p in pairs]); R = np.stack([p[1] for p in pairs])
    np.savez(tmp_path / "in.npz", L=L, R=R)
    code = ("import numpy as np, semantic_slam_mapping_amd as ssm\n"
            f"g = np.load(r'{tmp_path / 'in.npz'}'); L, R = g['L'], g['R']; n, h, w = L.shape\n"
            "c = ssm.Context(0, width=640, height=480, max_batch=2)\n"
            "out = {'pair': c.sgbm(L[0], R[0]), 'note_pair': np.array(c.last_error())}\n"
            "out['pd_depth'], out['pd_disp'] = c.stereo_depth(L[0], R[0], baseline=0.5, cu=160.0, cv=30.0, f=700.0, roix=20.0, roiy=5.0, roiz=40.0, scale=1000.0)\n"
            "out['note_depth'] = np.array(c.last_error())\n"
            "dl = c.dev_alloc(L.nbytes); dr = c.dev_alloc(R.nbytes); c.h2d(dl, L); c.h2d(dr, R)\n"
            "o = c.stereo_seq_process(dl, dr, n, w, h, stages=2, baseline=0.5, cu=160.0, cv=30.0, f=700.0, roix=20.0, roiy=5.0, roiz=40.0, scale=1000.0)\n"
            "c.sync(); out['note_seq'] = np.array(c.last_error())\n"
            "res = c.stereo_seq_fetch(o, n, w, h, 2); out['disp'] = res['disp']; out['depth'] = res['depth']\n"
            f"np.savez(r'{tmp_path / 'out.npz'}', **out); c.close()\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=root, SSM_SGBM_TEST_TIMEOUT=hook), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(tmp_path / "out.npz")
    po = oracle.sgbm_params()
    assert np.array_equal(got["pair"], oracle.sgbm(L[0], R[0], po))
    assert np.array_equal(got["pd_disp"], oracle.sgbm(L[0], R[0], po))
    assert np.array_equal(got["pd_depth"], oracle.disparity_to_depth(oracle.sgbm(L[0], R[0], po), 0.5, 160.0, 30.0, 700.0, 20.0, 5.0, 40.0, 1000.0))
    for k in range(n):
        d = oracle.sgbm(L[k], R[k], po)
        assert np.array_equal(got["disp"][k], d), k
        assert np.array_equal(got["depth"][k], oracle.disparity_to_depth(d, 0.5, 160.0, 30.0, 700.0, 20.0, 5.0, 40.0, 1000.0)), k
    if hook == "1":       # a reported time-out leaves a note (the call itself succeeds); the occupancy check chooses form 1 silently
        assert "form 1" in str(got["note_pair"]) and "form 1" in str(got["note_seq"]) and "3 sub-batch" in str(got["note_seq"])
        assert "form 1" in str(got["note_depth"])
    else:
        assert str(got["note_seq"]) == ""
