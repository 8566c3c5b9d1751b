"""Label fusion on a real MI355X (ssm_relabel_points, ssm_relabel, ssm_relabel_view_create, csrc/kernels_relabel.hip): device == ssm_relabel_host byte for byte --
every point's label, its packed counts through ssm_debug_relabel_record, the info -- on the case list of tests/relabel_ref.py (tests/test_relabel.py ties the host
function to the restatement), at the point counts around a wave and a block, with 0, 1, 2 and 16 views, on device-resident clouds (whose other 28 bytes per point
and size stay), after ssm_cloud_sor, between two ssm_carve calls, with the views' label images equal to the host's, a small call after a large one on one
context, once on a 640 x 480 and once on a 1241 x 376 cloud, under all three kernel forms, and with every refusal."""
import os
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import relabel_ref as R  # noqa: E402
import carve_ref as CR  # noqa: E402
from conftest import CAM  # noqa: E402

pytestmark = pytest.mark.gpu
W, H = 640, 480
CASES = list(R.cases())
FORMS = [0, 1, 2]          # csrc/kernels_relabel.hip: a depth and a label image per view; one packed word per pixel; packed with two views in flight
_memo = {}


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


@pytest.fixture(scope="module")
def c():
    import semantic_slam_mapping_amd as ssm
    x = ssm.Context(0, width=W, height=H, orb_features=500, max_batch=1, voxel_capacity_log2=12, camera=CAM)
    yield x
    x.close()


@pytest.fixture
def form(request, c):
    """the form of the views and calls of one test, the default again afterwards"""
    c.relabel_form(request.param)
    yield request.param
    c.relabel_form(-1)


class Views:
    """the device views of a list of host views (dicts: depth, label, camera), freed on the way out"""
    def __init__(self, c, views):
        self.c, self.h = c, []
        self.host = views
        for V in views:
            self.h.append(c.relabel_view(V["depth"], R.bgr_of_labels(V["label"]), V["camera"]))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        for h in self.h:
            self.c.relabel_view_free(h)


def host(views, T_views, pts, T_cloud, **params):
    import semantic_slam_mapping_amd as ssm
    return ssm.relabel_host([(V["depth"], V["label"], V["camera"]) for V in views], T_views, pts, T_cloud, **params)


def assert_points(c, vs, T_views, pts, T_cloud, what, **params):
    """ssm_relabel_points and its record against the host function"""
    want_l, want_v, want_i = host(vs.host, T_views, pts, T_cloud, **params)
    before = pts.tobytes()
    labels, info = c.relabel_points(vs.h, T_views, pts, T_cloud, **params)
    assert pts.tobytes() == before
    assert np.array_equal(labels, want_l), (what, np.nonzero(labels != want_l)[0][:5])
    assert info == want_i, (what, info, want_i)
    votes, rec = c.relabel_record(len(pts))
    assert np.array_equal(votes, want_v) and np.array_equal(rec, want_l), (what, np.nonzero(votes != want_v)[0][:5])
    return want_i


def case_of(name):
    return memo(name, R.cases()[name] if name in R.cases() else None)


@pytest.mark.parametrize("form", FORMS, indirect=True)
@pytest.mark.parametrize("name", CASES)
def test_case_list(c, name, form):
    import semantic_slam_mapping_amd as ssm
    cs = case_of(name)
    with Views(c, cs["views"]) as vs:
        for h, V in zip(vs.h, cs["views"]):
            lab = c.relabel_view_labels(h)
            assert np.array_equal(lab, V["label"]) and np.array_equal(lab, ssm.relabel_labels_host(R.bgr_of_labels(V["label"])))
        I = assert_points(c, vs, cs["T_views"], cs["pts"], cs["T_cloud"], name, **cs["params"])
        assert I["n_changed"] > I["n_filled"] > 0


@pytest.mark.parametrize("form", FORMS, indirect=True)
def test_point_counts_around_a_wave_and_a_block(c, form):
    cs = case_of("posed_160x120")
    with Views(c, cs["views"]) as vs:
        for n in (0, 1, 63, 64, 65, 255, 256, 257):
            I = assert_points(c, vs, cs["T_views"], cs["pts"][1000:1000 + n], cs["T_cloud"], n, **cs["params"])
            assert I["n_in"] == n and (n < 63 or I["n_changed"] > 0)


@pytest.mark.parametrize("form", FORMS, indirect=True)
def test_view_counts(c, form):
    cs = memo("sixteen", R.posed(70, 9, 8, 16))
    with Views(c, cs["views"]) as vs:
        for v in (0, 1, 2, 16):
            sub = Views.__new__(Views); sub.h, sub.host = vs.h[:v], vs.host[:v]
            I = assert_points(c, sub, cs["T_views"][:v], cs["pts"], cs["T_cloud"], v)
            assert (I["pairs_supported"] > 0) == (v > 0)
        sub = Views.__new__(Views); sub.h, sub.host = vs.h[::-1], vs.host[::-1]
        assert_points(c, sub, cs["T_views"][::-1], cs["pts"], cs["T_cloud"], "reversed", own_weight=3, min_votes=5)


def test_small_after_large(c):
    big, small = case_of("posed_160x120"), case_of("constructed")
    with Views(c, big["views"]) as vb, Views(c, small["views"]) as vs:
        assert_points(c, vb, big["T_views"], big["pts"], big["T_cloud"], "large", **big["params"])
        assert_points(c, vs, small["T_views"], small["pts"], small["T_cloud"], "small", **small["params"])
        with pytest.raises(Exception):
            c.relabel_record(len(big["pts"]))          # the record is the last call's


# ---- device-resident clouds
def scene():
    """a 640 x 480 depth image, a colour image, the cloud's semantic image (classes the back-projection neither gates nor masks, a quarter of the blocks wrong and a
    few of no palette colour) and the label images of four views that mostly agree with the truth"""
    def make():
        d = CR.scene_depth(W, H, 21)
        rng = np.random.default_rng(2)
        bgr = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        g = np.array([1, 4, 5, 6, 8])[rng.integers(0, 5, (H // 8, W // 8))]
        own = g.copy()
        wrong = rng.random(g.shape)
        own[wrong < 0.25] = np.array([1, 4, 5, 6, 8])[rng.integers(0, 5, int((wrong < 0.25).sum()))]
        own[wrong > 0.95] = R.U
        truth = g.repeat(8, 0).repeat(8, 1)
        views = []
        for k in range(4):
            lab = truth.copy()
            noise = rng.random((H, W))
            lab[noise < 0.03] = rng.integers(0, 12, int((noise < 0.03).sum()))
            lab[noise > 0.98] = R.U
            dv = d.copy()
            dv[rng.random((H, W)) < 0.02] = 0
            views.append(R.view(dv, lab, CAM))
        return d, bgr, R.bgr_of_labels(own.repeat(8, 0).repeat(8, 1)), views, [CR.pose(rng, 0.002, 0.004) for _ in range(4)], CR.pose(rng, 0.002, 0.004)
    return memo("scene", make)


def assert_cloud(c, vs, T_views, cl, T_cloud, what, **params):
    """ssm_relabel on a device cloud against the host function on its fetched points: the labels, and nothing else of the cloud, change"""
    before = c.cloud_fetch(cl).copy()
    want_l, want_v, want_i = host(vs.host, T_views, before, T_cloud, **params)
    info = c.relabel(vs.h, T_views, cl, T_cloud, **params)
    after = c.cloud_fetch(cl)
    assert len(after) == len(before) == c.cloud_size(cl) and info == want_i, (what, info, want_i)
    assert np.array_equal(after["label"], want_l), (what, np.nonzero(after["label"] != want_l)[0][:5])
    rest = after.copy(); rest["label"] = before["label"]
    assert rest.tobytes() == before.tobytes(), what
    votes, rec = c.relabel_record(len(before))
    assert np.array_equal(votes, want_v) and np.array_equal(rec, want_l), what
    return want_i, after.copy()


@pytest.mark.parametrize("form", FORMS, indirect=True)
def test_device_cloud_640x480(c, form):
    d, bgr, sem, views, Tv, Tc = scene()
    cl = c.backproject_dev(d, bgr, sem)
    try:
        with Views(c, views) as vs:
            I, _ = assert_cloud(c, vs, Tv, cl, Tc, "640x480")
            assert I["n_in"] > 250000 and I["n_changed"] > 10000 and I["n_filled"] > 1000 and I["pairs_voted"] > I["n_in"]
            I2, _ = assert_cloud(c, vs, Tv, cl, Tc, "again")          # the fused labels are what the next call starts from
            assert I2["n_changed"] < I["n_changed"] // 4
    finally:
        c.cloud_free(cl)


def kitti():
    """a 1241 x 376 cloud (depth in centimetres, the KITTI layout) and three views of that size"""
    def make():
        w, h = 1241, 376
        cam = (607.2, 185.2, 718.9, 718.9, 100.0)          # the KITTI layout: depth in centimetres
        rng = np.random.default_rng(9)
        d = (CR.scene_depth(w, h, 31).astype(np.int64) // 4).astype(np.uint16)
        truth = R.blocky(rng, w, h, 8, 0.05)
        views = []
        for k in range(3):
            lab = truth.copy()
            noise = rng.random((h, w))
            lab[noise < 0.03] = rng.integers(0, 12, int((noise < 0.03).sum()))
            views.append(R.view(d, lab, cam))
        xyz = CR.backproject(d, cam)
        own = truth[d > 0].copy()
        flip = rng.random(len(own))
        own[flip < 0.2] = rng.integers(0, 12, int((flip < 0.2).sum()))
        own[flip > 0.9] = R.U
        return views, [CR.pose(rng, 0.001, 0.01) for _ in range(3)], R.labelled(xyz, own, 9), CR.pose(rng, 0.001, 0.01)
    return memo("kitti", make)


@pytest.mark.parametrize("form", FORMS, indirect=True)
def test_cloud_1241x376(c, form):
    views, Tv, pts, Tc = kitti()
    with Views(c, views) as vs:
        I = assert_points(c, vs, Tv, pts, Tc, "1241x376")
        assert I["n_in"] > 400000 and I["n_changed"] > 30000 and I["n_filled"] > 10000


@pytest.mark.parametrize("form", FORMS, indirect=True)
def test_after_outlier_removal_and_between_carvings(c, form):
    """the cloud as ssm_cloud_sor leaves it, then one ssm_carve, the fusion (run counters untouched), and a second ssm_carve that gives what the host composition gives"""
    import semantic_slam_mapping_amd as ssm
    d, bgr, sem, views, Tv, Tc = scene()
    rng = np.random.default_rng(5)
    dep = np.zeros_like(d)
    dep[1::4, 1::4] = d[1::4, 1::4]
    dep.reshape(-1)[rng.choice(np.nonzero(d.reshape(-1))[0], 200, replace=False)] = 500          # speckles for the filter
    cl = c.backproject_dev(dep, bgr, sem)
    try:
        with Views(c, views[:3]) as vs:
            n0 = c.cloud_size(cl)
            c.cloud_sor(cl)
            assert c.cloud_size(cl) < n0
            I, _ = assert_cloud(c, vs, Tv[:3], cl, Tc, "after sor")
            assert I["n_changed"] > 500
            far = np.clip(d[::8, ::8].astype(np.int64) + 900 * (np.arange(W // 8) % 16 < 9), 1, 65535).astype(np.uint16)          # stripes pushed back: seen through there
            cam8 = (CAM[0] / 8, CAM[1] / 8, CAM[2] / 8, CAM[3] / 8, CAM[4])
            Tcv = CR.pose(rng, 0.004, 0.02)
            cv = c.carve_view(far, cam8)
            try:
                c.carve(cv, Tcv, [cl], [Tc], min_votes=2)
                run = c.cloud_run(cl).copy()
                assert run.any()
                _, fused = assert_cloud(c, vs, Tv[:3], cl, Tc, "after one carving", min_votes=1, own_weight=0)
                assert c.cloud_run(cl).tobytes() == run.tobytes()
                info = c.carve(cv, Tcv, [cl], [Tc], min_votes=2)[0]
            finally:
                c.carve_view_free(cv)
            hp, hrun, hinfo = ssm.carve_host(far, cam8, Tcv, fused, Tc, run=run, min_votes=2)
            assert info == hinfo and 0 < info["n_kept"] < len(fused)
            assert c.cloud_fetch(cl).tobytes() == hp.tobytes() and c.cloud_run(cl).tobytes() == hrun.tobytes()
    finally:
        c.cloud_free(cl)


def test_refusals(c):
    import semantic_slam_mapping_amd as ssm
    cs = case_of("constructed")
    E = np.eye(4)
    other = ssm.Context(0, width=W, height=H, orb_features=500, max_batch=1, voxel_capacity_log2=12, camera=CAM)
    try:
        with Views(c, cs["views"][:2]) as vs, Views(other, cs["views"][:1]) as vo:
            def refused(views=None, T_views=None, T_cloud=E, **kw):
                views = vs.h if views is None else views
                with pytest.raises(ssm.SsmError) as e:
                    c.relabel_points(views, [E] * len(views) if T_views is None else T_views, cs["pts"], T_cloud, **kw)
                assert e.value.code == -1, e.value
            refused(views=vs.h[:1] * 17)
            refused(views=[vs.h[0], None])
            refused(views=[vs.h[0], vs.h[1], vs.h[0]])
            refused(views=[vs.h[0], vo.h[0]])
            for kw in (dict(radius=-1), dict(radius=4), dict(edge_guard=2), dict(own_weight=16), dict(own_weight=-1), dict(min_votes=0), dict(min_votes=32), dict(tol_abs=-1.0),
                       dict(tol_abs=float("nan")), dict(tol_rel_ppm=1000001), dict(z_min=-0.1), dict(z_min=float("inf"))):
                refused(**kw)
                refused(views=[], **kw)
            bad = E.copy(); bad[2, 3] = float("nan")
            refused(T_views=[E, bad])
            refused(T_cloud=bad)
            V = cs["views"][0]
            for cam in ((float("nan"), 0, 64, 64, 1000), (0, 0, 64, float("inf"), 1000), (0, 0, 64, 64, 0.0), (0, 0, 64, 64, 1.0e6 + 1)):
                with pytest.raises(ssm.SsmError) as e:
                    c.relabel_view(V["depth"], R.bgr_of_labels(V["label"]), cam)
                assert e.value.code == -1
            lib = c.lib
            assert lib.ssm_relabel(c.h, None, None, 0, None, E.ctypes.data, None, None) == -1                 # no cloud
            assert lib.ssm_relabel_points(c.h, None, None, 0, None, 3, E.ctypes.data, None, None, None) == -1   # points promised, none given
            assert lib.ssm_relabel_view_create(c.h, None, None, 4, 4, None, None) == -1
            c.relabel_form(0)
            try:
                refused()                                         # views of the other form
                with pytest.raises(ssm.SsmError):
                    c.relabel_form(3)
            finally:
                c.relabel_form(-1)
            d, bgr, sem, _, _, _ = scene()                              # a cloud of the other context (same GPU): refused by either, taken by its own
            cl = other.backproject_dev(d, bgr, sem)
            try:
                with pytest.raises(ssm.SsmError) as e:
                    c.relabel(vs.h, [E, E], cl, E)
                assert e.value.code == -1 and "another context" in str(e.value)
                assert other.relabel(vo.h, [E], cl, E)["n_in"] == other.cloud_size(cl) > 0
            finally:
                other.cloud_free(cl)
            labels, info = c.relabel_points(vs.h, [E, E], cs["pts"], E)          # and the context still works
            assert info["n_in"] == len(cs["pts"])
    finally:
        other.close()
