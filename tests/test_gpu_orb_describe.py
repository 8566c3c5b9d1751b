"""The describe stage of the ORB front end (kp_prepare_kernel, orient_kernel, angle_kernel, brief_kernel) at PLANTED keypoints: ssm_debug_orb_describe
against tests/orb_describe_ref.py, every field byte for byte -- m10, m01, angle, sin, cos, the keypoint record, the descriptor, the position and the count.
The reference works on the levels of the DEVICE pyramid (ssm_debug_pyramid) and on oracle.gaussian7 of them; tests/test_orb_describe_ref.py holds it to
oracle/orb.c and pyref on the CPU and asserts that the case list of this file reaches its edges.  Planted: the legal extremes of every level with all 16
alignment residues at both borders; one patch translated by 1 .. 16 columns; slot shapes with empty levels, one keypoint, full levels, level boundaries inside
a wave's group of slots, and frames without any keypoint inside a batch; patches built for zero, one-sided, equal and extreme moments; planted moments through
every octant and boundary of the angle and every quadrant of the sin / cos reduction; custom BRIEF tables on the ring that reaches +-18; scores, depths; a
small call after a full one and an ordinary extraction afterwards; both blur variants; every refusal of the hook."""
import numpy as np
import pytest

import orb_describe_ref as R
from conftest import CAM, SEED

pytestmark = pytest.mark.gpu

BATCH = 9


class Rig:
    """one context of a geometry + the reference of what it is handed"""

    def __init__(self, oracle, w, h, levels, pattern=None, **kw):
        import semantic_slam_mapping_amd as ssm
        self.oracle, self.w, self.h, self.levels = oracle, w, h, levels
        self.geom = R.geometry(w, h, levels, R.NFEAT)
        self.pattern = R.default_pattern() if pattern is None else pattern
        extra = {} if pattern is None else {"brief_pattern": pattern}
        self.c = ssm.Context(0, width=w, height=h, orb_levels=levels, orb_features=R.NFEAT, max_batch=BATCH, voxel_capacity_log2=12, camera=CAM, **extra, **kw)
        assert self.c.cap == sum(L.sel_cap for L in self.geom)
        self._ref = {}

    def close(self):
        self.c.close()

    def images(self, img):
        """(levels, blurred levels) of one gray frame: the device's pyramid, the oracle's blur of it"""
        key = hash(img.tobytes())
        if key not in self._ref:
            lv = [v[:, :L.w] for v, L in zip(R.level_views(self.c.debug_pyramid(img[None])[0], self.geom), self.geom)]
            self._ref[key] = (lv, [self.oracle.gaussian7(v) for v in lv])
        return self._ref[key]

    def random_plants(self, counts, rng):
        """per level (k, 3) random (x, y, score) inside the window"""
        return [np.stack([rng.integers(R.EDGE, L.w - R.EDGE, k), rng.integers(R.EDGE, L.h - R.EDGE, k), rng.integers(0, 256, k)], 1) for k, L in zip(counts, self.geom)]

    def check(self, imgs, plants, depth=None, moments=None, what=""):
        """imgs: gray frames; plants: per frame, per level (k, 3) of (x, y, score); depth: None or per frame an image; moments: None or per frame (k, 2).  Runs the hook once
        and compares every frame with the reference; returns the hook's output and the references"""
        n = len(imgs)
        nsel = np.array([[len(p) for p in fr] for fr in plants], np.int32).reshape(n, self.levels)
        cat = [np.asarray(p, np.int64).reshape(-1, 3) for fr in plants for p in fr]
        allp = np.concatenate(cat) if cat else np.zeros((0, 3), np.int64)
        out = self.c.debug_orb_describe(np.stack(imgs), nsel, R.pack(allp[:, 0], allp[:, 1], allp[:, 2]), None if depth is None else np.stack(depth),
                                        None if moments is None else np.concatenate(moments))
        refs = []
        for f in range(n):
            k = int(nsel[f].sum())
            assert int(out["nkp"][f]) == k, "%s frame %d: nkp %d, planted %d" % (what, f, out["nkp"][f], k)
            lv, bl = self.images(imgs[f])
            ref = R.describe(lv, bl, self.geom, plants[f], self.pattern, CAM, None if depth is None else depth[f], None if moments is None else moments[f])
            kp = out["kps"][f]
            got = {"m10": out["moments"][f, :, 0], "m01": out["moments"][f, :, 1], "sn": out["sincos"][f, :, 0], "cs": out["sincos"][f, :, 1], "desc": out["desc"][f], "pos3d": out["pos3d"][f]}
            got.update({k_: kp[k_] for k_ in ("x", "y", "size", "angle", "response", "octave", "class_id")})
            d = R.first_difference(got, ref, k)
            if d is not None:
                i = d[1]
                raise AssertionError("%s frame %d keypoint %d (level %d, x %d, y %d, x mod 16 = %d): %s is %s, expected %s" % (
                    what, f, i, ref["level"][i], ref["px"][i], ref["py"][i], ref["px"][i] % 16, d[0], d[2], d[3]))
            for a in (out["kps"][f, k:], out["desc"][f, k:], out["pos3d"][f, k:], out["moments"][f, k:], out["sincos"][f, k:]):       # nothing is written behind the count
                assert (np.ascontiguousarray(a).view(np.uint8) == 0xA5).all(), "%s frame %d: a record behind nkp = %d was written" % (what, f, k)
            refs.append(ref)
        return out, refs


_rigs = {}


@pytest.fixture(scope="module")
def rig(oracle):
    """the default context of a geometry, shared by the tests of this module"""
    def get(w, h, levels):
        if (w, h, levels) not in _rigs:
            _rigs[(w, h, levels)] = Rig(oracle, w, h, levels)
        return _rigs[(w, h, levels)]
    yield get
    for r in _rigs.values():
        r.close()
    _rigs.clear()


def _chunks(pts, geom, frames):
    """the same point list for every level, dealt over `frames` frames by each level's slot count: per frame, per level (k, 3) with score = index & 255"""
    out = []
    for f in range(frames):
        fr = []
        for L in geom:
            p = [(x, y) for x, y in pts(L)][f * L.sel_cap:(f + 1) * L.sel_cap]
            idx = np.arange(f * L.sel_cap, f * L.sel_cap + len(p))
            fr.append(np.array([[x, y, i & 255] for (x, y), i in zip(p, idx)], np.int64).reshape(-1, 3))
        out.append(fr)
    assert all(sum(len(fr[l]) for fr in out) == len(pts(L)) for l, L in enumerate(geom))
    return out


def _frames_for(geom, npts):
    return max(-(-npts // L.sel_cap) for L in geom)


@pytest.mark.parametrize("w,h,levels", R.GEOMS)
def test_borders_and_residues(rig, w, h, levels):
    r = rig(w, h, levels)
    img = R.noise_image(w, h, 21)
    nfr = _frames_for(r.geom, max(len(R.border_points(L.w, L.h)) for L in r.geom))
    assert nfr <= BATCH
    plants = _chunks(lambda L: R.border_points(L.w, L.h), r.geom, nfr)
    r.check([img] * nfr, plants, what="borders")


@pytest.mark.parametrize("w,h,levels", R.GEOMS)
def test_translation_by_1_to_16_columns(rig, w, h, levels):
    """level 0 of a rolled image is the image rolled: an interior keypoint shifted with it keeps its moments and its descriptor while its staging offsets change"""
    r = rig(w, h, levels)
    img = R.noise_image(w, h, 22)
    base = [(60, 40), (75, h - 41), (w // 2 - 9, h // 2), (w - 80, 37)]
    imgs = [np.ascontiguousarray(np.roll(img, k, 1)) for k in range(17)]
    plants = [[np.array([[x + k, y, 9] for x, y in base], np.int64)] + [np.array([[L.w // 2 - 8 + k, L.h // 2, 3]], np.int64) for L in r.geom[1:]] for k in range(17)]
    got = []
    for a, b in ((0, 9), (9, 17)):
        out, _ = r.check(imgs[a:b], plants[a:b], what="translation")
        got += [(out["moments"][f, :4].copy(), out["desc"][f, :4].copy(), out["kps"][f, :4]["angle"].copy()) for f in range(b - a)]
    for x, _ in base:                                                                       # every residue of the staged patch's first column, and more than one first word
        assert {(x + k - 18) & 15 for k in range(17)} == set(range(16)) and len({(x + k - 18) & ~15 for k in range(17)}) >= 2
    for k in range(1, 17):
        for j in range(3):
            assert np.array_equal(got[k][j], got[0][j]), "shift %d changes %s of the level-0 keypoints %s" % (k, ("the moments", "the descriptor", "the angle")[j], np.flatnonzero((got[k][j] != got[0][j]).reshape(4, -1).any(1)))


@pytest.mark.parametrize("w,h,levels", R.GEOMS)
def test_slot_shapes(rig, w, h, levels):
    r = rig(w, h, levels)
    rng = np.random.default_rng(23)
    img = [R.noise_image(w, h, 24), R.noise_image(w, h, 25)]
    shapes = R.slot_shapes(r.geom)
    names = ["full", "none", "last_only"] + [n for n in shapes if n not in ("full", "none", "last_only")]
    plants = {n: r.random_plants(shapes[n], rng) for n in names}
    # calls of 3 and 9 frames with a different selection per frame, one of them none; then the rest
    r.check([img[0], img[1], img[0]], [plants[n] for n in ("full", "none", "sparse" if "sparse" in plants else "last_only")], what="shapes full/none/sparse")
    for i in range(0, len(names), BATCH):
        part = names[i:i + BATCH]
        r.check([img[j % 2] for j in range(len(part))], [plants[n] for n in part], what="shapes " + "/".join(part))
    # every frame empty
    out, _ = r.check([img[0]] * 3, [plants["none"]] * 3, what="no keypoint at all")
    assert (out["nkp"] == 0).all()


def _moment_patches():
    """name -> (31 x 31 patch, property its (m10, m01) must have): the disc's moments of constructed patches"""
    rng = np.random.default_rng(26)
    a = rng.integers(0, 256, (31, 31)).astype(np.uint8)
    v, u = np.mgrid[-15:16, -15:16]
    lr = np.where(u >= 0, a, a[:, ::-1])                         # p(v, u) = p(v, -u): m10 = 0
    ud = np.where(v >= 0, a, a[::-1, :])                         # p(v, u) = p(-v, u): m01 = 0
    ramp_v, ramp_u = np.clip(v * 3, -60, 60), np.clip(u * 3, -60, 60)
    cases = {
        "flat": (np.full((31, 31), 128, np.uint8), lambda a_, b_: a_ == 0 and b_ == 0),
        "black": (np.zeros((31, 31), np.uint8), lambda a_, b_: a_ == 0 and b_ == 0),
        "white": (np.full((31, 31), 255, np.uint8), lambda a_, b_: a_ == 0 and b_ == 0),
        "m10_zero_m01_pos": (np.clip(lr // 2 + 64 + ramp_v, 0, 255).astype(np.uint8), lambda a_, b_: a_ == 0 and b_ > 0),
        "m10_zero_m01_neg": (np.clip(lr // 2 + 64 - ramp_v, 0, 255).astype(np.uint8), lambda a_, b_: a_ == 0 and b_ < 0),
        "m01_zero_m10_pos": (np.clip(ud // 2 + 64 + ramp_u, 0, 255).astype(np.uint8), lambda a_, b_: b_ == 0 and a_ > 0),
        "m01_zero_m10_neg": (np.clip(ud // 2 + 64 - ramp_u, 0, 255).astype(np.uint8), lambda a_, b_: b_ == 0 and a_ < 0),
        "transposed_symmetric": (np.where(u >= v, a, a.T), lambda a_, b_: a_ == b_ and a_ != 0),
        "anti_transposed_symmetric": (np.where(u >= -v, a, a[::-1, ::-1].T), lambda a_, b_: a_ == -b_ and a_ != 0),
        "half_right": ((u > 0) * np.uint8(255), lambda a_, b_: a_ == R.max_moment() and b_ == 0),
        "half_left": ((u < 0) * np.uint8(255), lambda a_, b_: a_ == -R.max_moment() and b_ == 0),
        "half_bottom": ((v > 0) * np.uint8(255), lambda a_, b_: a_ == 0 and b_ == R.max_moment()),
        "half_top": ((v < 0) * np.uint8(255), lambda a_, b_: a_ == 0 and b_ == -R.max_moment()),
        "quadrant": (((u > 0) & (v > 0)) * np.uint8(255), lambda a_, b_: a_ == b_ and a_ > R.max_moment() // 3),
        "quadrant_opposite": (((u < 0) & (v > 0)) * np.uint8(255), lambda a_, b_: a_ == -b_ and b_ > R.max_moment() // 3),
    }
    return {k: (np.asarray(p, np.uint8), f) for k, (p, f) in cases.items()}


@pytest.mark.parametrize("w,h,levels", R.GEOMS)
def test_moments_from_constructed_patches(rig, w, h, levels):
    r = rig(w, h, levels)
    patches = _moment_patches()
    spots = [(x, y) for y in range(34, h - 34, 38) for x in range(34, w - 34, 38)]            # patch centres, 38 apart: the discs do not touch
    names = list(patches)
    nfr = -(-len(names) // min(len(spots), r.geom[0].sel_cap))
    per = -(-len(names) // nfr)
    imgs, plants, placed = [], [], []
    for f in range(nfr):
        img = R.noise_image(w, h, 27 + f); pl = []
        for j, name in enumerate(names[f * per:(f + 1) * per]):
            x, y = spots[(j * 7 + 3) % len(spots)] if len(spots) > 7 * per else spots[j]
            img[y - 15:y + 16, x - 15:x + 16] = patches[name][0]
            pl.append((x, y, j)); placed.append((f, name))
        assert len({p[:2] for p in pl}) == len(pl)
        imgs.append(img); plants.append([np.array(pl, np.int64)] + [np.zeros((0, 3), np.int64)] * (levels - 1))
    out, refs = r.check(imgs, plants, what="constructed moments")
    seen = 0
    for f in range(nfr):
        for j, (m10, m01) in enumerate(zip(refs[f]["m10"].tolist(), refs[f]["m01"].tolist())):
            name = placed[seen][1]; seen += 1
            assert patches[name][1](m10, m01), (name, m10, m01)                              # (of the REFERENCE's sums: the patch is what its name says)
    assert seen == len(names)


@pytest.mark.parametrize("w,h,levels", R.GEOMS)
def test_planted_moments_sweep(rig, w, h, levels):
    r = rig(w, h, levels)
    rng = np.random.default_rng(28)
    img = R.noise_image(w, h, 29)
    m = R.moment_cases()
    per = r.c.cap                                                                           # every level full
    for at in range(0, len(m), per * BATCH):
        part = m[at:at + per * BATCH]
        nfr = -(-len(part) // per)
        plants, moms = [], []
        for f in range(nfr):
            k = min(per, len(part) - f * per)
            counts, left = [], k
            for L in r.geom:
                counts.append(min(L.sel_cap, left)); left -= counts[-1]
            plants.append(r.random_plants(counts, rng)); moms.append(part[f * per:f * per + k])
        r.check([img] * nfr, plants, moments=moms, what="planted moments from case %d on" % at)


@pytest.mark.parametrize("w,h,levels", R.GEOMS)
@pytest.mark.parametrize("which", ["ring", "random"])
def test_custom_pattern(oracle, w, h, levels, which):
    r = Rig(oracle, w, h, levels, pattern=R.ring_pattern() if which == "ring" else R.random_pattern())
    try:
        img = R.noise_image(w, h, 30)
        nfr = _frames_for(r.geom, max(len(R.border_points(L.w, L.h)) for L in r.geom))
        plants = _chunks(lambda L: R.border_points(L.w, L.h), r.geom, nfr)
        rm = R.ring_moments()
        moms, at = [], 0
        for fr in plants:
            k = sum(len(p) for p in fr)
            moms.append(rm[(np.arange(at, at + k) * 5) % len(rm)]); at += k                 # (5 and 144 are coprime: neighbouring residues get angles 12.5 degrees apart, all 144 occur)
        r.check([img] * nfr, plants, moments=moms, what=which + " pattern, planted angles")
        r.check([img] * nfr, plants, what=which + " pattern, image moments")
    finally:
        r.close()


@pytest.mark.parametrize("w,h,levels", R.GEOMS)
def test_scores_and_depth(rig, w, h, levels):
    r = rig(w, h, levels)
    rng = np.random.default_rng(31)
    img = R.noise_image(w, h, 32)
    counts = [min(12, L.sel_cap) for L in r.geom]
    plants = []
    for f in range(4):
        p = r.random_plants(counts, rng)
        for q in p:
            q[:, 2] = np.resize([0, 255, 1, 254, 128], len(q))
        plants.append(p)
    depths = [np.zeros((h, w), np.uint16), np.ones((h, w), np.uint16), np.full((h, w), 65535, np.uint16), rng.integers(0, 65536, (h, w)).astype(np.uint16)]
    depths[3][::2, ::3] = 0
    out, refs = r.check([img] * 4, plants, depth=depths, what="depth")
    k = sum(counts)
    assert (out["pos3d"][0, :k] == 0).all() and (out["pos3d"][1, :k, 2] == np.float32(0.001)).all() and (out["pos3d"][2, :k, 2] == np.float32(65.535)).all()
    assert set(out["kps"][0, :k]["response"].tolist()) == {0.0, 255.0, 1.0, 254.0, 128.0}
    out, _ = r.check([img] * 4, plants, what="no depth image")
    assert (out["pos3d"][:, :k] == 0).all()


@pytest.mark.parametrize("w,h,levels", [(640, 480, 8), (176, 88, 1)])
def test_small_call_after_a_full_one_then_extraction(oracle, w, h, levels):
    r = Rig(oracle, w, h, levels)
    try:
        rng = np.random.default_rng(33)
        img = R.noise_image(w, h, 34)
        full = [r.random_plants([L.sel_cap for L in r.geom], rng) for _ in range(3)]
        r.check([img] * 3, full, moments=[rng.integers(-1000, 1000, (r.c.cap, 2)).astype(np.int32)] * 3, what="full")
        few = r.random_plants([2 if l % 2 == 0 else 0 for l in range(levels)], rng)
        r.check([img], [few], what="few after full")
        r.check([img] * 2, [few, r.random_plants([0] * levels, rng)], what="few and none after full")
        for i in (0, 3):                                                                     # the ordinary call is not affected by what was planted
            bgr = oracle.synth_frame(SEED, i, w, h)[0]
            gk, gd, _ = r.c.detect_features(bgr)
            ok, od = oracle.orb_extract(oracle.bgr2gray(bgr), nfeatures=R.NFEAT, nlevels=levels)
            assert len(ok) > 0 and gk.tobytes() == ok.tobytes() and np.array_equal(gd, od)
            r.check([img], [few], what="few after an extraction")
    finally:
        r.close()


@pytest.mark.parametrize("w,h,levels", R.GEOMS)
def test_both_blur_variants(oracle, monkeypatch, w, h, levels):
    rng = np.random.default_rng(35)
    img = R.noise_image(w, h, 36)
    got = {}
    plants = None
    for variant in (0, 1):
        monkeypatch.setenv("SSM_BLUR_VARIANT", str(variant))
        r = Rig(oracle, w, h, levels)
        try:
            if plants is None:
                plants = [r.random_plants([L.sel_cap for L in r.geom], rng) for _ in range(2)]
            out, _ = r.check([img, img[::-1].copy()], plants, what="blur variant %d" % variant)
            got[variant] = out
        finally:
            r.close()
    for k in got[0]:
        assert got[0][k].tobytes() == got[1][k].tobytes(), k


def test_every_refusal_of_the_hook(rig):
    import semantic_slam_mapping_amd as ssm
    w, h, levels = 640, 480, 8
    r = rig(w, h, levels)
    img = R.noise_image(w, h, 37)
    none = [np.zeros((0, 3), np.int64)] * levels

    def refused(imgs, plants, match):
        with pytest.raises(ssm.SsmError, match=match) as e:
            r.check(imgs, plants, what="refusal")
        assert e.value.code == -1                                                            # SSM_E_INVAL

    refused([img] * (BATCH + 1), [none] * (BATCH + 1), "max_batch")
    with pytest.raises(ssm.SsmError, match="max_batch") as e:                               # no frame at all
        r.c.debug_orb_describe(np.zeros((0, h, w), np.uint8), np.zeros((0, levels), np.int32), np.zeros(0, np.uint32))
    assert e.value.code == -1
    for l, L in enumerate(r.geom):
        over = [np.tile([[40, 40, 0]], (L.sel_cap + 1 if k == l else 0, 1)).reshape(-1, 3) for k in range(levels)]
        refused([img], [over], "nsel of frame 0 level %d outside" % l)
        refused([img, img], [none, over], "nsel of frame 1 level %d outside" % l)
        for x, y in ((R.EDGE - 1, 40), (L.w - R.EDGE, 40), (40, R.EDGE - 1), (40, L.h - R.EDGE), (0, 0), (L.w, 40), (4095, 4095), (40, L.h + 7)):
            bad = [np.array([[40, 40, 0], [x, y, 0]] if k == l else np.zeros((0, 3)), np.int64).reshape(-1, 3) for k in range(levels)]
            refused([img], [bad], r"planted keypoint \(%d, %d\) of frame 0 level %d outside" % (x, y, l))
    with pytest.raises(ssm.SsmError, match="nsel of frame 0 level 2 outside") as e:         # a negative count
        r.c.debug_orb_describe(img[None], np.array([[0, 0, -1, 0, 0, 0, 0, 0]], np.int32), np.zeros(0, np.uint32))
    assert e.value.code == -1
    with pytest.raises(ssm.SsmError, match="bad arguments"):                               # null pointers
        r.c._chk(r.c.lib.ssm_debug_orb_describe(r.c.h, None, 1, 1, *[None] * 10))
    # the window's own corners are accepted, and the context works after the refusals
    ok = [np.array([[x, y, 1] for x, y in R.window_corners(L.w, L.h)], np.int64) for L in r.geom]
    r.check([img], [ok], what="after the refusals")
