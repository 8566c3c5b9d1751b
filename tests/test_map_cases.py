"""The case table of the fused map stage (tests/map_cases.py) on the CPU: its restatement of the gates against the oracle (oracle/mapper.c) on every frame, and
every property a case claims -- the planted kept-pixel counts per wave in both layouts, the run patterns inside one lane's share, the single voxel, the block
tables that overflow and the ones that do not, the depth values around each gate, the hash slots, the cameras, the bit image's extent, the geometries the
context takes and refuses -- so that tests/test_gpu_map_planted.py cannot pass on a table that no longer plants them.  These are conditions on the INPUTS:
the seeds and constants in map_cases were chosen until the oracle alone satisfies them."""
import ctypes as C

import numpy as np
import pytest

import map_cases as K
from conftest import CAM

_clouds, _first = {}, {}


def clouds(oracle, c):
    """the oracle's cloud of every frame of a case (computed once)"""
    if c.name not in _clouds:
        _clouds[c.name] = [oracle.backproject(c.dep[f], c.bgr[f], c.sem[f], oracle.moving_mask(c.sem[f]), c.cfg.cam, None if c.poses is None else c.poses[f], c.cfg.maxd)
                           for f in range(c.n)]
    return _clouds[c.name]


def span_cloud(oracle, c, f, lo, hi):
    """the oracle's points of the pixels [lo, hi) (row-major) of frame f: the cloud is in pixel order"""
    if c.name not in _first:
        _first[c.name] = [np.concatenate([[0], np.cumsum(k.reshape(-1))]) for k in K.keep_mask(c)]
    k = _first[c.name][f]
    return clouds(oracle, c)[f][k[lo]:k[hi]]


def in_range(pts, leaf):
    """sso_voxel_key's range rule: floor(c * (1 / leaf)) in float, finite and inside (-2^20, 2^20) on every axis"""
    inv = np.float32(1.0) / np.float32(leaf)
    ok = np.ones(len(pts), bool)
    for a in "xyz":
        with np.errstate(over="ignore", invalid="ignore"):
            ok &= np.abs(np.floor(pts[a] * inv)) < np.float32(1048576.0)
    return ok


def test_table_is_deterministic_and_holds_what_the_issue_lists():
    names = [c.name for c in K.table()]
    assert len(names) == len(set(names)) >= 30
    a = K.waves("waves", K.G0)
    assert a.dep.tobytes() == K.case("waves").dep.tobytes() and a.sem.tobytes() == K.case("waves").sem.tobytes() and a.bgr.tobytes() == K.case("waves").bgr.tobytes()
    g = K.groups()
    assert {K.G0, K.G_D40, K.G_COARSE, K.G_ONE, K.G_DIV, K.G_5K, K.G_FRACTION, K.G_BELOW, K.G_CLAMP, K.ORDERED} | set(K.WIDTHS) == set(g)
    assert any(c.poses is None for c in K.table()) and any(c.poses is not None and np.array_equal(c.poses[0], np.eye(4)) for c in K.table())
    assert max(c.cfg.W * c.cfg.H * c.n for c in K.table()) <= 4064 * 131


def test_gates_restated_equal_the_oracle_on_every_frame(oracle):
    for c in K.table():
        keep, lab = K.keep_mask(c), K.label_image(c.sem)
        for f, cl in enumerate(clouds(oracle, c)):
            assert int(keep[f].sum()) == len(cl), "%s frame %d: keep_mask keeps %d pixels, the oracle emits %d points" % (c.name, f, keep[f].sum(), len(cl))
            # the same PIXELS, not just as many: the cloud is in row-major order and carries the pixel's camera colour and label
            px = c.bgr[f][keep[f]]
            assert np.array_equal(px[:, 0], cl["b"]) and np.array_equal(px[:, 1], cl["g"]) and np.array_equal(px[:, 2], cl["r"]), (c.name, f)
            assert np.array_equal(lab[f][keep[f]].astype(np.uint32), cl["label"]), (c.name, f)
        wc = K.wave_counts(c)
        assert wc.shape == (c.n, -(-c.cfg.W * c.cfg.H // K.WAVE)) and np.array_equal(wc.sum(1), keep.reshape(c.n, -1).sum(1))


@pytest.mark.parametrize("name", ["waves", "waves, coarse", "waves, division", "waves, scale 5000"])
def test_every_planted_count_is_there_in_both_layouts(name):
    c = K.case(name)
    wc, keep = K.wave_counts(c), K.keep_mask(c).reshape(c.n, -1, K.WAVE)
    assert np.array_equal(wc, c.claims["counts"])
    assert set(K.COUNTS) >= {0, 1, 2, 63, 64, 65, 66, 127, 128, 129, 191, 192, 193, 1023, 1024}
    for V in K.COUNTS:
        for layout in K.LAYOUTS:
            f, w = c.claims["planted"][(V, layout)]
            k = keep[f, w]
            assert int(wc[f, w]) == V == int(k.sum()), (V, layout)
            if layout == "first":
                assert k[:V].all()                                   # lanes 0 .. of the wave hold them, the last lanes' words hold none
            elif V:
                assert k[K.WAVE - 1]                                 # the last word of the wave holds the last kept pixel
                assert int(k.reshape(64, 16).any(1).sum()) == min(V, 64)      # ... and the others are spread over as many lanes' words as there are
    # the shares: lane i takes list entries [i P, (i + 1) P), P = ceil(V / 64)
    V = wc.reshape(-1)
    P = (V + 63) // 64
    lanes = np.where(P > 0, -(-V // np.maximum(P, 1)), 0)
    assert (P % 2 == 1).any() and ((P % 2 == 1) & (P > 1)).any()                    # an odd P: the loop's second pixel of the last trip is past the share
    assert ((V % np.maximum(P, 1) != 0) & (V > 0)).any()                             # a last lane that is only partly filled
    assert ((lanes < 64) & (V > 0)).any() and (lanes == 64).any()                    # lanes with no entry at all
    assert len(set(V.tolist())) > 40                                                 # ... and the random counts of the other waves


def test_wave_depths_split_neighbours_at_the_fine_leaf_and_not_at_the_coarse(oracle):
    fine, coarse = K.case("waves"), K.case("waves, coarse")
    f, w = fine.claims["planted"][(1024, "first")]
    for c, leaf in ((fine, 0.02), (coarse, 0.4)):
        cl = span_cloud(oracle, c, f, w * K.WAVE, (w + 1) * K.WAVE)
        assert len(cl) == K.WAVE
        keys = np.array([oracle.voxel_table(cl[i:i + 1], np.float32(leaf))["key"][0] for i in range(len(cl))])
        same = float((keys[1:] == keys[:-1]).mean())
        assert (same < 0.2) if leaf == 0.02 else (same > 0.8), (leaf, same)


@pytest.mark.parametrize("name,leaf", [("runs", 0.4), ("runs, fine", 0.02)])
def test_run_patterns_lie_inside_single_lane_shares(oracle, name, leaf):
    c = K.case(name)
    wc = K.wave_counts(c)
    seen, single = set(), 0
    for (f, w), (kind, P, V, pat) in c.claims["shares"].items():
        assert int(wc[f, w]) == V and P == (V + 63) // 64 and V == 64 * P
        seen.add((kind, P % 2))
        for lane in range(64):
            cl = span_cloud(oracle, c, f, w * K.WAVE + lane * P, w * K.WAVE + (lane + 1) * P)
            assert len(cl) == P and np.array_equal(cl["label"], np.array(pat, np.uint32)), (f, w, lane)
            tab = oracle.voxel_table(cl, np.float32(leaf))
            if leaf == 0.4 and len(tab) == 1:                      # the whole share in one voxel: the runs differ by the label alone
                single += 1
                for l in range(12):
                    assert int(tab["hist"][0, l]) == int((np.array(pat) == l).sum())
                assert int(tab["n"][0]) == P
    assert seen == {(k, odd) for k in K.RUN_PATTERNS for odd in (0, 1)}
    if leaf == 0.4:
        assert single > 0.7 * 64 * len(c.claims["shares"])
    aba = K.run_pattern("ABA", 15, (1, 3, 4, 5))
    assert aba[0] == aba[-1] == 1 and aba[5] == 3 and len(aba) == 15              # third run, back on the first key
    assert 255 in K.run_pattern("A?B", 16, (1, 3, 4, 5))


def test_one_voxel_takes_every_pixel_of_every_block(oracle):
    c = K.case("one voxel")
    assert K.keep_mask(c).all()
    tab = oracle.voxel_table(np.concatenate(clouds(oracle, c)), np.float32(c.cfg.leaf))
    assert len(tab) == 1 and int(tab["n"][0]) == 2 * 256 * 96
    for l in range(12):
        assert int(tab["hist"][0, l]) == c.claims["votes"].get(l, 0)
    assert tab["hist"][0, 8] != tab["hist"][0, 9] and set(c.claims["votes"]) == {8, 9, 1, 4}       # 8 | 9: both halves of one packed word
    per_block = 12288 * 5 // 8
    assert per_block < 65536                                                                     # the largest 16-bit count a block can reach in this table


def _block_voxels(oracle, c, f):
    npix = c.cfg.W * c.cfg.H
    return [len(oracle.voxel_table(span_cloud(oracle, c, f, lo, min(lo + 16 * K.BLOCK_WORDS, npix)), np.float32(c.cfg.leaf))) for lo in range(0, npix, 16 * K.BLOCK_WORDS)]


def test_block_tables_that_overflow_and_that_do_not(oracle):
    w = K.case("waves")
    assert max(max(_block_voxels(oracle, w, f)) for f in range(w.n)) > 256          # more voxels than the block's LDS table has slots: vox_direct
    assert max(_block_voxels(oracle, K.case("flat"), 0)) <= 256
    assert max(_block_voxels(oracle, K.case("one voxel"), 0)) == 1


def test_depth_values_sit_on_both_sides_of_every_gate(oracle):
    assert K.MAXD_FRACTION * 1000.0 != np.floor(K.MAXD_FRACTION * 1000.0)
    assert 1004.0 < K.MAXD_BELOW * 1000.0 < 1005.0 and K.dmax_of(K.G_BELOW) == 1004           # 1.005 is the decimal, the double product is below 1005
    assert K.G0.maxd * K.G0.cam[4] == 40000.0 and K.G_CLAMP.maxd * K.G_CLAMP.cam[4] >= 65535.0 and K.dmax_of(K.G_CLAMP) == 65535
    for name in ("depth 40 m", "depth 3.3003 m", "depth 1.005 m", "depth 100 m", "depth 7.77 m, scale 5000"):
        c = K.case(name)
        dm = K.dmax_of(c.cfg)
        want = {0, 1, dm - 1, dm, 65535} | ({dm + 1} if dm < 65535 else set())
        assert want <= set(c.claims["values"]) and want <= set(np.unique(c.dep).tolist()), name
        keep = K.keep_mask(c)
        assert np.array_equal(keep[0], (c.dep[0] != 0) & (c.dep[0] <= dm)), name                 # the integer rule of the kernel == the double rule of the oracle
        assert len(clouds(oracle, c)[0]) == int(keep.sum())
        assert bool(keep[0][c.dep[0] == 65535].all()) == (name == "depth 100 m")


def test_hash_slot_colours_cover_all_slots_and_none_is_of_the_palette():
    pal = {tuple(p) for p in K.PALETTE.tolist()}
    cols = K.slot_colours()
    assert [K.hash_slot(*c) for c in cols] == list(range(16)) and not (set(cols) & pal)
    occupied = {K.hash_slot(*p) for p in pal}
    assert len(occupied) == 12                                                  # the hash is perfect on the palette
    assert K.hash_slot(1, 0, 0) == 7 == K.hash_slot(*K.PALETTE[K.PEDESTRIAN])     # the sentinel of the empty slots lands on an occupied one
    for with_moving in (False, True):
        lab = K.label_image(K.label_colours(with_moving))
        assert set(range(12)) - set(lab.tolist()) == (set() if with_moving else set(K.MOVING))
        assert (lab == 255).sum() >= 12 * 5 + 16 + 3                            # the one-off neighbours, the slot colours, the sentinel, black, white
    for name in ("labels", "labels, division"):
        for f in range(2):                                                       # every colour of the list is in the frame
            used = {tuple(v) for v in K.case(name).sem[f].reshape(-1, 3).tolist()}
            assert {tuple(v) for v in K.label_colours(bool(f)).tolist()} <= used
    assert K.label_image(np.array([K.STRAY], np.uint8))[0] == 255


def test_cameras():
    assert K.CAM == CAM
    assert K.significand_all_ones(K.CAM_DIV[2]) and K.CAM_DIV[2] < 512.0 and not K.map_div_ok(K.CAM_DIV)
    for cfg in K.groups():
        if cfg.cam is not K.CAM_DIV:
            assert K.map_div_ok(cfg.cam), cfg
    assert K.CAM_5K[4] == 5000.0 and all(v != round(v) for v in K.CAM_5K[:4])
    assert {K.CAM, K.CAM_DIV, K.CAM_5K} <= {cfg.cam for cfg in K.groups()}


def test_bit_image_fits_and_the_table_holds_its_widest():
    best = (0, 0, 0)
    for wpr in range(1, 257):
        e = K.bit_image_words(wpr, 800)                 # 800 rows: more blocks than any phase of a block's start inside a row needs
        assert len(e) > wpr or wpr * 800 // K.BLOCK_WORDS > 256
        if e.max() > best[0]:
            best = (int(e.max()), wpr, int(e.argmax()))
    assert best == (2286, 254, 42) and best[0] <= K.MS2_CB_WORDS == 2304
    # ... and among the widths a context takes (<= 4000 pixels): 250 words a row, first at block 13, which the widest case of the table has
    acc = max((int(K.bit_image_words(wpr, 800).max()), wpr) for wpr in range(1, 251))
    assert acc == (2250, 250)
    e = K.bit_image_words(K.WIDE.W // 16, K.WIDE.H)
    assert K.WIDE.W == 4000 and int(e.max()) == 2250 and int(e.argmax()) == 13 and len(e) > 14
    assert sorted(cfg.W // 16 for cfg in K.WIDTHS) == [5, 11, 41, 249, 250]
    words = [cfg.W // 16 * cfg.H for cfg in K.WIDTHS]
    assert any(w % 64 and w % 256 and w % 768 for w in words) and (176, 88) in [(cfg.W, cfg.H) for cfg in K.WIDTHS]
    assert K.ORDERED.W % 16 != 0 and K.TOO_WIDE[0] > 4096 and K.TOO_WIDE[0] % 16 == 0 and K.TOO_WIDE in [r[:2] for r in K.REFUSED]
    assert any(cfg.H % 2 for cfg in K.WIDTHS)


def test_context_takes_the_tables_geometries_and_refuses_the_listed_ones():
    import semantic_slam_mapping_amd as ssm
    from semantic_slam_mapping_amd._lib import Config
    lib = ssm.load()

    def plan(w, h):
        cfg = Config()
        lib.ssm_config_default(C.byref(cfg))
        cfg.width, cfg.height, cfg.orb_levels, cfg.orb_features = w, h, 1, 100
        n = C.c_int(0)
        return lib.ssm_debug_fast_plan(C.byref(cfg), None, 0, C.byref(n), None)

    for cfg in K.groups():
        assert plan(cfg.W, cfg.H) == 0, cfg
    for w, h, why in K.REFUSED:
        assert plan(w, h) != 0, "%d x %d (%s) is accepted now: plant it in map_cases" % (w, h, why)
    assert plan(80, 76) == 0 and plan(64, 76) != 0 and plan(80, 75) != 0 and plan(4000, 76) == 0 and plan(4016, 76) != 0      # the table's extremes ARE the extremes


def block_dilate(moving, W, upper=True, lower=True):
    """the kernel's 5 x 5 dilate of one frame's moving pixels, block by block: a block masks its OWN 768 words from its own moving pixels and from those of the
    rows above (`upper`) and below (`lower`) that it classifies itself as its halo; without one of them, what a broken halo would give"""
    H, wpr = moving.shape[0], W // 16
    widx = np.arange(H)[:, None] * wpr + np.arange(W)[None, :] // 16
    out = np.zeros_like(moving)
    for bw0 in range(0, wpr * H, K.BLOCK_WORDS):
        bw1 = bw0 + K.BLOCK_WORDS
        src = moving & ((widx >= bw0) | upper) & ((widx < bw1) | lower)
        out |= (widx >= bw0) & (widx < bw1) & K.dilate5(src[None])[0]
    return out


@pytest.mark.parametrize("name", [n + s for n, _ in K.DILATE for s in ("", ", swapped")])
def test_dilate_cases_plant_single_pixels_at_every_listed_place(oracle, name):
    c = K.case(name)
    W, H = c.cfg.W, c.cfg.H
    lab = K.label_image(c.sem)
    moving = np.isin(lab, K.MOVING)
    pl = c.claims["planted"]
    assert len(set(pl)) == len(pl) == int(moving.sum()) and all(moving[f, y, x] for f, x, y in pl)
    assert np.array_equal(K.keep_mask(c), ~K.dilate5(moving))                     # every other pixel is keepable
    # SINGLE: no other moving pixel in the 9 x 9 neighbourhood of a plant, so no two 5 x 5 masks touch and every masked pixel has one cause
    for f, x, y in pl:
        assert int(moving[f, max(y - 4, 0):y + 5, max(x - 4, 0):x + 5].sum()) == 1, (name, f, x, y)
    assert int((~K.keep_mask(c)).sum()) == sum((min(x + 2, W - 1) - max(x - 2, 0) + 1) * (min(y + 2, H - 1) - max(y - 2, 0) + 1) for f, x, y in pl)
    assert {x for f, x, y in pl if f == 0} >= {0, 1, 2, 13, 14, 15, 16, 17, 18, W - 3, W - 2, W - 1}
    assert {y for f, x, y in pl if f == 1} >= {0, 1, 2, H - 3, H - 2, H - 1}
    assert {y for f, x, y in pl if f == 0} >= {H - 2, H - 1} and {y for f, x, y in pl if f == 1} >= {0, 1}      # the seam between two frames of one launch
    assert {(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)} <= {(x, y) for f, x, y in pl if f == 1}
    # the block boundaries: frame 2 holds their plants and nothing else
    bnd = c.claims["boundary"]
    assert bnd == K.block_boundary_plants(W, H) and {(x, y) for f, x, y in pl if f == 2} == set(bnd)
    nb = (W // 16 * H - 1) // K.BLOCK_WORDS
    assert bool(bnd) == (nb > 0)
    wpr = W // 16
    for k in range(1, nb + 1):
        r, xw = divmod(k * K.BLOCK_WORDS, wpr)
        rows = [y for y in range(r - 2, r + 3) if y < H]
        mine = [(x, y) for x, y in bnd if y in rows]
        assert sorted({y for x, y in mine}) == rows                                # two rows on each side of the boundary's row, and that row
        on = [x for x, y in mine if y == r]
        if xw:                                                                     # the boundary lies inside row r: a plant in each block's part of it
            assert any(x // 16 < xw for x in on) and any(x // 16 >= xw for x in on)
    if name.startswith("dilate 176 x 88"):
        assert divmod(K.BLOCK_WORDS, wpr)[1] == 9                                  # a block that ends in the middle of a row
    if nb:
        m = moving[2]
        assert np.array_equal(block_dilate(m, W), K.dilate5(m[None])[0])           # the model with both halos is the dilate
        for kw in ({"upper": False}, {"lower": False}):                            # ... and a block that drops either halo is WRONG on this frame
            wrong = block_dilate(m, W, **kw) != K.dilate5(m[None])[0]
            assert wrong.sum() >= 10 * nb, (name, kw, int(wrong.sum()))
    for f in range(3):
        for cls in K.MOVING:
            assert (lab[f] == cls).any() or (f == 2 and not bnd)
    tw = K.case(name[:-len(", swapped")] if name.endswith(", swapped") else name + ", swapped")      # the twin has the two classes the other way round
    tm = np.isin(K.label_image(tw.sem), K.MOVING)
    assert np.array_equal(tm, moving) and (K.label_image(tw.sem)[moving] != lab[moving]).all()


def test_pose_cases(oracle):
    c = K.case("poses")
    assert np.array_equal(c.poses[0], np.eye(4))
    for f in (1, 2):
        cl = clouds(oracle, c)[f]
        assert np.allclose(c.poses[f][:3, :3] @ c.poses[f][:3, :3].T, np.eye(3)) and np.linalg.det(c.poses[f][:3, :3]) > 0.999
        assert cl["x"].min() < 0 and cl["y"].min() < 0 and cl["z"].min() < 0
    cl = clouds(oracle, c)[1]
    assert (cl["x"] < 0).mean() > 0.3 and (cl["y"] < 0).mean() > 0.3 and (cl["z"] < 0).mean() > 0.3
    assert K.case("no pose").poses is None and K.case("no pose, division").poses is None


def test_out_of_range_cases(oracle):
    c = K.case("out of range")
    ok = [in_range(cl, c.cfg.leaf) for cl in clouds(oracle, c)]
    assert ok[0].all() and not ok[1].any() and 0.05 < ok[2].mean() < 0.95
    x1 = clouds(oracle, c)[1]["x"]
    assert 1.4e6 < float(np.floor(x1 * np.float32(50.0)).min()) < 1.6e6
    allpts = np.concatenate(clouds(oracle, c))
    tab = oracle.voxel_table(allpts, np.float32(c.cfg.leaf))
    assert int(tab["n"].sum()) == int(sum(o.sum() for o in ok)) < len(allpts)                    # the oracle's table skips exactly those points
    assert oracle.voxel_table(allpts[np.concatenate(ok)], np.float32(c.cfg.leaf)).tobytes() == tab.tobytes()
    s = K.case("out of range, saturating")
    ok = [in_range(cl, s.cfg.leaf) for cl in clouds(oracle, s)]
    assert not ok[0].any() and ok[1].all()
    assert float(np.abs(clouds(oracle, s)[0]["x"] * np.float32(50.0)).min()) > 2.0 ** 31           # beyond what a 32-bit integer holds
    assert [k for k in K.table() if k.claims.get("out_of_range")] == [c, s]
    for k in K.table():
        if not k.claims.get("out_of_range"):
            assert all(in_range(cl, k.cfg.leaf).all() for cl in clouds(oracle, k)), k.name
