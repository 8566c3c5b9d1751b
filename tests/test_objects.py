"""CPU tests of object extraction: ssm_objects_cells_host and ssm_objects_host -- the contract's arithmetic of include/ssm/objects_core.h, one
thread, no GPU -- against the numpy / scipy restatement tests/objects_ref.py byte for byte (records, object_id, per-point ids, info) on the shared case lists of
tests/objects_cases.py; the lists' own properties; order independence; refusals; the capacity rule; the host functions as a stand-alone C++ program, also under
AddressSanitizer + UndefinedBehaviorSanitizer; and the new kernels' register use."""
import ctypes as C
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import objects_ref as R  # noqa: E402
import objects_cases as OC  # noqa: E402
import grid_cases as GC  # noqa: E402

HOST = os.path.join(ROOT, "semantic_slam_mapping_amd", "host")
TILE = (32, 32)          # the patterns only need A tile size here; the GPU tests ask the library for its own
ARR = ("cls", "obstacle_label", "ground_q", "top_q", "n_high")
_cache = {}


def memo(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def host_cells(cs, cap=None, **kw):
    import semantic_slam_mapping_amd as ssm
    return ssm.objects_cells_host(*[cs[k] for k in ARR], cap=cap, **dict(cs["params"], **kw))


def ref_cells(cs, **kw):
    return R.cells(*[cs[k] for k in ARR], **dict(cs["params"], **kw))


def host_run(cs, clouds=None, T=None, **kw):
    import semantic_slam_mapping_amd as ssm
    return ssm.objects_host(cs["clouds"] if clouds is None else clouds, cs["T_clouds"] if T is None else T, grid=cs["grid"], **dict(cs["params"], **kw))


def equal_records(got, ref, what):
    assert got.dtype == ref.dtype == R.OBJECT_DTYPE and got.shape == ref.shape, (what, got.shape, ref.shape)
    for f in R.OBJECT_DTYPE.names:
        assert np.array_equal(got[f], ref[f]), (what, f, got[f][:8], ref[f][:8])
    assert got.tobytes() == ref.tobytes(), what


def test_layouts():
    import semantic_slam_mapping_amd as ssm
    from semantic_slam_mapping_amd._lib import ObjectsParams, ObjectsInfo
    assert ssm.OBJECT_DTYPE == R.OBJECT_DTYPE and R.OBJECT_DTYPE.itemsize == 104 and C.sizeof(ObjectsInfo) == 64
    P = ObjectsParams(); ssm.load().ssm_objects_params_default(C.byref(P))
    D = R.DEFAULTS
    assert (P.label_mask, P.connectivity, P.min_cells, P.min_points, P.min_height) == (D["label_mask"], 8, 2, 20, 0.3) and P.label_mask == 0xE00
    assert ssm.objects_params(labels=[9, 11, 9]).label_mask == (1 << 9) | (1 << 11)
    with pytest.raises(TypeError):
        ssm.objects_params(min_cell=1)


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("pattern", list(OC.patterns()))
def test_cells_host_equals_restatement_on_the_patterns(pattern, conn):
    for nx, ny in OC.shapes(*TILE):
        cs = OC.cell_case(OC.patterns()[pattern](nx, ny, *TILE), dict(OC.LOOSE, connectivity=conn))
        rec, oid, info, _ = ref_cells(cs)
        got, goid, ginfo = host_cells(cs)
        equal_records(got, rec, (pattern, nx, ny))
        assert goid.dtype == np.int32 and np.array_equal(goid, oid) and ginfo == info, (pattern, nx, ny, ginfo, info)
        assert info["kept"] == info["components"] == len(rec) and int(rec["cells"].sum()) == info["member_cells"] == int((cs["obstacle_label"] != 255).sum())


@pytest.mark.parametrize("name", list(OC.cell_cases()))
def test_cells_host_equals_restatement_on_the_cases(name):
    cs = OC.cell_cases()[name]()
    for conn in (4, 8):
        rec, oid, info, _ = ref_cells(cs, connectivity=conn)
        got, goid, ginfo = host_cells(cs, connectivity=conn)
        equal_records(got, rec, (name, conn))
        assert np.array_equal(goid, oid) and ginfo == info, (name, conn, ginfo, info)


@pytest.mark.parametrize("name", list(OC.cloud_cases()))
def test_host_equals_restatement(name):
    cs = memo(name, OC.cloud_cases()[name])
    rec, oid, ids, info, g = memo(("ref", name), lambda: R.run(cs["clouds"], cs["T_clouds"], cs["grid"], **cs["params"]))
    before = [c.tobytes() for c in cs["clouds"]]
    got, goid, gids, ginfo = host_run(cs)
    equal_records(got, rec, name)
    assert np.array_equal(goid, oid) and gids.dtype == np.int32 and np.array_equal(gids, ids) and ginfo == info, (name, ginfo, info)
    assert [c.tobytes() for c in cs["clouds"]] == before
    # the invariant: every object's points are its cells' HIGH points
    assert np.array_equal(got["n_points"], got["cell_points"].astype(np.uint32)) and int(got["n_points"].sum()) == ginfo["object_points"] == int((gids >= 0).sum())
    assert ginfo["n_in"] == sum(len(c) for c in cs["clouds"]) == len(gids)
    for k, o in enumerate(got):
        assert int((gids == k).sum()) == o["n_points"] and o["n_label"] <= o["n_points"]
        assert o["x_min_q"] <= o["sum_x"] // max(int(o["n_points"]), 1) <= o["x_max_q"] and o["z_max_q"] == o["top_q"]


def lib_cells(cs, **kw):
    """ssm_objects_cells_host's answer in the restatement's form (records, object_id, info, every component's (root, verdict)): the verdicts of the rejected
    components come from a second call under rules that keep everything, each judged by the library's own counts; checked against the restatement on the way"""
    rec, oid, info = host_cells(cs, **kw)
    every = host_cells(cs, **dict(kw, min_cells=0, min_points=0, min_height=0.0))[0]
    kept = set(rec["root"].tolist())
    P = R.params_of(dict(cs["params"], **kw))
    verdicts = []
    for o in every:
        v = "kept" if int(o["root"]) in kept else "rejected_cells" if o["cells"] < P["min_cells"] else "rejected_points" if o["cell_points"] < P["min_points"] else "rejected_height"
        verdicts.append((int(o["root"]), v))
    assert sum(v == "kept" for _, v in verdicts) == info["kept"] and all(sum(v == k for _, v in verdicts) == info[k] for k in ("rejected_cells", "rejected_points", "rejected_height"))
    want = ref_cells(cs, **kw)
    equal_records(rec, want[0], "lib_cells")
    assert np.array_equal(oid, want[1]) and info == want[2] and verdicts == want[3]
    return rec, oid, info, verdicts


def lib_run(clouds, T_clouds, grid, **params):
    """ssm_objects_host's answer in the restatement's form (records, object_id, ids, info)"""
    import semantic_slam_mapping_amd as ssm
    return ssm.objects_host(clouds, T_clouds, grid=grid, **params)


def test_cases_are_what_they_are_for():
    """the properties the case lists are for, asserted on what the LIBRARY gives (ssm_objects_cells_host, ssm_objects_host; lib_cells also ties every answer to the
    restatement): a diagonal contact, labels that never join, the mask, each rejection rule and their order, the numbering, long chains, the street's objects"""
    cs = OC.diagonal_contact()
    assert lib_cells(cs, connectivity=8)[2]["components"] == 1 and lib_cells(cs, connectivity=4)[2]["components"] == 2
    assert lib_cells(cs, connectivity=8)[0]["root"].tolist() == [6] and lib_cells(cs, connectivity=4)[0]["root"].tolist() == [6, 12]
    for conn, want in ((4, [(6, 3), (8, 1), (12, 1)]), (8, [(6, 3), (8, 2)])):          # adjacent cells of different labels never join
        rec = lib_cells(OC.different_labels(), connectivity=conn)[0]
        assert list(zip(rec["root"].tolist(), rec["cells"].tolist())) == want, (conn, rec)
    rec, oid, info, _ = lib_cells(OC.label_outside_mask())
    assert info["member_cells"] == 2 and rec["root"].tolist() == [10] and (oid >= 0).sum() == 2          # labels 4, 8 and 12 form nothing
    assert lib_cells(OC.label_outside_mask(), labels=[4, 8])[2]["member_cells"] == 10
    assert lib_cells(OC.not_an_obstacle(), connectivity=8)[2]["components"] == 2
    rec, oid, info, verdicts = lib_cells(OC.rejections())
    assert [v for _, v in verdicts] == ["kept", "rejected_cells", "rejected_points", "rejected_height", "rejected_cells", "rejected_points", "kept"]
    assert (info["kept"], info["rejected_cells"], info["rejected_points"], info["rejected_height"]) == (2, 2, 2, 1) and rec["root"].tolist() == [0, 54]
    cs = OC.rejections()          # each rule alone: relaxing exactly that rule lets the component in
    one = lib_cells(cs, min_cells=1)[2]          # B is kept, E goes on to the points rule
    assert (one["kept"], one["rejected_cells"], one["rejected_points"]) == (3, 0, 3)
    assert lib_cells(cs, min_points=19)[2]["rejected_points"] == 1 and lib_cells(cs, min_height=511 / 1024)[2]["rejected_height"] == 0
    assert lib_cells(cs, min_cells=1, min_points=0)[2]["rejected_height"] == 3          # E and F come to the height rule once the earlier ones let them pass
    rec, oid, _, _ = lib_cells(OC.ids_ascend())
    assert rec["root"].tolist() == sorted(rec["root"].tolist()) == [5, 6, 21, 30, 35] and [int(oid.ravel()[r]) for r in rec["root"]] == [0, 1, 2, 3, 4]
    tw, th = TILE
    for name in ("serpentine", "spiral", "u_shape"):          # one chain across every tile
        L = OC.patterns()[name](2 * tw + 2, 2 * th + 3, tw, th)
        rec = lib_cells(OC.cell_case(L, dict(OC.LOOSE, connectivity=4)))[0]
        assert len(rec) == 1 and rec["root"][0] == 0 and rec["cells"][0] == (L != 255).sum() > 2 * (tw + th), name
    L = OC.checkerboard(tw + 1, th + 1, tw, th)
    assert len(lib_cells(OC.cell_case(L, dict(OC.LOOSE, connectivity=4)))[0]) == (L != 255).sum() and len(lib_cells(OC.cell_case(L, dict(OC.LOOSE, connectivity=8)))[0]) == 1
    L = OC.tile_corner(2 * tw + 2, 2 * th + 3, tw, th)
    assert L[th - 1, tw - 1] == L[th, tw] == 9 and len(lib_cells(OC.cell_case(L, dict(OC.LOOSE, connectivity=8)))[0]) == 2 == len(lib_cells(OC.cell_case(L, dict(OC.LOOSE, connectivity=4)))[0]) - 2
    assert len(lib_cells(OC.cell_case(OC.rings(tw + 1, th, tw, th)))[0]) == th // 2
    # the street: the two cars are one object under 8 and two under 4; the pedestrian's single cell and the flat bike fall to the defaults; the fence is no member
    rec8 = memo(("ref", "street_m3"), lambda: lib_run(*[OC.cloud_cases()["street_m3"]()[k] for k in ("clouds", "T_clouds", "grid")], min_cells=1))[0]
    assert sorted(rec8["label"].tolist()) == [9, 10]
    cs = memo("street_conn4", OC.cloud_cases()["street_conn4"])
    assert sorted(lib_run(cs["clouds"], cs["T_clouds"], cs["grid"], **cs["params"])[0]["label"].tolist()) == [9, 9, 10]
    cs = memo("street_defaults", OC.cloud_cases()["street_defaults"])
    rec, _, ids, info = lib_run(cs["clouds"], cs["T_clouds"], cs["grid"])
    assert rec["label"].tolist() == [9] and info["rejected_cells"] == 1 and info["rejected_height"] == 1 and 0 < (ids >= 0).sum() < info["n_in"]
    car = rec[0]
    assert car["n_label"] < car["n_points"] and (car["cx_min"], car["cx_max"], car["cy_min"], car["cy_max"]) == (4, 9, 4, 8)          # some of its points carry other labels


@pytest.mark.parametrize("name", ["street_m3", "street_posed", "street_conn4"])
def test_order_does_not_matter(name):
    cs = memo(name, OC.cloud_cases()[name])
    want = host_run(cs)
    rng = np.random.default_rng(5)
    perms = [rng.permutation(len(c)) for c in cs["clouds"]]
    clouds = [c[p] for c, p in zip(cs["clouds"], perms)][::-1]
    got = host_run(cs, clouds, cs["T_clouds"][::-1])
    equal_records(got[0], want[0], name)
    assert np.array_equal(got[1], want[1]) and got[3] == want[3]
    # the per-point ids follow their points
    off = np.cumsum([0] + [len(c) for c in cs["clouds"]])
    back = np.concatenate([want[2][off[k]:off[k + 1]][perms[k]] for k in range(len(perms))][::-1])
    assert np.array_equal(got[2], back)


def test_capacity():
    """cap = K - 1: SSM_E_CAPACITY, *n_out = K, nothing else written; cap = K: everything"""
    import semantic_slam_mapping_amd as ssm
    from semantic_slam_mapping_amd._lib import ObjectsInfo, ObjectsParams, GridParams
    lib = ssm.load()
    cs = OC.ids_ascend()
    rec, oid, info, _ = ref_cells(cs)
    K = len(rec)
    P = ssm.objects_params(**cs["params"])
    a = [np.ascontiguousarray(cs[k]) for k in ARR]
    for cap, rc_want in ((K - 1, -4), (0, -4), (K, 0)):
        out = np.full(K + 1, 7, np.uint8).view(np.uint8).repeat(104).view(R.OBJECT_DTYPE); ids = np.full(oid.shape, -7, np.int32); I = ObjectsInfo(); I.kept = -7; n = C.c_int(-7)
        rc = lib.ssm_objects_cells_host(*[x.ctypes.data for x in a], 6, 6, C.byref(P), out.ctypes.data, cap, C.byref(n), ids.ctypes.data, C.byref(I))
        assert rc == rc_want and n.value == K
        if rc:
            assert (out.view(np.uint8) == 7).all() and (ids == -7).all() and I.kept == -7 and "need 5" in lib.ssm_last_error(None).decode()
        else:
            assert out[:K].tobytes() == rec.tobytes() and (out[K:].view(np.uint8) == 7).all() and np.array_equal(ids, oid) and I.kept == K
    cs = memo("street_m3", OC.cloud_cases()["street_m3"])
    want = host_run(cs)
    K = len(want[0])
    assert K == 2
    with pytest.raises(ssm.SsmError) as e:
        ssm.objects_host(cs["clouds"], cs["T_clouds"], grid=cs["grid"], cap=K - 1, **cs["params"])
    assert e.value.code == -4
    keep, ptrs, n, Tc, m = ssm.api._pack_clouds(cs["clouds"], cs["T_clouds"], True)
    G = ssm.grid_params(**cs["grid"]); P = ssm.objects_params(**cs["params"])
    out = np.full((K + 1) * 104, 7, np.uint8); oid = np.full((G.ny, G.nx), -7, np.int32); ids = np.full(int(n.sum()), -7, np.int32); I = ObjectsInfo(); I.kept = -7; k = C.c_int(-7)
    rc = lib.ssm_objects_host(ptrs, n.ctypes.data, Tc.ctypes.data, m, C.byref(G), C.byref(P), out.ctypes.data, K - 1, C.byref(k), oid.ctypes.data, ids.ctypes.data, C.byref(I))
    assert rc == -4 and k.value == K and (out == 7).all() and (oid == -7).all() and (ids == -7).all() and I.kept == -7
    rc = lib.ssm_objects_host(ptrs, n.ctypes.data, Tc.ctypes.data, m, C.byref(G), C.byref(P), out.ctypes.data, K, C.byref(k), None, None, None)          # the optional outputs
    assert rc == 0 and out[:K * 104].tobytes() == want[0].tobytes() and (out[K * 104:] == 7).all()


def test_refusals():
    import semantic_slam_mapping_amd as ssm
    lib = ssm.load()
    cs = OC.ids_ascend()
    street = memo("street_m3", OC.cloud_cases()["street_m3"])
    nan, inf = float("nan"), float("inf")
    bad = (dict(connectivity=6), dict(connectivity=0), dict(connectivity=-8), dict(min_cells=-1), dict(min_points=-1), dict(min_height=-0.1), dict(min_height=nan), dict(min_height=inf))
    for kw in bad:
        with pytest.raises(ssm.SsmError) as e:
            host_cells(cs, **kw)
        assert e.value.code == -1 and "objects:" in str(e.value), kw
        with pytest.raises(ssm.SsmError) as e:
            host_run(street, **kw)
        assert e.value.code == -1, kw
    for kw in (dict(min_cells=0), dict(min_points=0), dict(min_height=0.0), dict(min_height=1e300), dict(label_mask=0), dict(label_mask=0xFFFFFFFF), dict(min_cells=2 ** 31 - 1)):
        host_cells(cs, **kw)          # the limits themselves are legal
    assert len(host_cells(cs, min_height=1e300)[0]) == 0 and len(host_cells(cs, label_mask=0)[0]) == 0
    # a grid whose extent leaves +-2^20 m, on each side
    for g in (dict(x0=-1048576.5), dict(x0=1048576.0 - 5.0), dict(y0=-1048577.0), dict(y0=1048576.0 - 4.0), dict(cell=1e5)):
        with pytest.raises(ssm.SsmError) as e:
            ssm.objects_host(street["clouds"], street["T_clouds"], grid=dict(street["grid"], **g))
        assert e.value.code == -1 and "2^20" in str(e.value), g
    ssm.objects_host(street["clouds"], street["T_clouds"], grid=dict(street["grid"], x0=-1048576.0, y0=1048576.0 - 5.0))          # the limit itself
    with pytest.raises(ssm.SsmError):
        ssm.objects_host(street["clouds"], street["T_clouds"], grid=dict(street["grid"], cell=-1.0))          # the grid's own refusals come through
    # null arguments, sizes, the same cloud twice, 2^31 points
    P = ssm.objects_params(); a = [np.ascontiguousarray(cs[k]) for k in ARR]; ptr = [x.ctypes.data for x in a]; n = C.c_int(0); out = np.zeros(36, R.OBJECT_DTYPE)
    for i in range(5):
        args = list(ptr); args[i] = None
        assert lib.ssm_objects_cells_host(*args, 6, 6, C.byref(P), out.ctypes.data, 36, C.byref(n), None, None) == -1
    assert lib.ssm_objects_cells_host(*ptr, 6, 6, C.byref(P), out.ctypes.data, 36, None, None, None) == -1
    assert lib.ssm_objects_cells_host(*ptr, 6, 6, C.byref(P), None, 36, C.byref(n), None, None) == -1
    assert lib.ssm_objects_cells_host(*ptr, 6, 6, C.byref(P), out.ctypes.data, -1, C.byref(n), None, None) == -1
    for nx, ny in ((0, 6), (6, 0), (-1, 6), (4097, 4096)):
        assert lib.ssm_objects_cells_host(*ptr, nx, ny, C.byref(P), out.ctypes.data, 36, C.byref(n), None, None) == -1
    assert lib.ssm_objects_cells_host(*ptr, 6, 6, None, out.ctypes.data, 36, C.byref(n), None, None) == 0 and n.value == len(R.cells(*[cs[k] for k in ARR])[0])          # null parameters: the defaults
    one = street["clouds"][0]
    with pytest.raises(ssm.SsmError) as e:
        ssm.objects_host([one, one], [GC.EYE, GC.EYE], grid=street["grid"])
    assert e.value.code == -1 and "twice" in str(e.value)
    G = ssm.grid_params(**street["grid"]); T2 = np.ascontiguousarray(np.tile(np.eye(4).reshape(16), 2))
    two = (C.c_void_p * 2)(one.ctypes.data, one[1:].ctypes.data)
    for counts, word in (([2 ** 31 - 1, 1], "2^31"), ([1, -1], "negative")):
        cnt = np.ascontiguousarray(counts, np.int32)
        assert lib.ssm_objects_host(two, cnt.ctypes.data, T2.ctypes.data, 2, C.byref(G), C.byref(P), out.ctypes.data, 36, C.byref(n), None, None, None) == -1
        assert word in lib.ssm_last_error(None).decode()
    assert lib.ssm_objects_host(two, None, T2.ctypes.data, 2, C.byref(G), C.byref(P), out.ctypes.data, 36, C.byref(n), None, None, None) == -1
    assert lib.ssm_objects_host(two, np.ones(2, np.int32).ctypes.data, T2.ctypes.data, 2, C.byref(G), C.byref(P), out.ctypes.data, 36, None, None, None, None) == -1


def test_host_functions_as_a_program_and_under_sanitizers():
    """host/test_objects_core.cpp: a stand-alone program (its own main, no library, no device) over the host functions, built plainly and with
    -fsanitize=address,undefined"""
    for target in ("test_objects_core", "test_objects_core_san", "test_objects_stub", "test_objects_stub_san"):          # (_stub: the sanitizer builds' stand-in entry points)
        subprocess.run(["make", "-s", "-C", HOST, target], check=True, capture_output=True, timeout=600)
        r = subprocess.run([os.path.join(HOST, target)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "ALL PASSED" in r.stdout and "FAIL" not in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


def test_kernels_neither_spill_nor_use_scratch():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    from test_abi import _resource_usage
    usage = _resource_usage("kernels_objects.hip")
    names = ("obj_begin_kernel", "obj_local_kernelILi4E", "obj_local_kernelILi8E", "obj_merge_kernelILi4E", "obj_merge_kernelILi8E", "obj_flatten_kernel", "obj_clear_records_kernel",
             "obj_figures_kernel", "obj_keep_kernel", "obj_compact_kernel", "obj_paint_kernel", "obj_points_begin_kernel", "obj_points_kernel", "obj_points_runs_kernel")
    for n in names:
        hit = [k for k in usage if n in k]
        assert len(hit) == 1, (n, sorted(usage))
        u = usage[hit[0]]
        assert u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0 and u.get("ScratchSize [bytes/lane]", 0) == 0, (hit[0], u)
