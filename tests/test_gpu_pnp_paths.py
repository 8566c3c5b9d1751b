"""ssm_pnp_solve (csrc/kernels_pnp.hip) on the named cases of tests/pnp_cases.py, whose census (test_pnp_cases.py) says which Levenberg paths they reach: every length of
a run of trials up to the tenth, both early terminations, one to four rounds, the re-marked outlier, the fourth round with edges out; degenerate geometry; inputs whose
intermediates are not finite.  The device restates ssm_pnp::solve with speculative streaks of trials, a system built beside the first candidate and a decide / clear /
set bookkeeping, so every case runs in the cluster of eight blocks and in one block, with the edge list in LDS and in global memory; the contract is bit-exact and
oracle/pnp.c is the reference: success, count, flag list and pose bytes, no tolerance (an entry that is NaN on both sides is equal).  Also the list sizes up to the
accepted maximum, the sizes around the LDS capacity, the refusal above the maximum, the wrap of the exchange ring's pass numbers, and the tracker's chain in its
1, 2, 4 and 8 block forms on match tables built from the cases."""
import os
import time
import numpy as np
import pytest
import pnp_cases as pc
from test_pnp import CAM

pytestmark = pytest.mark.gpu
KCAM = (CAM[2], CAM[3], CAM[0], CAM[1])            # (fx, fy, cx, cy)
CASES = pc.FINITE + pc.GEOMETRIC + pc.NONFINITE
GLOBAL_N = 9000                                    # rows of a padded case: above the LDS capacity (asserted below)


def _solve_and_compare(c, ref, img, obj, T0, mi):
    ok_o, T_o, inl_o = ref
    ok_d, T_d, flags, m = c.pnp_solve(img, obj, KCAM, T0, min_inliers=mi)
    assert ok_d == ok_o and m == len(inl_o)
    assert np.flatnonzero(flags).tolist() == inl_o.tolist()
    assert pc.same_pose(T_d, T_o)
    return T_d, flags, m


_refs = {}


def _ref(oracle, case, rows=None):
    """(arrays, oracle result) of a case, or of the case padded to `rows`; computed once"""
    if (case.name, rows) not in _refs:
        img, obj, T0, mi = pc.get(case) if rows is None else pc.padded(case, rows)
        _refs[(case.name, rows)] = ((img, obj, T0, mi), oracle.pnp_solve(img, obj, CAM, T0, min_inliers=mi))
    return _refs[(case.name, rows)]


@pytest.fixture(scope="module")
def cluster():
    import semantic_slam_mapping_amd as ssm
    c = ssm.Context(0, width=640, height=480, max_batch=1)
    assert c.pnp_solve_blocks() == 8
    yield c
    still = c.pnp_solve_blocks()
    c.close()
    assert still == 8                                              # (a time-out would have moved the context to one block: the comparisons above were not the cluster's)


@pytest.fixture(scope="module")
def one_block(oracle):
    """a context of its own whose first call sees the exchange's time-out word set (test hook), which moves it to one block per solve for good"""
    import semantic_slam_mapping_amd as ssm
    c = ssm.Context(0, width=640, height=480, max_batch=1)
    old = os.environ.get("SSM_PNP_TEST_TIMEOUT")
    os.environ["SSM_PNP_TEST_TIMEOUT"] = "1"
    try:
        args, ref = _ref(oracle, pc.FINITE[0])
        _solve_and_compare(c, ref, *args)
    finally:
        if old is None:
            del os.environ["SSM_PNP_TEST_TIMEOUT"]
        else:
            os.environ["SSM_PNP_TEST_TIMEOUT"] = old
    assert c.pnp_solve_blocks() == 1
    yield c
    still = c.pnp_solve_blocks()
    c.close()
    assert still == 1


def test_the_padded_cases_are_beyond_the_lds_capacity():
    import semantic_slam_mapping_amd as ssm
    cap = ssm.pnp_lds_edge_capacity()
    assert max(len(pc.get(c)[0]) for c in CASES) <= cap < GLOBAL_N
    assert 4096 < cap < 6250                                       # 24 bytes per edge beside a static part between 10 KB and 60 KB


@pytest.mark.parametrize("memory", ["lds", "global"])
@pytest.mark.parametrize("form", ["cluster", "one_block"])
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_device_equals_oracle(request, oracle, case, form, memory):
    c = request.getfixturevalue(form)
    args, ref = _ref(oracle, case, None if memory == "lds" else GLOBAL_N)
    _solve_and_compare(c, ref, *args)
    assert c.pnp_solve_blocks() == (8 if form == "cluster" else 1)


@pytest.mark.parametrize("form", ["cluster", "one_block"])
@pytest.mark.parametrize("case", pc.SIZE, ids=[c.name for c in pc.SIZE])
def test_largest_list(request, oracle, case, form):
    """65535 correspondences: 64 edges per thread, so the last bit of a thread's decision mask is in use"""
    args, ref = _ref(oracle, case)
    assert len(args[0]) == 65535
    _solve_and_compare(request.getfixturevalue(form), ref, *args)


def test_one_more_than_the_largest_list_is_refused(cluster, oracle):
    from semantic_slam_mapping_amd.api import SsmError
    with pytest.raises(SsmError, match="at most 65535 correspondences"):
        cluster.pnp_solve(np.zeros((65536, 2), np.float32), np.ones((65536, 3), np.float32), KCAM, np.eye(4))
    args, ref = _ref(oracle, pc.FINITE[1])
    _solve_and_compare(cluster, ref, *args)                        # the context goes on working
    assert cluster.pnp_solve_blocks() == 8


@pytest.mark.parametrize("form", ["cluster", "one_block"])
@pytest.mark.parametrize("over", [0, 1])
def test_at_the_lds_capacity_and_one_more(request, oracle, form, over):
    """the longest list the kernels keep in LDS, and the shortest they keep in global memory"""
    import semantic_slam_mapping_amd as ssm
    args, ref = _ref(oracle, pc.sized(ssm.pnp_lds_edge_capacity() + over))
    _, flags, m = _solve_and_compare(request.getfixturevalue(form), ref, *args)
    assert m > 0.8 * len(flags)


def test_ring_epoch_wrap(oracle):
    """4100 consecutive cluster solves on one context: the ring's pass tags start from a 12-bit launch number, which wraps after 4096 calls; the ring must be zeroed then,
    or a granule left by the launch of 4096 calls ago with the same tag would be read as a sum.  Every result equals the first, the first equals the oracle."""
    import semantic_slam_mapping_amd as ssm
    c = ssm.Context(0, width=640, height=480, max_batch=1)
    try:
        args, ref = _ref(oracle, pc.WRAP)
        img, obj, T0, mi = args
        T1, flags1, m1 = _solve_and_compare(c, ref, *args)
        t0 = time.perf_counter()
        bad = []
        for k in range(1, 4100):
            ok, T, flags, m = c.pnp_solve(img, obj, KCAM, T0, min_inliers=mi)
            if not (ok == ref[0] and m == m1 and T.tobytes() == T1.tobytes() and flags.tobytes() == flags1.tobytes()):
                bad.append(k)
        print("ring epoch wrap: 4099 solves in %.2f s" % (time.perf_counter() - t0))
        assert bad == []
        assert c.pnp_solve_blocks() == 8                           # all of them were the cluster's
    finally:
        c.close()


# ---- the tracker's chain (pnp_chain_kernel: the same pc_solve behind the chain's own gather) in every block count, on match tables built from the cases
CHAIN_CASES = [c for c in pc.FINITE + pc.GEOMETRIC
               if np.array_equal(pc.get(c)[2], np.eye(4)) and int((pc.get(c)[1] != 0).any(1).sum()) >= 15]


def _two_frame_tables(c, img, obj, cap):
    """a two-frame ssm_seq_out_dev by hand: frame 0's positions are the case's points, frame 1's key points its pixels, frame 1's match table against frame 0 pairs
    entry i with entry i -- frame 1 is then solved from the identity start with the case's correspondences (those with depth)"""
    from semantic_slam_mapping_amd._lib import SeqOutDev
    from semantic_slam_mapping_amd.api import KEYPOINT_DTYPE, DMATCH_DTYPE
    n, R = len(img), c.R
    kps = np.zeros((2, cap), KEYPOINT_DTYPE); kps["x"][1, :n] = img[:, 0]; kps["y"][1, :n] = img[:, 1]
    pos = np.zeros((2, cap, 3), np.float32); pos[0, :n] = obj
    matches = np.zeros((2, R, cap), DMATCH_DTYPE); matches["queryIdx"][1, R - 1, :n] = np.arange(n); matches["trainIdx"][1, R - 1, :n] = np.arange(n)
    nmatch = np.full((2, R), -1, np.int32); nmatch[1, R - 1] = n
    arrays = [kps, np.zeros((2, cap, 32), np.uint8), pos, np.full(2, n, np.int32), matches, nmatch, np.zeros(2, np.int32)]
    ptrs = []
    for a in arrays:
        ptrs.append(c.dev_alloc(a.nbytes)); c.h2d(ptrs[-1], a)
    return SeqOutDev(*ptrs, cap, R), ptrs


@pytest.fixture(scope="module")
def chain_ctx():
    import semantic_slam_mapping_amd as ssm
    c = ssm.Context(0, width=640, height=480, max_batch=2, camera=CAM)
    yield c
    c.close()


@pytest.mark.parametrize("case", CHAIN_CASES, ids=[c.name for c in CHAIN_CASES])
def test_chain_in_every_block_count(chain_ctx, oracle, case):
    import semantic_slam_mapping_amd as ssm
    c = chain_ctx
    img, obj, T0, mi = pc.get(case)
    has = (obj != 0).any(1)                                        # the chain's gather drops the correspondences without depth
    ok_o, T_o, inl_o = oracle.pnp_solve(img[has], obj[has], CAM, np.eye(4), min_inliers=mi)
    tracked = len(inl_o) >= 15
    seq, ptrs = _two_frame_tables(c, img, obj, 64)
    try:
        host = ssm.Tracker(c, use_device=False)
        try:
            ph, ih = host.run(seq, 2)
        finally:
            host.close()
        assert tuple(int(v) for v in ih[1]) == (1, int(tracked), int(has.sum()), len(inl_o))
        assert ph[0].tobytes() == np.eye(4).tobytes() and ph[1].tobytes() == (T_o if tracked else np.eye(4)).tobytes()
        for b in (1, 2, 4, 8):
            dev = ssm.Tracker(c, use_device=True, blocks=b)
            try:
                pd, idv = dev.run(seq, 2)
                assert idv.tobytes() == ih.tobytes() and pd.tobytes() == ph.tobytes(), b
                assert dev.last_error() == "" and dev.stats() == (1, 1), b          # frame 1 ran on the device, no downgrade
            finally:
                dev.close()
    finally:
        for p in ptrs:
            c.dev_free(p)
