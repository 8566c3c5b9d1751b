"""The named PnP cases of tests/pnp_cases.py on the CPU: the C oracle (oracle/pnp.c), the Python restatement (tests/golden/pyref.py) and the host class
(include/ssm/pnp.h over pnp_core.h) agree on every one, and the census proves that the list reaches the solver paths its cases are named for -- the device
comparison of test_gpu_pnp_paths.py runs the same list, so this is what says which paths the device has been shown to restate."""
import numpy as np
import pytest
import pnp_cases as pc
from test_pnp import CAM, _host

ALL_FINITE = pc.FINITE + pc.GEOMETRIC
ids = lambda cs: [c.name for c in cs]
same_pose = pc.same_pose


@pytest.mark.parametrize("case", ALL_FINITE, ids=ids(ALL_FINITE))
def test_oracle_equals_python_restatement(oracle, case):
    img, obj, T0, mi = pc.get(case)
    ok_o, T_o, inl_o = oracle.pnp_solve(img, obj, CAM, T0, min_inliers=mi)
    ok_p, T_p, inl_p, _ = pc.pyref_result(case)
    assert ok_o == ok_p and inl_o.tolist() == inl_p.tolist()
    assert T_o.tobytes() == T_p.tobytes()                         # one numeric contract: the same bits (test_pnp.py compares this pair the same way)


@pytest.mark.parametrize("case", ALL_FINITE + pc.NONFINITE + pc.SIZE, ids=ids(ALL_FINITE + pc.NONFINITE + pc.SIZE))
def test_host_equals_oracle(oracle, tmp_path, case):
    img, obj, T0, mi = pc.get(case)
    ok_o, T_o, inl_o = oracle.pnp_solve(img, obj, CAM, T0, min_inliers=mi)
    ok_h, T_h, inl_h = _host(tmp_path, img, obj, T0)
    assert ok_o == ok_h and inl_o.tolist() == inl_h.tolist()
    assert same_pose(T_o, T_h)


def test_nonfinite_cases_are_decided(oracle):
    """what the contract's plain IEEE arithmetic makes of the edges that are not sound (oracle; the host and the device are compared with it elsewhere)"""
    res = {c.name: oracle.pnp_solve(*pc.get(c)[:2], CAM, pc.get(c)[2], min_inliers=10) for c in pc.NONFINITE}
    for name, (ok, T, inl) in res.items():
        assert ok and np.isfinite(T).all(), name
    assert 7 in res["nan_coordinate"][2].tolist()                 # NaN > 5.991 is false: the edge is never counted out
    assert 11 not in res["inf_pixel"][2].tolist()                 # inf > 5.991: out


def test_census_reaches_every_event():
    tot = pc.census(ALL_FINITE)
    assert [e for e in pc.EVENTS if tot[e] == 0] == []


@pytest.mark.parametrize("case", ALL_FINITE, ids=ids(ALL_FINITE))
def test_case_reaches_the_paths_it_is_named_for(case):
    ev = pc.pyref_result(case)[3]
    assert set(ev) <= set(pc.EVENTS + pc.NOT_REACHED)
    assert [e for e in case.reaches if ev.get(e, 0) == 0] == []


def test_events_do_not_change_the_result():
    import pyref
    c = pc.FINITE[0]
    img, obj, T0, mi = pc.get(c)
    ok, T, inl = pyref.pnp_solve(img, obj, CAM, T0, min_inliers=mi)
    ok_e, T_e, inl_e, _ = pc.pyref_result(c)
    assert ok == ok_e and T.tobytes() == T_e.tobytes() and inl.tolist() == inl_e.tolist()


@pytest.mark.parametrize("case", ALL_FINITE + pc.NONFINITE, ids=ids(ALL_FINITE + pc.NONFINITE))
def test_trailing_depthless_rows_change_nothing(oracle, case):
    """the device tests pad a case to 9000 rows to move its edge list from LDS to global memory: the pose and the leading flags must not depend on that"""
    img, obj, T0, mi = pc.get(case)
    ok, T, inl = oracle.pnp_solve(img, obj, CAM, T0, min_inliers=mi)
    imgp, objp, _, _ = pc.padded(case)
    okp, Tp, inlp = oracle.pnp_solve(imgp, objp, CAM, T0, min_inliers=mi)
    assert okp and len(imgp) == 9000
    assert same_pose(T, Tp) and inlp.tolist() == inl.tolist()
