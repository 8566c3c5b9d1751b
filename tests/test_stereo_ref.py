"""The independent references of tests/stereo_ref.py against the CPU oracle on every constructed edge case of tests/test_gpu_stereo_edges.py, and
the property each case is built to have (a case that drifts off the kernel path it exists for fails here).  No GPU."""
import numpy as np
import pytest
import stereo_ref as R

GFTT = R.gftt_cases()
SPECKLE = R.speckle_cases()


@pytest.mark.parametrize("name", sorted(GFTT))
def test_gftt_reference_matches_oracle(oracle, name):
    img, mc, q, md, prop = GFTT[name]
    eig = oracle.min_eigen_map(img)
    p = R.gftt_properties(eig, q, md)
    assert prop(p), (name, {k: v for k, v in p.items() if k != "pts"})
    ref = R.gftt_select(eig, mc, q, md)
    o = oracle.gftt(img, mc, q, md)
    assert len(ref) > 0 and ref.tobytes() == o.tobytes()


def test_gftt_case_paths():
    """the GPU paths the GFTT cases reach, from their properties: more rounds than the 1 + 12 launched, more stronger neighbours than the 32-entry
    list, windows wider than the bit-image scan (rad > 15), more candidates than the w*h/4 + 1024 list, and max_corners cutting a run of ties"""
    from oracle.binding import Oracle
    o = Oracle()
    props = {n: R.gftt_properties(o.min_eigen_map(c[0]), c[2], c[3]) for n, c in GFTT.items()}
    assert min(props["chain_rising"]["rounds"], props["chain_falling"]["rounds"]) >= 64 > 1 + 12
    assert props["cluster_md15"]["max_stronger"] > R.GFTT_DEPS
    assert any(np.ceil(GFTT[n][3]) > 15 and props[n]["max_stronger"] > 0 for n in GFTT)
    for n in ("plateau_64x48_md8", "plateau_64x48_md1", "plateau_64x48_md1.5"):
        h, w = GFTT[n][0].shape
        assert props[n]["candidates"] > w * h // 4 + 1024
    assert props["plateau_64x48_md1"]["kept"] > 64 * 48 // 4 + 1024                  # more kept corners than the list: the top-cap search
    # ties: all candidates share one value, so the cut at max_corners lies inside the run
    img, mc, q, md, _ = GFTT["ties_cut"]
    e = o.min_eigen_map(img); pts = props["ties_cut"]["pts"]
    vals = e[pts[:, 1].astype(int), pts[:, 0].astype(int)]
    assert vals[mc - 1] == vals[mc]
    # the exact-boundary pairs: 16 px apart kept at minDistance 16 but not at 16.5; 244 = 12^2 + 10^2 kept at 15.5 but not at 16
    e = o.min_eigen_map(GFTT["pairs_md16.0"][0])
    assert [len(R.gftt_select(e, 0, 0.001, md)) for md in (15.5, 16.0, 16.5)] == [6, 5, 3]


@pytest.mark.parametrize("name", sorted(SPECKLE))
def test_speckle_reference_matches_oracle(oracle, name):
    maps, nv, ms, md, prop = SPECKLE[name]
    assert prop(R.speckle_components(maps[0], nv, md)), name
    for m in maps:
        assert np.array_equal(R.filter_speckles(m, nv, ms, md), oracle.filter_speckles(m, nv, ms, md))
        med = R.median3_s16(m)
        assert np.array_equal(med, oracle.median3_s16(m))
        assert np.array_equal(R.filter_speckles(med, nv, ms, md), oracle.filter_speckles(med, nv, ms, md))


def test_speckle_reference_sizes_and_joins():
    """the hand-counted facts behind the speckle cases: removal at exactly max_size, survival at max_size + 1, joins at max_diff, splits above it"""
    a = np.full((5, 6), R.NV, np.int16); a[1:3, 1:3] = 7
    assert (R.filter_speckles(a, R.NV, 4, 0) == R.NV).all()
    assert np.array_equal(R.filter_speckles(a, R.NV, 3, 0), a)
    b = a.copy(); b[1:3, 3:5] = 9
    assert np.array_equal(R.filter_speckles(b, R.NV, 4, 2), b) and (R.filter_speckles(b, R.NV, 4, 1) == R.NV).all()
    m = np.array([[-32768, 32767, 0], [5, 5, 5]], np.int16)
    assert np.array_equal(R.median3_s16(m), np.array([[5, 5, 5], [5, 5, 5]], np.int16))
