"""CPU tests of label fusion: ssm_relabel_host -- the contract's arithmetic of include/ssm/relabel_core.h, one thread, no GPU -- against the
numpy restatement tests/relabel_ref.py byte for byte (labels, packed votes, every info field, the label image from BGR) on the shared case list; the list's own
properties; the order of the views; refusals; empty calls; the host function as a stand-alone C++ program, also under AddressSanitizer +
UndefinedBehaviorSanitizer; and the new kernels' register use."""
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import relabel_ref as R  # noqa: E402

HOST = os.path.join(ROOT, "semantic_slam_mapping_amd", "host")
CASES = list(R.cases())
_cache = {}
U = R.U


def ref_of(name):
    """-> (case, restatement), computed once and shared"""
    if name not in _cache:
        cs = R.cases()[name]()
        _cache[name] = (cs, R.run_case(cs))
    return _cache[name]


def host_relabel(cs, order=None, **kw):
    import semantic_slam_mapping_amd as ssm
    order = list(range(len(cs["views"]))) if order is None else order
    views = [(cs["views"][k]["depth"], cs["views"][k]["label"], cs["views"][k]["camera"]) for k in order]
    return ssm.relabel_host(views, [cs["T_views"][k] for k in order], cs["pts"], cs["T_cloud"], **dict(cs["params"], **kw))


def equal(got, ref, what=""):
    labels, votes, info = got
    assert labels.dtype == np.uint32 and votes.dtype == np.uint64
    assert np.array_equal(votes, ref["votes"]), (what, "votes", np.nonzero(votes != ref["votes"])[0][:5])
    assert np.array_equal(labels, ref["labels"]), (what, "labels", np.nonzero(labels != ref["labels"])[0][:5])
    assert labels.tobytes() == ref["labels"].tobytes() and votes.tobytes() == ref["votes"].tobytes(), what
    for f in R.INFO_FIELDS:
        assert info[f] == ref["info"][f], (what, f, info[f], ref["info"][f])


@pytest.mark.parametrize("name", CASES)
def test_host_equals_restatement(name):
    cs, ref = ref_of(name)
    before = cs["pts"].tobytes()
    got = host_relabel(cs)
    equal(got, ref, name)
    assert cs["pts"].tobytes() == before
    I = got[2]
    assert I["n_filled"] <= I["n_changed"] <= I["n_voted"] <= I["n_supported"] <= I["n_in"] == len(cs["pts"])
    assert I["n_voted"] <= I["pairs_voted"] <= I["pairs_supported"] <= I["n_in"] * len(cs["views"])


def test_label_image_equals_restatement():
    import semantic_slam_mapping_amd as ssm
    rng = np.random.default_rng(7)
    lab = rng.integers(0, 13, (9, 31)).astype(np.uint8)
    lab[lab == 12] = U
    sem = R.bgr_of_labels(lab)
    near = np.array(R.PALETTE, np.uint8)[rng.integers(0, 12, (9, 31))]
    near[..., 1] ^= 1                                        # one bit off a palette colour: unknown
    for img, want in ((sem, lab), (near, np.full((9, 31), U, np.uint8))):
        got = ssm.relabel_labels_host(img)
        assert got.dtype == np.uint8 and np.array_equal(got, want) and np.array_equal(R.labels_of_bgr(img), want)
    assert ssm.relabel_labels_host(np.zeros((0, 5, 3), np.uint8)).shape == (0, 5)


def count(votes, l):
    return (int(votes) >> (5 * l)) & 31


def test_cases_are_what_they_are_for():
    """every case changes some labels and fills some unknowns; the list holds every situation the rule distinguishes"""
    seen = set()
    for name in CASES:
        cs, ref = ref_of(name)
        assert ref["info"]["n_changed"] > ref["info"]["n_filled"] > 0, name
        if len({v["depth"].shape for v in cs["views"]}) > 1:
            seen.add("two_sizes")
        if any((v["label"] == U).any() for v in cs["views"]):
            seen.add("view_255")
        if (cs["pts"]["label"] > 11).any():
            seen.add("cloud_above_11")
        for i, y in enumerate(ref["why"]):
            c, L0, L1 = y["counts"], int(cs["pts"]["label"][i]), int(ref["labels"][i])
            best = max(c)
            assert sum(k << (5 * l) for l, k in enumerate(c)) == int(ref["votes"][i]) and best <= 31
            if best == 31:
                seen.add("count_31")
            if L0 <= 11 and best and c[L0] == best and c.count(best) > 1:
                assert L1 == L0
                seen.add("tie_own_wins_" + str(c[L0]))
            if (L0 > 11 or c[L0] < best) and c.count(best) > 1 and best >= cs["params"].get("min_votes", 2):
                assert L1 == c.index(best)
                seen.add("tie_lowest_id")
            if 0 < best < cs["params"].get("min_votes", 2):
                assert L1 == L0
                seen.add("below_min_votes")
            if y["guarded"]:
                seen.add("guarded")
    assert seen >= {"two_sizes", "view_255", "cloud_above_11", "count_31", "tie_own_wins_1", "tie_lowest_id", "below_min_votes", "guarded"}, seen
    # the constructed points are the situations their names say
    cs, ref = ref_of("constructed")
    cs0, ref0 = ref_of("constructed_no_guard")
    equal(host_relabel(cs), ref, "constructed")                  # what is asserted of the restatement below holds for the product
    equal(host_relabel(cs0), ref0, "constructed_no_guard")
    at = {n: i for i, n in enumerate(cs["names"])}
    L = lambda n: int(ref["labels"][at[n]])          # noqa: E731
    assert L("tie_own_wins") == 3 and ref["why"][at["tie_own_wins"]]["counts"][3] == ref["why"][at["tie_own_wins"]]["counts"][5] == 1
    assert L("tie_lowest_id") == 4 and L("tie_lowest_id_own_loses") == 4
    assert L("edge_guard") == 2 and ref["why"][at["edge_guard"]]["guarded"] == [1] and int(ref0["labels"][at["edge_guard"]]) == 6      # the withheld vote flips the result
    assert L("below_min_votes") == U and count(ref["votes"][at["below_min_votes"]], 5) == 1
    assert L("cloud_label_12") == 1 and L("cloud_label_upper_bytes") == 1 and L("overruled") == 10
    assert L("occluded_view_does_not_vote") == 0 and L("seen_through_view_does_not_vote") == 0 and L("agreement") == 11 and L("nothing") == U and L("behind") == 4
    assert ref["votes"][at["behind"]] == 1 << 20 and ref["votes"][at["nothing"]] == 0
    cs, ref = ref_of("saturated")
    equal(host_relabel(cs), ref, "saturated")
    assert len(cs["views"]) == 16 and cs["params"]["own_weight"] == 15
    assert ref["labels"].tolist() == [3, 8, 2, 6, 0, 0] and count(ref["votes"][0], 3) == 31 and count(ref["votes"][4], 0) == count(ref["votes"][4], 11) == 15


@pytest.mark.parametrize("name", ["constructed", "saturated", "posed_160x120"])
def test_order_of_views_does_not_matter(name):
    cs, ref = ref_of(name)
    v = len(cs["views"])
    rng = np.random.default_rng(11)
    for order in (list(range(v))[::-1], rng.permutation(v).tolist()):
        equal(host_relabel(cs, order), ref, (name, order))


def test_empty_calls():
    import semantic_slam_mapping_amd as ssm
    cs, ref = ref_of("constructed")
    labels, votes, info = ssm.relabel_host([], [], cs["pts"], cs["T_cloud"])                      # v = 0: only the own vote, nothing changes
    own = cs["pts"]["label"]
    assert np.array_equal(labels, own) and info == dict(n_in=len(own), n_supported=0, n_voted=0, n_changed=0, n_filled=0, pairs_supported=0, pairs_voted=0)
    assert np.array_equal(votes, np.where(own <= 11, np.uint64(1) << (5 * np.minimum(own, 11)).astype(np.uint64), np.uint64(0)))
    labels, votes, info = host_relabel(dict(cs, pts=cs["pts"][:0]))                               # n = 0
    assert len(labels) == 0 and len(votes) == 0 and info == dict(n_in=0, n_supported=0, n_voted=0, n_changed=0, n_filled=0, pairs_supported=0, pairs_voted=0)
    labels, votes, info = ssm.relabel_host([], [], cs["pts"][:0], cs["T_cloud"])
    assert len(labels) == 0 and info["n_in"] == 0


def test_refusals():
    import semantic_slam_mapping_amd as ssm
    cs, _ = ref_of("constructed")
    V = cs["views"][0]
    one = [(V["depth"], V["label"], V["camera"])]

    def refused(views=one, T_views=None, T_cloud=np.eye(4), **kw):
        with pytest.raises(ssm.SsmError) as e:
            ssm.relabel_host(views, [np.eye(4)] * len(views) if T_views is None else T_views, cs["pts"], T_cloud, **kw)
        assert e.value.code == -1, e.value          # SSM_E_INVAL

    refused(views=one * 17)
    for kw in (dict(radius=-1), dict(radius=4), dict(edge_guard=-1), dict(edge_guard=2), dict(own_weight=-1), dict(own_weight=16), dict(min_votes=0), dict(min_votes=32),
               dict(tol_abs=-0.01), dict(tol_abs=float("nan")), dict(tol_abs=2.0e6), dict(tol_rel_ppm=-1), dict(tol_rel_ppm=1000001), dict(z_min=-1.0),
               dict(z_min=float("inf")), dict(z_min=float("nan"))):
        refused(**kw)
        refused(views=[], **kw)                                       # the parameters are checked without a view too
    bad = np.eye(4); bad[1, 3] = float("nan")
    refused(T_views=[bad])
    refused(T_cloud=bad)
    bad = np.eye(4); bad[0, 0] = float("inf")
    refused(T_views=[bad])
    for cam in ((float("nan"), 0, 64, 64, 1000), (0, 0, float("inf"), 64, 1000), (0, 0, 64, 64, 0.0), (0, 0, 64, 64, -1.0), (0, 0, 64, 64, 1.0e6 + 1), (0, 0, 64, 64, float("nan"))):
        refused(views=[(V["depth"], V["label"], cam)])
    ssm.relabel_host([(V["depth"], V["label"], (0, 0, 64, 64, 1.0e6))], [np.eye(4)], cs["pts"], np.eye(4))          # the largest scale is legal
    ssm.relabel_host(one * 16, [np.eye(4)] * 16, cs["pts"], np.eye(4))                                              # and so are 16 views
    lib = ssm.load()
    assert lib.ssm_relabel_host(None, None, 1, None, 0, None, None, None, None, None) == -1
    assert lib.ssm_relabel_labels_host(None, 3, None) == -1 and lib.ssm_relabel_labels_host(None, -1, None) == -1
    with pytest.raises(TypeError):
        ssm.relabel_params(no_such=1)
    P = ssm.relabel_params()
    assert (P.radius, P.edge_guard, P.own_weight, P.min_votes, P.tol_abs, P.tol_rel_ppm, P.z_min) == (1, 1, 1, 2, 0.05, 20000, 0.1)


def test_host_function_as_a_program_and_under_sanitizers():
    """host/test_relabel_core.cpp: a stand-alone program (its own main, no library, no device) over the host function, built plainly and with
    -fsanitize=address,undefined"""
    for target in ("test_relabel_core", "test_relabel_core_san"):
        subprocess.run(["make", "-s", "-C", HOST, target], check=True, capture_output=True, timeout=600)
        r = subprocess.run([os.path.join(HOST, target)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "ALL PASSED" in r.stdout and "FAIL" not in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


def test_kernels_neither_spill_nor_use_scratch():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    from test_abi import _resource_usage
    usage = _resource_usage("kernels_relabel.hip")
    for n, k in (("relabel_kernelILi0E", 1), ("relabel_kernelILi1E", 1), ("relabel_kernelILi2E", 1), ("relabel_labels_kernel", 1)):
        hit = [f for f in usage if n in f]
        assert len(hit) == k, (n, sorted(usage))
        u = usage[hit[0]]
        assert u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0 and u.get("ScratchSize [bytes/lane]", 0) == 0, (hit[0], u)
