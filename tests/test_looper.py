"""Looper on the host (no GPU): the vocabulary loader, vocab.transform and vocab.score of libssm_hip.so against tests/looper_ref.py, the independent
restatement of the DBoW2 contract that sums sequentially in float64, the committed golden file, and the rgbd_tutor::Looper class.
Tolerances: the library sums in a lane order of its own (include/ssm/looper_core.h), so a value is compared within 8 m 2^-53 relative (m = the vector's
length: the norm is a sum of m positive terms, each summation order is within (m - 1) 2^-53 of the exact sum) and a score within 8 cap 2^-53 absolute
(cap = 2024 entries: a sum of at most cap terms whose magnitudes total at most 4)."""
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import looper_ref as R  # noqa: E402

HOST = os.path.join(ROOT, "semantic_slam_mapping_amd", "host")
SIZES = (0, 1, 63, 64, 65, 1000, 2024)
SCORE_TOL = 8 * 2024 * 2.0 ** -53
VOCABS = {"k10L3": lambda: R.make_vocab(10, 3, 11), "k4L5": lambda: R.make_vocab(4, 5, 12), "irregular": lambda: R.make_irregular_vocab(13)}
# transform only: a 300-child root over 17- to 20-child groups with planted duplicate descriptors, and three words of which some or all weigh nothing
TRANSFORM_VOCABS = dict(VOCABS, wide=lambda: R.make_wide_vocab(14)[0], tiny=lambda: R.make_tiny_vocab(15), tiny_zero1=lambda: R.make_tiny_vocab(15, zero=(1,)),
                        tiny_zero02=lambda: R.make_tiny_vocab(15, zero=(0, 2)), tiny_zero_all=lambda: R.make_tiny_vocab(15, zero=(0, 1, 2)))


def _ssm():
    import semantic_slam_mapping_amd as ssm
    return ssm


def _load_text(tmp_path, arrays, name="v.txt", **kw):
    p = str(tmp_path / name)
    R.write_vocab_text(p, *arrays, **kw)
    return _ssm().Vocabulary(p)


@pytest.mark.parametrize("name", sorted(VOCABS))
def test_loader_info_and_create_agree(tmp_path, name):
    arrays = VOCABS[name]()
    rv = R.RefVocab(*arrays)
    v = _load_text(tmp_path, arrays)
    assert (v.k, v.L, v.nodes, v.words, v.scoring, v.weighting) == (arrays[0], arrays[1], rv.nodes, rv.words, 0, 0)
    v2 = _ssm().Vocabulary.from_arrays(*arrays)
    assert (v2.nodes, v2.words) == (v.nodes, v.words)
    q = R.rand_desc(np.random.default_rng(1), 700)
    a, b = v.transform(q), v2.transform(q)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_loader_skips_blank_lines(tmp_path):
    arrays = R.make_vocab(3, 2, 5)
    v = _load_text(tmp_path, arrays, trailing_blank=True)
    assert (v.nodes, v.words) == (13, 9)
    p = tmp_path / "blank.txt"
    lines = open(str(tmp_path / "v.txt")).read().split("\n")
    p.write_text("\n" + lines[0] + "\n\n  \n" + "\n".join(lines[1:]) + "\n\n")
    assert _ssm().Vocabulary(str(p)).nodes == 13


def _lines(k=2, L=2):
    """a valid 2-level vocabulary as text lines: ids 1, 2 under the root, 3 .. 6 under them"""
    z = " ".join(["7"] * 32)
    return [f"{k} {L} 0 0", f"0 0 {z} 0", f"0 0 {z} 0", f"1 1 {z} 1.5", f"1 1 {z} 2.5", f"2 1 {z} 0.5", f"2 1 {z} 3"]


@pytest.mark.parametrize("case", ["parent_later", "parent_self", "leaf_with_children", "inner_without_children", "root_without_children", "short_line",
                                  "long_line", "byte_range", "not_a_number", "bad_header", "scoring", "weighting", "k_range", "L_range", "missing_file"])
def test_loader_rejects(tmp_path, case):
    ssm = _ssm()
    ln = _lines()
    z = " ".join(["7"] * 32)
    if case == "parent_later":
        ln[2] = f"5 0 {z} 0"
    elif case == "parent_self":
        ln[2] = f"2 0 {z} 0"
    elif case == "leaf_with_children":
        ln[1] = f"0 1 {z} 1"
    elif case == "inner_without_children":
        ln = ln[:5]                                   # id 2 keeps isLeaf = 0 and loses its children
    elif case == "root_without_children":
        ln = ln[:1]
    elif case == "short_line":
        ln[3] = "1 1 " + " ".join(["7"] * 31) + " 1.5"
    elif case == "long_line":
        ln[3] = ln[3] + " 9"
    elif case == "byte_range":
        ln[3] = "1 1 " + " ".join(["7"] * 31) + " 256 1.5"
    elif case == "not_a_number":
        ln[3] = ln[3].replace("7 7", "7 x", 1)
    elif case == "bad_header":
        ln[0] = "2 2 0"
    elif case == "scoring":
        ln[0] = "2 2 1 0"
    elif case == "weighting":
        ln[0] = "2 2 0 1"
    elif case == "k_range":
        ln[0] = "21 2 0 0"
    elif case == "L_range":
        ln[0] = "2 11 0 0"
    p = tmp_path / "bad.txt"
    if case != "missing_file":
        p.write_text("\n".join(ln) + "\n")
    with pytest.raises(ssm.SsmError) as e:
        ssm.Vocabulary(str(p))
    assert e.value.code == -1 and len(str(e.value)) > 20, str(e.value)          # SSM_E_INVAL and a message


def test_loader_accepts_the_valid_form_of_the_rejection_cases(tmp_path):
    p = tmp_path / "ok.txt"
    p.write_text("\n".join(_lines()) + "\n")
    v = _ssm().Vocabulary(str(p))
    assert (v.nodes, v.words) == (7, 4)
    wof, ids, vals = v.transform(np.full((3, 32), 7, np.uint8))      # every distance ties at 0: the first child wins at both levels
    assert wof.tolist() == [0, 0, 0] and ids.tolist() == [0] and vals.tolist() == [1.0]
    for k, L in ((0, 1), (20, 10)):                                      # the loader's limits, inclusive
        p.write_text("\n".join(_lines(k, L)) + "\n")
        assert _ssm().Vocabulary(str(p)).k == k


@pytest.mark.parametrize("name", sorted(TRANSFORM_VOCABS))
def test_transform_against_restatement(name):
    arrays = TRANSFORM_VOCABS[name]()
    rv = R.RefVocab(*arrays)
    v = _ssm().Vocabulary.from_arrays(*arrays)
    rng = np.random.default_rng(21)
    for n in SIZES:
        q = R.rand_desc(rng, n)
        wof, ids, vals = v.transform(q)
        rwof, rids, rvals = rv.transform(q)
        assert np.array_equal(wof, rwof) and np.array_equal(ids, rids), n
        m = len(ids)
        if n == 0:
            assert m == 0
            continue
        tol = 8 * m * 2.0 ** -53
        rel = np.abs(vals - rvals) / rvals
        print(f"{name} n={n} m={m} max rel {rel.max() if m else 0:.3g} (tol {tol:.3g}) |sum - 1| {abs(vals.sum() - 1) if m else 0:.3g}")
        assert m == 0 or rel.max() <= tol
        assert m == 0 or abs(float(np.sum(vals)) - 1.0) <= tol
        assert np.all(np.diff(ids) > 0)
        zero_words = set(np.nonzero(rv.word_weight <= 0)[0].tolist())
        assert not (set(ids.tolist()) & zero_words)                       # features of zero-weight words are absent
        assert set(ids.tolist()) == set(int(w) for w in wof if int(w) not in zero_words)
    if name == "irregular":
        assert len(zero_words) > 0
    if name == "tiny_zero_all":
        assert len(ids) == 0 and len(wof) == SIZES[-1]                    # a non-empty frame, an empty vector
    if name.startswith("tiny"):
        assert set(wof.tolist()) == {0, 1, 2}                             # runs of about n / 3


def test_wide_vocab_earlier_copy_wins():
    """the 300-child root and the 17- to 20-child groups: a query equal to a duplicated descriptor is at distance 0 from both copies and gets the earlier one,
    on the host path and in the restatement; random queries meet natural ties for the minimum at the root as well"""
    arrays, queries, want = R.make_wide_vocab(14)
    rv = R.RefVocab(*arrays)
    v = _ssm().Vocabulary.from_arrays(*arrays)
    assert (v.k, v.L, v.nodes, rv.cnt[0]) == (20, 2, rv.nodes, 300) and sorted(set(rv.cnt[1:21].tolist())) == [17, 18, 19, 20] and not rv.cnt[21:].any()
    assert len(queries) == len(R.WIDE_ROOT_PAIRS) + len(R.WIDE_GROUPS) * len(R.WIDE_GROUP_PAIRS)
    assert np.array_equal(rv.words_of(queries), want) and np.array_equal(v.transform(queries)[0], want)
    inner = want[len(R.WIDE_ROOT_PAIRS):]                                # the group queries did go down into their groups: words of the groups' leaves
    assert inner.min() >= 280 and len(set(inner.tolist())) == len(inner)
    desc = arrays[4]                                                     # every root child's own descriptor: itself, or the earlier copy
    first = np.arange(300); first[[b for _, b in R.WIDE_ROOT_PAIRS]] = [a for a, _ in R.WIDE_ROOT_PAIRS]
    leaves = np.arange(20, 300)
    assert np.array_equal(v.transform(desc[leaves])[0], first[leaves] - 20) and np.array_equal(rv.words_of(desc[leaves]), first[leaves] - 20)
    q = R.rand_desc(np.random.default_rng(22), 200)
    dist = R._POP[desc[None, :300] ^ q[:, None]].sum(2)
    ties = int(((dist == dist.min(1)[:, None]).sum(1) > 1).sum())
    print(f"{ties} of 200 random queries tie for the minimum at the root")
    assert ties >= 20                                                    # (about one in five: 300 distances of spread 8 around 128, the minimum near 100)
    assert np.array_equal(v.transform(q)[0], rv.words_of(q))


def test_score_matrix_and_candidates_range_restate_score():
    """the vectorised sum of looper_ref is score() bit for bit, and candidates_range with the default arguments is candidates()"""
    arrays = R.make_vocab(10, 2, 21)
    rv = R.RefVocab(*arrays)
    rng = np.random.default_rng(78)
    vecs = [rv.transform(R.rand_desc(rng, n))[1:] for n in (0, 1, 30, 80, 55, 0, 300, 2)]
    S = R.score_matrix(vecs, rv.words)
    for q, a in enumerate(vecs):
        for e, b in enumerate(vecs):
            assert S[q, e] == R.score(*a, *b) and not np.signbit(S[q, e])
    ids = [5, 3, 40, -7, 12, 13, 100, 0]
    assert R.candidates_range(vecs, ids, 0, len(vecs), -1, 0.2, 4) == R.candidates(vecs, ids, 0.2, 4) == R.candidates_range(vecs, ids, 0, len(vecs), -1, 0.2, 4, scores=S)
    got = R.candidates_range(vecs, ids, 2, 3, 7, -1.0, -1)
    assert [(q, e) for q, e, _ in got] == [(q, e) for q in (2, 3, 4) for e in range(7)]      # 0 > -1 and |d| > -1: every pair in range, later entries and self too
    assert R.candidates_range(vecs, ids, 2, 3, 0, -1.0, -1) == [] and R.candidates_range(vecs, ids, 2, 0, -1, -1.0, -1) == []


def test_transform_capacity_reports_needed():
    ssm = _ssm()
    v = ssm.Vocabulary.from_arrays(*R.make_vocab(10, 3, 11))
    q = R.rand_desc(np.random.default_rng(3), 300)
    _, ids, _ = v.transform(q)
    with pytest.raises(ssm.SsmError) as e:
        v.transform(q, cap=len(ids) - 1)
    assert e.value.code == -4 and e.value.needed == len(ids)


def test_score_against_restatement():
    arrays = R.make_vocab(10, 3, 11)
    v = _ssm().Vocabulary.from_arrays(*arrays)
    rng = np.random.default_rng(31)
    base = R.rand_desc(rng, 2024)
    vecs = []
    for n, share in ((2024, 0), (2024, 1500), (1000, 900), (65, 65), (64, 10), (1, 1)):
        q = R.rand_desc(rng, n); q[:share] = base[:share]
        vecs.append(v.transform(q)[1:])
    worst = worst_exact = 0.0
    for a in vecs:
        for b in vecs:
            s, r, x = v.score(*a, *b), R.score(*a, *b), R.score_exact(*a, *b)
            worst = max(worst, abs(s - r)); worst_exact = max(worst_exact, abs(s - x), abs(r - x))
            assert abs(s - r) <= SCORE_TOL, (s, r)
            assert abs(s - x) <= SCORE_TOL and abs(r - x) <= SCORE_TOL, (s, r, x)      # both summation orders against the sum without one
        assert abs(v.score(*a, *a) - 1.0) <= SCORE_TOL
    print(f"worst |score - restatement| {worst:.3g}, worst |host or restatement - exact| {worst_exact:.3g} (tol {SCORE_TOL:.3g})")
    assert R.score_exact(*vecs[0], np.zeros(0, np.int32), np.zeros(0)) == 0.0
    empty = (np.zeros(0, np.int32), np.zeros(0))
    assert v.score(*empty, *vecs[0]) == 0.0 and v.score(*vecs[0], *empty) == 0.0 and v.score(*empty, *empty) == 0.0
    ids, vals = vecs[0]
    a = (ids[0::2], vals[0::2]); b = (ids[1::2], vals[1::2])
    assert v.score(*a, *b) == 0.0 and v.score(*b, *a) == 0.0            # disjoint: exactly 0


def test_golden_file():
    g = np.load(os.path.join(ROOT, "tests", "golden", "looper.npz"))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "looper.npz")) < 200 * 1024
    v = _ssm().Vocabulary.from_arrays(int(g["k"]), int(g["L"]), g["parent"], g["is_leaf"], g["desc"], g["weight"])
    assert (v.nodes, v.words) == (1111, 1000)
    vecs = []
    for i in range(8):
        wof, ids, vals = v.transform(g["sets"][i])
        m = int(g["vec_len"][i])
        assert np.array_equal(wof, g["words"][i]) and np.array_equal(ids, g["vec_ids"][i, :m])
        assert (np.abs(vals - g["vec_vals"][i, :m]) / g["vec_vals"][i, :m]).max() <= 8 * m * 2.0 ** -53
        vecs.append((ids, vals))
    for q in range(8):
        for e in range(8):
            assert abs(v.score(*vecs[q], *vecs[e]) - g["scores"][q, e]) <= SCORE_TOL
    assert all(g["scores"][i + 4, i] > 0.2 for i in range(4)) and g["scores"][0, 1] < 0.2      # the shared halves show


def test_looper_class_host_path(tmp_path):
    """host/test_looper.cpp: rgbd_tutor::Looper without a context (the host path): ids, strict comparisons, the float threshold, late queries"""
    subprocess.run(["make", "-C", HOST, "test_looper"], check=True, stdout=subprocess.DEVNULL)
    arrays = R.make_vocab(10, 3, 11)
    R.write_vocab_text(str(tmp_path / "vocab.txt"), *arrays)
    out = subprocess.run([os.path.join(HOST, "test_looper"), str(tmp_path), str(tmp_path / "vocab.txt")], capture_output=True, text=True, timeout=300)
    assert "ALL PASSED" in out.stdout and out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert out.stdout.count("PASS ") >= 5
