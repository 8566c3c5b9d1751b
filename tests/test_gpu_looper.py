"""The device looper (ssm_looper_*, csrc/kernels_bow.hip) on a real MI355X: bit-for-bit equal to the host path of the same library (one arithmetic:
include/ssm/looper_core.h), candidate lists exactly those of tests/looper_ref.py (the independent restatement that sums sequentially), growth, capacity
reporting, ownership, and the exp_mapping driver's --loops mode per frame and in bulk."""
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import looper_ref as R  # noqa: E402
from conftest import CAM, SEED  # noqa: E402

pytestmark = pytest.mark.gpu
HOST = os.path.join(ROOT, "semantic_slam_mapping_amd", "host")
SIZES = (0, 1, 63, 64, 65, 1000, 2024)
VOCABS = {"k10L3": lambda: R.make_vocab(10, 3, 11), "k4L5": lambda: R.make_vocab(4, 5, 12), "irregular": lambda: R.make_irregular_vocab(13)}


@pytest.fixture(scope="module")
def ctx2k():
    """a context whose frames hold up to 2024 descriptors (orb_features 2000 + 3 per level)"""
    import semantic_slam_mapping_amd as ssm
    c = ssm.Context(0, orb_features=2000, max_batch=1, voxel_capacity_log2=16, camera=CAM)
    assert c.cap == 2024
    yield c
    c.close()


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("name", sorted(VOCABS))
def test_device_vectors_equal_host_bits(ctx2k, name):
    import semantic_slam_mapping_amd as ssm
    v = ssm.Vocabulary.from_arrays(*VOCABS[name]())
    lp = ssm.Looper(ctx2k, v)
    rng = np.random.default_rng(41)
    for e, n in enumerate(SIZES):
        q = R.rand_desc(rng, n)
        lp.add(q, 7 * e)
        assert _same(lp.bow(e), v.transform(q)[1:]), (name, n)
    assert len(lp) == len(SIZES)
    lp.close()


def test_device_vectors_equal_host_bits_orbvoc_sized_tree(ctx2k):
    """k = 10, L = 6: 1 111 111 nodes (35.6 MB of descriptors), seeded random bytes"""
    import semantic_slam_mapping_amd as ssm
    arrays = R.make_vocab(10, 6, 0x0B0C, dbow_order=False)
    v = ssm.Vocabulary.from_arrays(*arrays)
    assert (v.nodes, v.words) == (1111111, 1000000)
    lp = ssm.Looper(ctx2k, v)
    q = R.rand_desc(np.random.default_rng(42), 1000)
    lp.add(q, 0)
    wof, ids, vals = v.transform(q)
    assert _same(lp.bow(0), (ids, vals))
    rwof = R.RefVocab(*arrays).words_of(q)
    assert np.array_equal(wof, rwof)                         # and the host path itself descends like the restatement on the large tree
    lp.close()


def test_bulk_add_equals_per_frame_add(ctx):
    import semantic_slam_mapping_amd as ssm
    v = ssm.Vocabulary.from_arrays(*R.make_vocab(10, 3, 11))
    n, W, H = 4, 640, 480
    bufs = [ctx.dev_alloc(n * W * H * 3), ctx.dev_alloc(n * W * H * 2), ctx.dev_alloc(n * W * H * 3), ctx.dev_alloc(n * 128)]
    ctx.synth_frames_dev(SEED, 0, n, *bufs)
    out = ctx.seq_process(*bufs, n, stages=ssm.api.STAGE_ORB)
    bulk, single = ssm.Looper(ctx, v), ssm.Looper(ctx, v)
    bulk.add_dev(out, n, [100, 101, 105, 120])
    ctx.sync()
    res = ctx.seq_fetch(out, n)
    assert int(res["nkp"].min()) > 100
    for f in range(n):
        d = res["desc"][f, :int(res["nkp"][f])]
        single.add(d, [100, 101, 105, 120][f])
        assert _same(bulk.bow(f), single.bow(f)) and _same(bulk.bow(f), v.transform(d)[1:]), f
    assert np.array_equal(bulk.scores(3), single.scores(3))
    a, b = bulk.query(0, n, 0.0, 3), single.query(0, n, 0.0, 3)
    assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and len(a[0]) > 0
    bulk.close(); single.close()
    for p in bufs:
        ctx.dev_free(p)


def test_loop_set_scores_and_candidates(ctx):
    """160 frames x 1000 descriptors, k = 10, L = 5; every fourth frame from 100 on keeps a random half of frame f - 90's descriptors"""
    import semantic_slam_mapping_amd as ssm
    arrays = R.make_vocab(10, 5, 0x5EED, dbow_order=False)
    rv = R.RefVocab(*arrays)
    v = ssm.Vocabulary.from_arrays(*arrays)
    sets, planted = R.loop_set(0x100D)
    F = len(sets)
    frame_ids = list(range(F))
    lp = ssm.Looper(ctx, v)
    host, ref = [], []
    for f, d in enumerate(sets):
        lp.add(d, frame_ids[f])
        host.append(v.transform(d)[1:])
        ref.append(rv.transform(d)[1:])
        assert np.array_equal(host[-1][0], ref[-1][0])
    # scores: device == host path bit for bit on the whole lower triangle
    for q in range(F):
        dev = lp.scores(q)
        hst = np.array([v.score(*host[q], *host[e]) for e in range(q + 1)])
        assert dev.tobytes() == hst.tobytes(), q
    # candidates: exactly the restatement's list, pairs and order
    rs = [[R.score(*ref[q], *ref[e]) for e in range(q + 1)] for q in range(F)]
    flat = np.array([s for row in rs for s in row])
    for thr, interval in ((0.1, 60), (0.015, 60)):
        gap = np.abs(flat - thr).min()
        want = R.candidates(ref, frame_ids, thr, interval, scores=rs)
        print(f"threshold {thr}: {len(want)} candidates, nearest score {gap:.3g} from the threshold")
        assert gap > 1e-9                                    # the condition: no score so close that a last-bit difference could move a candidate
        pairs, sc = lp.query(0, F, thr, interval)
        assert [tuple(p) for p in pairs.tolist()] == [(q, e) for q, e, _ in want]
        assert np.abs(sc - np.array([s for _, _, s in want])).max() <= 8 * 2024 * 2.0 ** -53 if len(want) else True
        if thr == 0.1:
            assert [(q, e) for q, e, _ in want] == planted and len(planted) == 15
    # a sub-range of queries against a fixed prefix of the database
    pairs, sc = lp.query(120, 20, 0.1, 60, against=50)
    assert [tuple(p) for p in pairs.tolist()] == [(q, e) for q, e in planted if 120 <= q < 140 and e < 50]
    lp.close()


def test_growth_capacity_clear_repeat_and_ownership():
    import semantic_slam_mapping_amd as ssm
    base = ssm.live_allocations()
    c = ssm.Context(0, orb_features=1000, max_batch=1, voxel_capacity_log2=16, camera=CAM)
    with_ctx = ssm.live_allocations()
    v = ssm.Vocabulary.from_arrays(*R.make_vocab(10, 3, 11))
    rng = np.random.default_rng(43)
    small = [R.rand_desc(rng, int(rng.integers(5, 60))) for _ in range(5000)]
    planted = [(f, f - 3000) for f in range(4000, 5000, 50)]
    for f, e in planted:
        small[f] = small[e]                                    # identical frames: score 1 up to rounding

    def run():
        lp = ssm.Looper(c, v)
        for f, d in enumerate(small):
            lp.add(d, f)
        assert len(lp) == 5000
        vecs = [lp.bow(e) for e in (0, 1, 255, 256, 257, 1023, 1024, 4095, 4096, 4999)]
        pairs, sc = lp.query(4000, 1000, 0.5, 100)
        return lp, vecs, pairs, sc

    lp, vecs, pairs, sc = run()
    for e, got in zip((0, 1, 255, 256, 257, 1023, 1024, 4095, 4096, 4999), vecs):
        assert _same(got, v.transform(small[e])[1:]), e          # entries written before each growth are intact
    assert len(pairs) > 8 and set(planted) <= set(tuple(p) for p in pairs.tolist())
    with pytest.raises(ssm.SsmError) as e:
        lp.query(4000, 1000, 0.5, 100, cap=8)
    assert e.value.code == -4 and e.value.needed == len(pairs)
    lp.clear()
    assert len(lp) == 0
    lp.add(small[7], 0)
    assert _same(lp.bow(0), v.transform(small[7])[1:])
    lp.close()
    lp2, vecs2, pairs2, sc2 = run()                           # two identical runs: identical bytes
    assert all(_same(a, b) for a, b in zip(vecs, vecs2)) and pairs.tobytes() == pairs2.tobytes() and sc.tobytes() == sc2.tobytes()
    lp2.close()
    assert ssm.live_allocations() == with_ctx
    c.close()
    assert ssm.live_allocations() == base


def _run_driver(tmp_path, name, extra, flags):
    prm = tmp_path / f"{name}.txt"
    base = open(os.path.join(HOST, "parameters_test.txt")).read().replace("end_index=8", "end_index=40").replace("map_output=/tmp/ssm_test_map.pcd", f"map_output={tmp_path}/{name}.pcd")
    prm.write_text(base + extra)
    r = subprocess.run([os.path.join(HOST, "exp_mapping"), str(prm), *flags], capture_output=True, text=True, timeout=600)
    print(r.stdout[-1500:], r.stderr[-1500:])
    assert r.returncode == 0
    return r.stdout


def _field(out, key):
    toks = out.split()
    return toks[toks.index(key) + 1]


def test_driver_loops_per_frame_equals_batched(tmp_path):
    """exp_mapping --loops on the synthetic stream with a vocabulary written here: the per-frame Looper and the bulk BatchLooper print the same loop_fnv"""
    R.write_vocab_text(str(tmp_path / "vocab.txt"), *R.make_vocab(10, 3, 11))
    extra = f"\nlooper_vocab_file={tmp_path}/vocab.txt\nlooper_min_sim_score=0.05\nlooper_min_interval=3\ntracker_chunk=10\nssm_max_batch=4\n"
    a = _run_driver(tmp_path, "perframe", extra + f"loops_output={tmp_path}/loops_a.txt\n", ["--loops"])
    b = _run_driver(tmp_path, "batched", extra + f"loops_output={tmp_path}/loops_b.txt\n", ["--loops", "--batched"])
    k = _run_driver(tmp_path, "key", extra + "looper=1\n", [])
    assert int(_field(a, "loop_candidates")) > 0 and int(_field(a, "keyframes")) > 8
    assert _field(a, "loop_candidates") == _field(b, "loop_candidates") == _field(k, "loop_candidates")
    assert _field(a, "loop_fnv") == _field(b, "loop_fnv") == _field(k, "loop_fnv")
    la = open(tmp_path / "loops_a.txt").read()
    assert la == open(tmp_path / "loops_b.txt").read() and len(la.splitlines()) == int(_field(a, "loop_candidates"))
    off = _run_driver(tmp_path, "off", extra, [])
    assert "loop_candidates" not in off and "loop_fnv" not in off
    # without the flag the looper keys change nothing: the summary line's deterministic fields are those of a run whose file does not mention the looper
    plain = _run_driver(tmp_path, "plain", "", [])
    for key in ("frames", "keyframes", "pose_fnv"):
        assert _field(off, key) == _field(plain, key)
