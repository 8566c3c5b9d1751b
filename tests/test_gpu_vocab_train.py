"""The device vocabulary trainer (csrc/kernels_vocab_train.hip, csrc/ssm_vocab_train.hip) against the host function, byte for byte -- the exported arrays
(parent, is_leaf, descriptors, weights), word_of_feature and the report -- with the numpy restatement tests/vocab_train_ref.py as the third leg (tree, words
and report exact; the host function's weights are checked against it on the CPU in tests/test_vocab_train.py).  Sizes: a root of 1, 2 and around every
multiple of the wave (64), the block (256) and four blocks (1024), plus 4097, with the narrowest and the two widest trees; every k path at 600; a deep tree with
leaves above L; thousands of tiny nodes on the last level; low-entropy descriptors (ties in assignment, majority and seeding); max_iters 1 and 2; empty frames;
the one-pass hook on constructed states (an empty cluster, exact half splits, equidistant centres, a node across chunk boundaries); and the trained vocabulary
in the device looper: the candidates of the planted loop set are exactly the planted pairs."""
import functools
import os
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import looper_ref as LR  # noqa: E402
import vocab_train_ref as V  # noqa: E402

pytestmark = pytest.mark.gpu
EDGE_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097)

CASES = {}
for _n in EDGE_SIZES:
    CASES[f"root{_n}_k2_L1"] = (lambda n=_n: V.rand_sets(100 + n, n, min(n, 3)), 2, 1, 32)
    CASES[f"edge{_n}_k17_L2"] = (lambda n=_n: V.rand_sets(200 + n, n, min(n, 3)), 17, 2, 32)
    CASES[f"edge{_n}_k20_L2"] = (lambda n=_n: V.rand_sets(300 + n, n, min(n, 3)), 20, 2, 32)
for _k in (2, 3, 16, 17, 20):
    CASES[f"n600_k{_k}"] = (lambda k=_k: V.rand_sets(400 + k, 600, 5), _k, 3, 32)
CASES["deep_n300_k2_L6"] = (lambda: V.rand_sets(4, 300, 3), 2, 6, 32)
CASES["tiny_nodes_n4096_k20_L3"] = (lambda: V.rand_sets(5, 4096, 8), 20, 3, 32)
for _n, _b in ((600, 1), (600, 2), (2000, 1), (2000, 2)):
    CASES[f"low_entropy_n{_n}_bytes{_b}"] = (lambda n=_n, b=_b: V.low_entropy_sets(500 + n + b, n, b), 10, 3, 32)
for _it in (1, 2, 32):
    CASES[f"iters{_it}_low"] = (lambda: V.low_entropy_sets(3, 2000, 2), 10, 3, _it)
    CASES[f"iters{_it}_rand"] = (lambda: V.rand_sets(6, 1500, 6), 10, 3, _it)
CASES["empty_frames"] = (lambda: V.with_empty_frames(V.rand_sets(7, 700, 6)), 10, 3, 32)
CASES["clustered"] = (lambda: V.clustered_sets(4)[0], 8, 2, 32)


def _ssm():
    import semantic_slam_mapping_amd as ssm
    return ssm


@functools.lru_cache(maxsize=None)
def _ref(name):
    make, k, L, iters = CASES[name]
    return V.train(make(), k, L, iters)


def _same_vocab(a, b):
    assert a.report == b.report
    for x, y, what in zip(a.arrays(), b.arrays(), ("parent", "is_leaf", "desc", "weight")):
        assert x.tobytes() == y.tobytes(), what
    assert a.word_of_feature.tobytes() == b.word_of_feature.tobytes()
    assert (a.k, a.L, a.nodes, a.words) == (b.k, b.L, b.nodes, b.words)


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_host_equals_restatement(ctx, name):
    ssm = _ssm()
    make, k, L, iters = CASES[name]
    sets = make()
    host = ssm.Vocabulary.train(sets, k, L, iters)
    dev = ssm.Vocabulary.train(sets, k, L, iters, ctx=ctx)
    _same_vocab(dev, host)
    r = _ref(name)
    parent, leaf, desc, _ = dev.arrays()
    assert np.array_equal(parent, r["parent"]) and np.array_equal(leaf, r["is_leaf"]) and np.array_equal(desc, r["desc"])
    assert np.array_equal(dev.word_of_feature, r["word_of_feature"]) and dev.report == r["report"]
    host.close(); dev.close()


def test_cases_reach_every_path():
    """what the list above is there for, counted by the restatement: ties of both kinds, early seeding stops, capped nodes, emptied clusters, leaves above L"""
    total = V.Events()
    for name in ("low_entropy_n600_bytes1", "low_entropy_n2000_bytes2", "iters1_low", "clustered", "deep_n300_k2_L6"):
        total.add(_ref(name)["events"])
    for ev in V.EVENT_NAMES:
        assert total[ev] > 0, ev
    assert _ref("tiny_nodes_n4096_k20_L3")["report"]["nodes"] > 3000
    assert _ref("deep_n300_k2_L6")["report"]["levels"] == 6


@pytest.mark.parametrize("state", list(V.kmajority_states()))
def test_one_pass_on_constructed_states(ctx, state):
    ssm = _ssm()
    desc, node_of, cluster_of, centres = V.kmajority_states()[state]
    ev = V.Events()
    rc, ra = V.kmajority_ref(desc, node_of, cluster_of, centres, ev)
    hc, ha = ssm.vocab_kmajority(desc, node_of, cluster_of, centres)
    dc, da = ssm.vocab_kmajority(desc, node_of, cluster_of, centres, ctx=ctx)
    assert dc.tobytes() == hc.tobytes() and da.tobytes() == ha.tobytes()
    assert np.array_equal(dc, rc) and np.array_equal(da, ra)
    assert ev[{"empty": "emptied_clusters", "half_split": "majority_ties", "equidistant": "assign_ties", "wide": "emptied_clusters"}[state]] > 0


def test_trained_on_the_device_the_looper_finds_the_planted_pairs(ctx):
    ssm = _ssm()
    sets, planted = LR.loop_set(5, frames=60, n=200, first_revisit=40, every=4, back=35)
    v = ssm.Vocabulary.train(sets, 10, 3, 32, ctx=ctx)
    host = ssm.Vocabulary.train(sets, 10, 3, 32)
    _same_vocab(v, host)
    lp = ssm.Looper(ctx, v)
    for f, d in enumerate(sets):
        lp.add(d, f)
    pairs, scores = lp.query(0, 60, 0.38, 3)
    lp.close()
    assert [tuple(p) for p in pairs.tolist()] == sorted(planted)
    assert scores.min() > 0.5
