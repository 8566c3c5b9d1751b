"""Independent restatement of the vocabulary-training contract in numpy: hierarchical k-majority tree, farthest-point seeding, nearest-centre
assignment with the lowest centre on ties, bitwise majority with an even split giving 1, breadth-first ids, weight = log(F / Ni).  It works on unpacked bits and
distance matrices, node by node, and shares no code with the library.  It also COUNTS the events the tests must have seen (`Events`), and holds the seeded input
generators the CPU and the GPU tests share."""
import math
import numpy as np

_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)
EVENT_NAMES = ("assign_ties", "majority_ties", "seeding_stops", "capped_nodes", "emptied_clusters", "leaves_above_L")


class Events(dict):
    def __init__(self):
        super().__init__({n: 0 for n in EVENT_NAMES})

    def add(self, other):
        for n in EVENT_NAMES:
            self[n] += other[n]


def _dist(X, Cs):
    """n x nc Hamming distances"""
    return _POP[X[:, None, :] ^ Cs[None, :, :]].sum(2)


def kmajority_pass(X, a, Cs, ev=None):
    """step 4 once for one node: rows X (n x 32), clusters a, centres Cs (nc x 32) -> (new centres, new clusters)"""
    ev = ev if ev is not None else Events()
    Cs = Cs.copy()
    bits = np.unpackbits(X, axis=1).astype(np.int64)
    for j in range(len(Cs)):
        mem = a == j
        cnt = int(mem.sum())
        if cnt == 0:
            ev["emptied_clusters"] += 1                                     # keeps its centre
            continue
        ones = bits[mem].sum(0)
        ev["majority_ties"] += int((2 * ones == cnt).sum())
        Cs[j] = np.packbits((2 * ones >= cnt).astype(np.uint8))
    d = _dist(X, Cs)
    na = d.argmin(1)                                                        # the first minimum: the lowest centre on ties
    ev["assign_ties"] += int(((d == d.min(1, keepdims=True)).sum(1) > 1).sum())
    return Cs, na


def train(desc_sets, k=10, L=5, max_iters=32):
    """-> dict(parent, is_leaf, desc, weight, ni, word_of_feature, report, events, levels_of_nodes)"""
    sets = [np.asarray(d, np.uint8).reshape(-1, 32) for d in desc_sets]
    F = len(sets)
    D = np.concatenate(sets)
    N = len(D)
    frame_of = np.concatenate([np.full(len(d), f, np.int64) for f, d in enumerate(sets)])
    ev = Events()
    parent, is_leaf, desc = [], [], []
    leaf_of = np.zeros(N, np.int64)
    cur = [(0, np.arange(N))]
    passes = [0] * 10
    levels = capped = 0
    level = 0
    while cur:
        if level > 0:
            levels = level
        nxt = []
        for nid, idx in cur:
            X = D[idx]
            word = level == L
            if not word and nid != 0 and (X == X[0]).all():
                word = True
                ev["leaves_above_L"] += 1
            if word:
                is_leaf[nid - 1] = 1
                leaf_of[idx] = nid
                continue
            Cs = [X[0]]
            m = _dist(X, X[:1])[:, 0]
            for _ in range(1, k):
                if m.max() == 0:
                    ev["seeding_stops"] += 1
                    break
                i = int(m.argmax())                                         # the first maximum: the lowest index
                Cs.append(X[i])
                m = np.minimum(m, _dist(X, X[i:i + 1])[:, 0])
            Cs = np.stack(Cs)
            d = _dist(X, Cs)
            a = d.argmin(1)
            ev["assign_ties"] += int(((d == d.min(1, keepdims=True)).sum(1) > 1).sum())
            n_pass = 0
            for it in range(1, max_iters + 1):
                n_pass = it
                Cs, na = kmajority_pass(X, a, Cs, ev)
                changed = bool((na != a).any())
                a = na
                if not changed:
                    break
                if it == max_iters:
                    capped += 1
                    ev["capped_nodes"] += 1
            passes[level] = max(passes[level], n_pass)
            for j in range(len(Cs)):
                mem = a == j
                if mem.any():
                    parent.append(nid); is_leaf.append(0); desc.append(Cs[j])
                    nxt.append((len(parent), idx[mem]))
        cur = nxt
        level += 1
    parent = np.array(parent, np.int32); is_leaf = np.array(is_leaf, np.uint8); desc = np.stack(desc).astype(np.uint8)
    word_of_id = np.full(len(parent) + 1, -1, np.int64)
    leaves = np.nonzero(is_leaf)[0]
    word_of_id[leaves + 1] = np.arange(len(leaves))
    wof = word_of_id[leaf_of]
    ni = np.zeros(len(leaves), np.int64)
    for w, cnt in zip(*np.unique(np.unique(np.stack([wof, frame_of], 1), axis=0)[:, 0], return_counts=True)):
        ni[w] = cnt
    weight = np.zeros(len(parent), np.float64)
    weight[leaves] = [math.log(F / int(x)) for x in ni]
    report = {"nodes": len(parent) + 1, "words": len(leaves), "levels": levels, "capped_nodes": capped, "passes": passes}
    return {"parent": parent, "is_leaf": is_leaf, "desc": desc, "weight": weight, "ni": ni, "word_of_feature": wof.astype(np.int32), "report": report, "events": ev}


# ---- seeded inputs ----------------------------------------------------------------------------------------------------------------------------------------
def rand_sets(seed, n, frames=1):
    """n random descriptors, split into `frames` frames of nearly equal size"""
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    cuts = [n * f // frames for f in range(frames + 1)]
    return [d[cuts[f]:cuts[f + 1]] for f in range(frames)]


def low_entropy_sets(seed, n, random_bytes, frames=4):
    """only the first `random_bytes` bytes are random, the rest zero: equal descriptors, ties in every rule"""
    rng = np.random.default_rng(seed)
    d = np.zeros((n, 32), np.uint8)
    d[:, :random_bytes] = rng.integers(0, 256, size=(n, random_bytes), dtype=np.uint8)
    cuts = [n * f // frames for f in range(frames + 1)]
    return [d[cuts[f]:cuts[f + 1]] for f in range(frames)]


def clustered_sets(seed, n=4000, centres=40, noise=0.06, frames=8):
    """n descriptors from `centres` planted centres, every bit flipped with probability `noise` -> (sets, the centre of every descriptor)"""
    rng = np.random.default_rng(seed)
    cb = rng.integers(0, 2, size=(centres, 256), dtype=np.uint8)
    label = rng.integers(0, centres, size=n)
    bits = cb[label] ^ (rng.random((n, 256)) < noise).astype(np.uint8)
    d = np.packbits(bits, axis=1)
    cuts = [n * f // frames for f in range(frames + 1)]
    return [d[cuts[f]:cuts[f + 1]] for f in range(frames)], label


def with_empty_frames(sets):
    """an empty frame first, two in the middle and one last"""
    e = np.zeros((0, 32), np.uint8)
    mid = len(sets) // 2
    return [e] + list(sets[:mid]) + [e, e] + list(sets[mid:]) + [e]


def kmajority_states():
    """constructed states for one pass: name -> (desc, node_of, cluster_of, centres n_nodes x k x 32)
      empty:       node 0 has three clusters and no member in cluster 1; node 1 is ordinary
      half_split:  a cluster of four whose members split 2 : 2 in 40 bits (the majority gives 1), and one of two members that differ in every bit
      equidistant: after the update two centres are equal / equally far from members: the lowest centre must win
      wide:        700 members in one node over 5 clusters (a node that crosses chunk boundaries), then small nodes, with an empty cluster in each"""
    rng = np.random.default_rng(77)
    st = {}
    d = rng.integers(0, 256, size=(9, 32), dtype=np.uint8)
    st["empty"] = (d, np.array([0] * 5 + [1] * 4), np.array([0, 0, 2, 2, 0, 0, 1, 1, 0]), rng.integers(0, 256, size=(2, 3, 32), dtype=np.uint8))
    base = rng.integers(0, 2, size=256, dtype=np.uint8)
    four = np.tile(base, (4, 1)); four[:2, :40] ^= 1
    two = np.stack([base, base ^ 1])
    other = rng.integers(0, 2, size=(3, 256), dtype=np.uint8)
    d = np.packbits(np.concatenate([four, two, other]), axis=1)
    st["half_split"] = (d, np.zeros(9, np.int64), np.array([0] * 4 + [1] * 2 + [2] * 3), rng.integers(0, 256, size=(1, 3, 32), dtype=np.uint8))
    # clusters 0 and 1 hold the same rows, so their new centres are equal and every member is equally far from both; cluster 2 holds the complement
    rows = rng.integers(0, 256, size=(3, 32), dtype=np.uint8)
    d = np.concatenate([rows, rows, rows ^ 0xFF])
    st["equidistant"] = (d, np.zeros(9, np.int64), np.array([0] * 3 + [1] * 3 + [2] * 3), rng.integers(0, 256, size=(1, 3, 32), dtype=np.uint8))
    n_small = 40
    d = rng.integers(0, 256, size=(700 + 3 * n_small, 32), dtype=np.uint8)
    d[:700, 4:] = 0                                                          # ties inside the wide node
    node = np.concatenate([np.zeros(700, np.int64), 1 + np.arange(3 * n_small) // 3])
    clus = np.concatenate([rng.choice([0, 1, 3, 4], size=700), rng.choice([0, 2], size=3 * n_small)])
    st["wide"] = (d, node, clus, rng.integers(0, 256, size=(1 + n_small, 5, 32), dtype=np.uint8))
    return st


def kmajority_ref(desc, node_of, cluster_of, centres, ev=None):
    desc = np.asarray(desc, np.uint8); node_of = np.asarray(node_of); cluster_of = np.asarray(cluster_of)
    centres = np.array(centres, np.uint8); out = np.zeros(len(desc), np.int32)
    for v in np.unique(node_of):
        sel = node_of == v
        centres[v], out[sel] = kmajority_pass(desc[sel], cluster_of[sel], centres[v], ev)
    return centres, out
