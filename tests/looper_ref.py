"""Independent restatement of the Looper contract: DBoW2 TemplatedVocabulary<FORB> with L1_NORM scoring and TF_IDF weights, as
rgbd_tutor::Looper uses it (reference include/looper.h, src/looper.cpp).  numpy for the bit counts, everything else plain Python; every sum is SEQUENTIAL
in ascending word id, in float64, like DBoW2's -- the library sums in a lane order of its own (include/ssm/looper_core.h), so values agree to rounding and
ids agree exactly.  Also the seeded vocabulary / descriptor generators the looper tests, the golden file and scripts/looper_bench.py share."""
from fractions import Fraction
import numpy as np

_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


class RefVocab:
    """parent[i], is_leaf[i], desc[i], weight[i] describe node id i + 1 (id 0 = the root), in file order"""

    def __init__(self, k, L, parent, is_leaf, desc, weight):
        self.k, self.L = int(k), int(L)
        self.parent = np.asarray(parent, np.int64); self.is_leaf = np.asarray(is_leaf, np.uint8)
        self.desc = np.asarray(desc, np.uint8).reshape(-1, 32); self.weight = np.asarray(weight, np.float64)
        n = len(self.parent)
        order = np.argsort(self.parent, kind="stable")                     # children of an id: consecutive here, in file order
        self.kids = order + 1
        self.cnt = np.bincount(self.parent, minlength=n + 1).astype(np.int64)
        self.start = np.concatenate([[0], np.cumsum(self.cnt)[:-1]])
        self.word_of_id = np.full(n + 1, -1, np.int64)
        leaves = np.nonzero(self.is_leaf > 0)[0]
        self.word_of_id[leaves + 1] = np.arange(len(leaves))
        self.word_weight = self.weight[leaves]
        self.nodes, self.words = n + 1, len(leaves)

    def words_of(self, desc):
        """word id of every descriptor: first child, replaced by a later one only when strictly closer"""
        desc = np.asarray(desc, np.uint8).reshape(-1, 32)
        cur = np.zeros(len(desc), np.int64)
        while True:
            live = np.nonzero(self.cnt[cur] > 0)[0]
            if len(live) == 0:
                break
            c = cur[live]
            best = self.kids[self.start[c]]
            bd = _POP[self.desc[best - 1] ^ desc[live]].sum(1)
            for j in range(1, int(self.cnt[c].max())):
                has = np.nonzero(self.cnt[c] > j)[0]
                cand = self.kids[self.start[c[has]] + j]
                d = _POP[self.desc[cand - 1] ^ desc[live[has]]].sum(1)
                better = d < bd[has]
                best[has[better]] = cand[better]; bd[has[better]] = d[better]
            cur[live] = best
        return self.word_of_id[cur]

    def transform(self, desc):
        """-> (word of every feature, ids ascending, values)"""
        wof = self.words_of(desc)
        vec = {}
        for w in wof:                                                      # feature order, one addition per feature
            wt = float(self.word_weight[w])
            if wt > 0:
                vec[int(w)] = vec.get(int(w), 0.0) + wt
        ids = sorted(vec)
        vals = [vec[i] for i in ids]
        norm = 0.0
        for v in vals:
            norm += abs(v)
        if norm > 0:
            vals = [v / norm for v in vals]
        return wof.astype(np.int32), np.array(ids, np.int32), np.array(vals, np.float64)


def score(ids1, v1, ids2, v2):
    if len(ids1) == 0 or len(ids2) == 0:
        return 0.0
    _, a, b = np.intersect1d(ids1, ids2, assume_unique=True, return_indices=True)
    s = 0.0
    for x, y in zip(np.asarray(v1, np.float64)[a].tolist(), np.asarray(v2, np.float64)[b].tolist()):
        s += abs(x - y) - abs(x) - abs(y)
    return -0.5 * s


def score_exact(ids1, v1, ids2, v2):
    """the same sum over the float64 inputs in rationals, rounded once at the end: a reference with no summation order of its own"""
    if len(ids1) == 0 or len(ids2) == 0:
        return 0.0
    _, a, b = np.intersect1d(ids1, ids2, assume_unique=True, return_indices=True)
    s = Fraction(0)
    for x, y in zip(np.asarray(v1, np.float64)[a].tolist(), np.asarray(v2, np.float64)[b].tolist()):
        x, y = Fraction(x), Fraction(y)
        s += abs(x - y) - abs(x) - abs(y)
    return float(Fraction(-1, 2) * s)


def score_matrix(vectors, words):
    """score(vectors[q], vectors[e]) for every (q, e), the same bits as score(): cumsum adds one term after the other in ascending word id, and the 0.0 of a
    word that is not common changes nothing"""
    D = np.zeros((len(vectors), words))
    for f, (ids, vals) in enumerate(vectors):
        D[f, ids] = vals
    S = np.zeros((len(vectors), len(vectors)))
    if words == 0:
        return S
    for q in range(len(vectors)):
        a = D[q]
        t = np.where((D != 0) & (a != 0), (np.abs(a - D) - np.abs(a)) - np.abs(D), 0.0)
        S[q] = -0.5 * np.cumsum(t, axis=1)[:, -1]
    return S + 0.0                                                          # -0.5 * 0.0 is -0.0; score() returns +0.0 for empty vectors


def candidates(vectors, frame_ids, min_sim_score, min_interval, scores=None):
    """Looper::getPossibleLoops for every entry q right after its own add: entries 0 .. q in database order -> [(q, e, score)]"""
    out = []
    for q in range(len(vectors)):
        for e in range(q + 1):
            s = scores[q][e] if scores is not None else score(*vectors[q], *vectors[e])
            if s > min_sim_score and abs(int(frame_ids[e]) - int(frame_ids[q])) > min_interval:
                out.append((q, e, s))
    return out


def candidates_range(vectors, frame_ids, first, n, against, min_sim_score, min_interval, scores=None):
    """candidates() with the library's query arguments: the query entries first .. first + n - 1, each against the entries 0 .. against - 1 (against < 0: 0 .. q)
    -> [(q, e, score)] by (q, e)"""
    out = []
    for q in range(first, first + n):
        for e in range(q + 1 if against < 0 else against):
            s = scores[q][e] if scores is not None else score(*vectors[q], *vectors[e])
            if s > min_sim_score and abs(int(frame_ids[e]) - int(frame_ids[q])) > min_interval:
                out.append((q, e, float(s)))
    return out


# ---- generators -----------------------------------------------------------------------------------------------------------------------------------------
def make_vocab(k, L, seed, dbow_order=True):
    """a full k-ary tree of depth L with seeded random descriptors and weights.  dbow_order: ids in the order DBoW2's HKmeans creates them (the k children of
    a node together, then each child's subtree); else level by level"""
    rng = np.random.default_rng(seed)
    n = sum(k ** l for l in range(1, L + 1))
    if dbow_order:
        parent = np.zeros(n, np.int32); level = np.zeros(n, np.int32)
        nxt, stack = 0, [(0, 0)]
        while stack:
            pid, lv = stack.pop()
            ids = list(range(nxt + 1, nxt + 1 + k)); nxt += k
            for i in ids:
                parent[i - 1] = pid; level[i - 1] = lv + 1
            if lv + 1 < L:
                stack.extend((i, lv + 1) for i in reversed(ids))
        is_leaf = (level == L).astype(np.uint8)
    else:
        parent = np.zeros(n, np.int32); is_leaf = np.zeros(n, np.uint8)
        first, prev_first, prev_n = 1, 0, 1                                 # ids of the level being filled / of its parents
        for l in range(1, L + 1):
            m = prev_n * k
            parent[first - 1:first - 1 + m] = np.repeat(np.arange(prev_first, prev_first + prev_n, dtype=np.int32), k)
            if l == L:
                is_leaf[first - 1:first - 1 + m] = 1
            prev_first, prev_n, first = first, m, first + m
    desc = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    weight = np.where(is_leaf > 0, rng.uniform(0.5, 12.0, n), 0.0)
    return k, L, parent, is_leaf, desc, weight


def make_irregular_vocab(seed, k=6, L=4):
    """short sibling groups, leaves above level L, some zero weights, a few duplicated sibling descriptors (ties)"""
    rng = np.random.default_rng(seed)
    parent, leaf, level = [], [], []
    stack = [(0, 0)]
    while stack:
        pid, lv = stack.pop(0) if rng.random() < 0.5 else stack.pop()
        nc = int(rng.integers(1, k + 1))
        for _ in range(nc):
            parent.append(pid); level.append(lv + 1)
            is_l = lv + 1 == L or (lv + 1 >= 2 and rng.random() < 0.3)
            leaf.append(1 if is_l else 0)
            if not is_l:
                stack.append((len(parent), lv + 1))
    n = len(parent)
    parent = np.array(parent, np.int32); leaf = np.array(leaf, np.uint8)
    desc = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    for i in range(1, n):                                                   # equal siblings: the earlier one must win
        if parent[i] == parent[i - 1] and rng.random() < 0.15:
            desc[i] = desc[i - 1]
    weight = np.where(leaf > 0, rng.uniform(0.5, 12.0, n), 0.0)
    weight[(leaf > 0) & (rng.random(n) < 0.2)] = 0.0
    return k, L, parent, leaf, desc, weight


WIDE_ROOT_PAIRS = ((40, 41), (50, 66), (70, 85), (100, 260), (30, 299))    # children of the root (all leaves): adjacent lanes of a 16-lane group, 16 apart (same
#                                                                             lane, next trip), 15 apart, 160 apart, and a later copy in a lower lane (299 % 16 < 30 % 16)
WIDE_GROUP_PAIRS = ((4, 5), (1, 17), (3, 18), (9, 16))                      # the same inside a 19- and a 20-child group (160 apart does not fit)
WIDE_GROUPS = (2, 3)


def make_wide_vocab(seed):
    """header k = 20, L = 2, but the root has 300 children: the first 20 are inner nodes with 17 .. 20 leaf children, the other 280 are leaves (the loader caps
    the header's k, not the children of a node).  Duplicate descriptors sit in the child pairs above: the EARLIER child must win.  A planted descriptor
    inside group g is g's own descriptor with 10 bits flipped, so that a query equal to it goes to g at the root (random descriptors are about 128 bits away).
    -> (the vocabulary's arrays, queries equal to every planted descriptor, the word id each of them must get)"""
    rng = np.random.default_rng(seed)
    parent = [0] * 300
    leaf = [0] * 20 + [1] * 280
    gstart = []
    for c in range(20):
        gstart.append(len(parent))
        parent += [c + 1] * (17 + c % 4); leaf += [1] * (17 + c % 4)
    n = len(parent)
    parent = np.array(parent, np.int32); leaf = np.array(leaf, np.uint8)
    desc = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    planted = []                                                            # (index of the earlier copy, of the later one)
    for a, b in WIDE_ROOT_PAIRS:
        desc[b] = desc[a]; planted.append((a, b))
    for g in WIDE_GROUPS:
        for a, b in WIDE_GROUP_PAIRS:
            d = np.unpackbits(desc[g]); d[rng.permutation(256)[:10]] ^= 1
            desc[gstart[g] + a] = desc[gstart[g] + b] = np.packbits(d); planted.append((gstart[g] + a, gstart[g] + b))
    weight = np.where(leaf > 0, rng.uniform(0.5, 12.0, n), 0.0)
    word_of_index = np.cumsum(leaf) - 1                                     # leaves in file order
    queries = np.stack([desc[a] for a, _ in planted])
    return (20, 2, parent, leaf, desc, weight), queries, word_of_index[[a for a, _ in planted]].astype(np.int32)


def make_tiny_vocab(seed, zero=()):
    """k = 3, L = 1: three words; those in `zero` have weight 0"""
    rng = np.random.default_rng(seed)
    desc = rng.integers(0, 256, size=(3, 32), dtype=np.uint8)
    weight = rng.uniform(0.5, 12.0, 3)
    weight[list(zero)] = 0.0
    return 3, 1, np.zeros(3, np.int32), np.ones(3, np.uint8), desc, weight


def write_vocab_text(path, k, L, parent, is_leaf, desc, weight, scoring=0, weighting=0, trailing_blank=False):
    with open(path, "w") as f:
        f.write(f"{k} {L} {scoring} {weighting}\n")
        for p, l, d, w in zip(parent.tolist(), is_leaf.tolist(), np.asarray(desc).tolist(), weight.tolist()):
            f.write(f"{p} {l} " + " ".join(map(str, d)) + f" {w!r}\n")
        if trailing_blank:
            f.write("\n")


def rand_desc(rng, n):
    return rng.integers(0, 256, size=(n, 32), dtype=np.uint8)


def loop_set(seed, frames=160, n=1000, first_revisit=100, every=4, back=90):
    """descriptor sets of a sequence with planted revisits: every `every`-th frame from `first_revisit` on keeps a random half of frame f - back's descriptors"""
    rng = np.random.default_rng(seed)
    sets, planted = [], []
    for f in range(frames):
        d = rand_desc(rng, n)
        if f >= first_revisit and (f - first_revisit) % every == 0:
            keep = rng.permutation(n)[:n // 2]
            d[keep] = sets[f - back][keep]
            planted.append((f, f - back))
        sets.append(d)
    return sets, planted
