"""Writes tests/golden/looper.npz from tests/looper_ref.py (the independent restatement of the Looper contract): the (k, L) = (10, 3) vocabulary arrays,
8 descriptor sets (sets 4 .. 7 share half of their descriptors with sets 0 .. 3), their bag-of-words vectors (padded to the longest; `vec_len` says how
much of each row counts), the word of every feature and the 8 x 8 score matrix score(row = query, column = stored).  Arrays only.
Run from the repository root: python tests/golden/make_looper_golden.py"""
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import looper_ref as R  # noqa: E402


def main():
    k, L, parent, is_leaf, desc, weight = R.make_vocab(10, 3, 0x100B)
    rv = R.RefVocab(k, L, parent, is_leaf, desc, weight)
    rng = np.random.default_rng(0x100C)
    n = 200
    sets = [R.rand_desc(rng, n) for _ in range(4)]
    for i in range(4):
        d = R.rand_desc(rng, n)
        keep = rng.permutation(n)[:n // 2]
        d[keep] = sets[i][keep]
        sets.append(d)
    tr = [rv.transform(d) for d in sets]
    m = max(len(t[1]) for t in tr)
    vec_ids = np.full((8, m), -1, np.int32); vec_vals = np.zeros((8, m), np.float64); vec_len = np.zeros(8, np.int32)
    for i, (_, ids, vals) in enumerate(tr):
        vec_ids[i, :len(ids)] = ids; vec_vals[i, :len(ids)] = vals; vec_len[i] = len(ids)
    scores = np.array([[R.score(tr[q][1], tr[q][2], tr[e][1], tr[e][2]) for e in range(8)] for q in range(8)])
    np.savez_compressed(os.path.join(HERE, "looper.npz"), k=np.int32(k), L=np.int32(L), parent=parent, is_leaf=is_leaf, desc=desc, weight=weight,
                        sets=np.stack(sets), words=np.stack([t[0] for t in tr]), vec_ids=vec_ids, vec_vals=vec_vals, vec_len=vec_len, scores=scores)
    print(os.path.getsize(os.path.join(HERE, "looper.npz")), "bytes")


if __name__ == "__main__":
    main()
