"""The case table of the quad-tree selection's tests (K4, ORBextractor::DistributeOctTree), shared by tests/test_octree_cases.py (the two CPU references against
each other, and the paths the table reaches) and tests/test_gpu_orb_octree.py (octree_kernel through ssm_debug_orb_octree against them).

A case is built for ONE LEVEL of a configuration: Case(name, cands, cellmax) with cands (k, 3) int64 rows (xr, yr, score) relative to minBorder, in RANK order
(the order FAST detects in: cells row-major, raster inside a cell), and cellmax (nCols * nRows) the per-cell maxima of S = score + 1 the kernel is handed.
The candidate words (encode), the survivors of the ini / min drop rule (survivors) and the reference selection (reference) all follow from that.

Encoding, as fast_tile's cellx / celly tables and level_candidates of oracle/orb.c have it: with W = w - 2 minB, H = h - 2 minB the valid positions are
3 <= xr < W - 3, 3 <= yr < H - 3; the cell column is (xr - 3) // wCell, the offset inside it xr - col * wCell (3 .. wCell + 2); rows likewise."""
import collections
import math
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import pyref                  # noqa: E402

f32 = np.float32
EDGE = 19
OT_KCAP = 2048                # candidates of a level whose node ids the kernel keeps in LDS; above: global scratch
INI, MIN = 20, 7              # orb_iniThFAST, orb_minThFAST of the default configuration

# width, height, levels, scale, features, max_batch: the contexts of tests/test_gpu_orb_octree.py
CONTEXTS = [(640, 480, 8, 1.2, 1000, 3),       # NODES 256
            (1241, 376, 8, 1.2, 2000, 3),      # NODES 512, 4 roots
            (640, 480, 8, 1.2, 4500, 2),       # NODES 1024
            (176, 120, 1, 1.2, 600, 1),        # tiny frame, one level with N = 600
            (96, 320, 1, 1.2, 300, 1)]         # tall frame: round(W / H) = 0, the nIni guard

Level = collections.namedtuple("Level", "w h minB nCols nRows wCell hCell nfeat nIni cand_cap sel_cap W H cell_off cand_off sel_off")
GEOM_FIELDS = Level._fields[:11]               # what ssm_debug_orb_octree's geometry query lists per level
Case = collections.namedtuple("Case", "name cands cellmax")


def geometry(w, h, nlevels, scale, nfeatures):
    """the levels of a configuration by the formulas of ssm_orb_plan.cpp, + cells_total, cand_total, sel_total and the kernel instance's NODES"""
    sf, inv, feat = pyref.level_params(nfeatures, scale, nlevels)
    levels, cells, cands, sels = [], 0, 0, 0
    for l in range(nlevels):
        lw, lh = pyref.cv_round(float(f32(f32(w) * inv[l]))), pyref.cv_round(float(f32(f32(h) * inv[l])))
        minB = EDGE - 3
        W, H = lw - 2 * minB, lh - 2 * minB
        nCols, nRows = int(f32(W) / f32(30)), int(f32(H) / f32(30))
        wCell, hCell = int(math.ceil(float(f32(f32(W) / f32(nCols))))), int(math.ceil(float(f32(f32(H) / f32(nRows)))))
        nIni = max(int(math.floor(float(f32(W) / f32(H)) + 0.5)), 1)
        cand_cap = ((lw + 1) // 2 + nCols + 1) * ((lh + 1) // 2 + nRows + 1)
        levels.append(Level(lw, lh, minB, nCols, nRows, wCell, hCell, feat[l], nIni, cand_cap, feat[l] + 3, W, H, cells, cands, sels))
        cells += nCols * nRows; cands += cand_cap; sels += feat[l] + 3
    need = max(max(L.nfeat + 3, 4 * L.nIni + 8) for L in levels)
    return dict(levels=levels, cells_total=cells, cand_total=cands, sel_total=sels, nodes=256 if need <= 248 else 512 if need <= 504 else 1024)


def planted_levels(nlevels):
    """the levels every case is planted on: level 0 and a middle one"""
    return sorted({0, nlevels // 2})


# ---------------------------------------------------------------- encoding and the references
def cell_of(L, x, y):
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    return (y - 3) // L.hCell * L.nCols + (x - 3) // L.wCell


def rank_word(L, x, y):
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    cj, ci = (x - 3) // L.wCell, (y - 3) // L.hCell
    return ((ci * L.nCols + cj) << 14 | (y - ci * L.hCell) << 7 | (x - cj * L.wCell)).astype(np.uint32)


def encode(L, cands):
    """(k, 2) uint32: the two cand_t words of every candidate, in the order given"""
    c = np.asarray(cands, np.int64).reshape(-1, 3)
    lo = (c[:, 0] | c[:, 1] << 12 | c[:, 2] << 24).astype(np.uint32)
    return np.stack([lo, rank_word(L, c[:, 0], c[:, 1])], 1)


def in_rank_order(L, cands):
    c = np.asarray(cands, np.int64).reshape(-1, 3)
    assert len({(int(x), int(y)) for x, y, _ in c}) == len(c), "positions must be unique: FAST cannot emit a pixel twice"
    assert ((c[:, 0] >= 3) & (c[:, 0] < L.W - 3) & (c[:, 1] >= 3) & (c[:, 1] < L.H - 3) & (c[:, 2] >= 0) & (c[:, 2] < 255)).all()
    return c[np.argsort(rank_word(L, c[:, 0], c[:, 1]), kind="stable")]


def natural_cellmax(L, cands):
    cm = np.zeros(L.nCols * L.nRows, np.int32)
    if len(cands):
        np.maximum.at(cm, cell_of(L, cands[:, 0], cands[:, 1]), (cands[:, 2] + 1).astype(np.int32))
    return cm


def make(L, name, cands, cellmax=None):
    c = in_rank_order(L, cands)
    assert len(c) <= L.cand_cap
    return Case(name, c, natural_cellmax(L, c) if cellmax is None else np.asarray(cellmax, np.int32))


def survivors(L, case, ini=INI, mn=MIN):
    """the drop rule: a key survives iff S > (cellmax > ini ? ini : min)"""
    c = case.cands
    if not len(c):
        return c
    cm = case.cellmax[cell_of(L, c[:, 0], c[:, 1])]
    return c[(c[:, 2] + 1) > np.where(cm > ini, ini, mn)]


def octree_args(L):
    return L.minB, L.w - EDGE + 3, L.minB, L.h - EDGE + 3, L.nfeat


def reference(L, case, oracle=None, trace=None, ini=INI, mn=MIN):
    """the selected (xr, yr, score) rows in output order: the oracle's literal C list code, or (oracle None) pyref's port of it"""
    s = survivors(L, case, ini, mn)
    if oracle is not None:
        return s[oracle.distribute_octtree(s, *octree_args(L))].reshape(-1, 3)
    return np.array(pyref.distribute_octtree([tuple(int(v) for v in r) for r in s], *octree_args(L), trace=trace), np.int64).reshape(-1, 3)


def sel_words(L, rows):
    """the packed words of the selection in absolute level coordinates, as the describe stage reads them"""
    r = np.asarray(rows, np.int64).reshape(-1, 3)
    return ((r[:, 0] + L.minB) | (r[:, 1] + L.minB) << 12 | r[:, 2] << 24).astype(np.uint32)


def orders(case, seed=0):
    """the three buffer orders every case is planted in: rank order, reversed, a seeded shuffle (index arrays into case.cands)"""
    k = len(case.cands)
    return {"rank": np.arange(k), "reversed": np.arange(k)[::-1].copy(), "shuffled": np.random.default_rng(1000 + seed).permutation(k)}


# ---------------------------------------------------------------- builders: (level geometry, seed) -> Case
def _positions(L, rng, nc):
    nx, ny = L.W - 6, L.H - 6
    idx = rng.choice(nx * ny, size=min(nc, nx * ny, L.cand_cap), replace=False)
    return np.stack([3 + idx % nx, 3 + idx // nx], 1).astype(np.int64)


def random(L, seed, nc, name=None):
    rng = np.random.default_rng(seed)
    p = _positions(L, rng, nc)
    return make(L, name or "random(%d)" % nc, np.column_stack([p, rng.integers(7, 255, len(p))]))


def few_scores(L, seed, nc):
    """three distinct scores only: most nodes hold several keys of the best response"""
    rng = np.random.default_rng(seed)
    p = _positions(L, rng, nc)
    return make(L, "few_scores(%d)" % nc, np.column_stack([p, rng.choice([30, 90, 200], len(p))]))


def lattice(L, seed, step):
    """a regular grid with one score: equal node sizes throughout (the second phase's order is decided by the creation sequence) and a tie in every node"""
    xs, ys = np.arange(3, L.W - 3, step), np.arange(3, L.H - 3, step)
    g = np.stack(np.meshgrid(xs, ys), -1).reshape(-1, 2)
    return make(L, "lattice(%d)" % step, np.column_stack([g, np.full(len(g), 50)])[:L.cand_cap])


def cluster(L, seed):
    """a 10 x 10 block in the first quadrant of the first root: the root's split yields one child, the list does not grow, one key is selected"""
    g = np.stack(np.meshgrid(np.arange(3, 13), np.arange(3, 13)), -1).reshape(-1, 2)
    rng = np.random.default_rng(seed)
    return make(L, "cluster", np.column_stack([g, rng.integers(25, 255, len(g))]))


def _with_pairs(L, p, k):
    """p + a free neighbour (right, else below) of each of its first keys that has one, k in all"""
    have, out = {tuple(q) for q in p}, [list(q) for q in p]
    for q in p:
        if len(out) >= len(p) + k:
            break
        for a in ((q[0] + 1, q[1]), (q[0], q[1] + 1)):
            if a[0] < L.W - 3 and a[1] < L.H - 3 and a not in have:
                have.add(a); out.append(list(a))
                break
    return np.array(out, np.int64)


def sparse(L, seed, nc):
    """fewer keys than N, two of them side by side in the window's corner, where no split line of the first passes falls between them: once every other key
    has a node of its own the pair's node still splits, into ONE child -- "no growth" ends the first phase with fewer nodes than keys.  (Scores from 25: every
    key survives the drop rule)"""
    rng = np.random.default_rng(seed)
    nc = min(nc, L.nfeat - 1)
    p = [q for q in _positions(L, rng, nc).tolist() if q not in ([3, 3], [4, 3])][:nc - 2] + [[3, 3], [4, 3]]
    return make(L, "sparse(%d)" % nc, np.column_stack([np.array(p), rng.integers(25, 255, len(p))]))


def pairs(L, seed, k):
    """N - 2k spread keys and k adjacent pairs: the list comes close enough to N for the mode switch, the second phase separates the spread keys and then
    meets a pass in which every split parent (a pair) yields one child: "no growth" in the second phase, below N"""
    rng = np.random.default_rng(seed)
    p = _with_pairs(L, _positions(L, rng, max(L.nfeat - 2 * k, 1)).tolist(), k)
    return make(L, "pairs(%d)" % k, np.column_stack([p, rng.integers(25, 255, len(p))]))


def exact_n(L, seed, uneven=False):
    """the first phase reaches N exactly: N // 4 nodes of one depth of the first root's tree hold one key in each quadrant, N % 4 more hold a single key, all
    side by side in the tree's order -- before the last pass the list is N // 4 + N % 4 long and list + 3 * expandable == N, which is not above N (no mode
    switch); the pass then yields N nodes.  None where the level's cells get too small for that.  uneven: every other of those nodes holds a fifth key, so that
    the size order of the second phase differs from the list order -- a mode switch taken at list + 3 * expandable == N shows in the output order"""
    rng = np.random.default_rng(seed)
    E, S = L.nfeat // 4, L.nfeat % 4
    e, _ = _root_edges(L)

    def split(c):
        x0, y0, x1, y1 = c
        mx, my = x0 + (x1 - x0 + 1) // 2, y0 + (y1 - y0 + 1) // 2
        return [(x0, y0, mx, my), (mx, y0, x1, my), (x0, my, mx, y1), (mx, my, x1, y1)]

    def spot(c):                                                     # a valid position inside the rectangle, or None
        x0, y0, x1, y1 = max(c[0], 3), max(c[1], 3), min(c[2], L.W - 3), min(c[3], L.H - 3)
        return (int(rng.integers(x0, x1)), int(rng.integers(y0, y1))) if x0 < x1 and y0 < y1 else None

    cells = [(e[0], 0, e[1], L.H)]
    while len(cells) < E + S:
        cells = [q for c in cells for q in split(c)]
    keys, full, extra = [], 0, []
    for c in cells:
        quads = [spot(q) for q in split(c)]
        if None in quads:
            continue
        if full < E:
            keys += quads; full += 1
            if uneven and full % 2:
                more = [q for q in (spot(split(c)[0]) for _ in range(20)) if q != quads[0]]
                extra += more[:1]
        elif len(keys) < 4 * E + S:
            keys.append(quads[0])
    if len(keys) != L.nfeat or uneven and not extra:
        return None
    keys += extra
    return make(L, "exact_n_uneven" if uneven else "exact_n", np.column_stack([np.array(keys), rng.integers(25, 255, len(keys))]))


def _root_edges(L):
    hX = f32(f32(L.W) / f32(L.nIni))
    return [int(f32(hX * f32(i))) for i in range(L.nIni + 1)], hX


def _root_of(L, x):
    _, hX = _root_edges(L)
    return min(int(f32(f32(x) / hX)), L.nIni - 1)


def roots_ends(L, seed):
    """keys only in the first and the last root (nIni >= 2): the roots between them are erased before the first pass"""
    if L.nIni < 2:
        return None
    rng = np.random.default_rng(seed)
    p = [q for q in _positions(L, rng, 4000).tolist() if _root_of(L, q[0]) in (0, L.nIni - 1)][:300]
    return make(L, "roots_ends", np.column_stack([np.array(p), rng.integers(7, 255, len(p))]))


def roots_single(L, seed):
    """one root with exactly one key (it starts as a leaf), the others with several; the key at the largest valid xr, where x / hX reaches the last root's clamp"""
    if L.nIni < 2:
        return None
    rng = np.random.default_rng(seed)
    p = [q for q in _positions(L, rng, 4000).tolist() if _root_of(L, q[0]) != 1][:200]
    e, _ = _root_edges(L)
    p.append([max(e[1] + 1, 3), L.H // 2])
    if [L.W - 4, 3] not in p:
        p.append([L.W - 4, 3])
    return make(L, "roots_single", np.column_stack([np.array(p), rng.integers(7, 255, len(p))]))


def thresholds(L, seed, ini=INI, mn=MIN):
    """cells whose maximum is above ini (they keep S > ini only) beside cells whose maximum is exactly ini or below (they keep S > min), with S = score + 1 at
    min, min + 1, ini and ini + 1 in both kinds"""
    rows = []
    for ci in range(L.nRows):
        for cj in range(L.nCols):
            x0, y0 = 3 + cj * L.wCell, 3 + ci * L.hCell
            S = [mn, mn + 1, ini, ini + 1] if (ci + cj) % 2 == 0 else [mn, mn + 1, ini] if (ci + cj) % 4 == 1 else [mn, mn + 1, ini - 1]
            for k, s in enumerate(S):
                x, y = x0 + 2 * k, y0 + (k % 2) * 2
                if x < L.W - 3 and y < L.H - 3:
                    rows.append([x, y, s - 1])
    return make(L, "thresholds", np.array(rows))


def all_dropped(L, seed, ini=INI, mn=MIN):
    """no key survives: S = min where the cell's maximum is min, and S <= ini under a planted cell maximum above ini"""
    rng = np.random.default_rng(seed)
    p = _positions(L, rng, 300)
    half = cell_of(L, p[:, 0], p[:, 1]) % 2 == 0
    c = make(L, "all_dropped", np.column_stack([p, np.where(half, mn - 1, rng.integers(mn, ini, len(p)))]))
    cm = c.cellmax.copy()
    cm[1::2] = np.where(cm[1::2] > 0, ini + 7, 0)
    return Case(c.name, c.cands, cm)


def extremes(L, seed):
    """the four corners of the valid window, both sides of the first split lines mx, my of every root, and some keys around them"""
    rng = np.random.default_rng(seed)
    e, _ = _root_edges(L)
    p = {(3, 3), (L.W - 4, 3), (3, L.H - 4), (L.W - 4, L.H - 4)}
    my = int(math.ceil(L.H / 2))
    for i in range(L.nIni):
        mx = e[i] + int(math.ceil((e[i + 1] - e[i]) / 2))
        for x in (mx - 1, mx):
            for y in (my - 1, my):
                if 3 <= x < L.W - 3 and 3 <= y < L.H - 3:
                    p.add((x, y))
    p |= {tuple(q) for q in _positions(L, rng, 40).tolist()}
    p = np.array(sorted(p))
    return make(L, "extremes", np.column_stack([p, rng.integers(7, 255, len(p))]))


def empty(L, seed=0):
    return make(L, "empty", np.zeros((0, 3), np.int64))


def table(L, ini=INI, mn=MIN):
    """every case of one level, in a fixed order with committed seeds (chosen on the CPU so that the table reaches every path: tests/test_octree_cases.py)"""
    N = L.nfeat
    t = [random(L, 100 + i, nc) for i, nc in enumerate([1, 2, 3, N - 1, N, N + 1, 4 * N, 2047, 2048, 2049, 5000])]
    t += [random(L, 200 + i, 3 * N + 7 * i, "random(3N+%d)#%d" % (7 * i, i)) for i in range(6)]
    t += [few_scores(L, 300, N + 1), few_scores(L, 301, 4 * N), few_scores(L, 302, 2049)]
    t += [lattice(L, 0, 5), lattice(L, 0, 9), lattice(L, 0, 16)]
    t += [cluster(L, 400), sparse(L, 500, 100), sparse(L, 501, 40), pairs(L, 600, 10), pairs(L, 601, 4), exact_n(L, 650), exact_n(L, 651, True)]
    t += [roots_ends(L, 700), roots_single(L, 701), thresholds(L, 800, ini, mn), all_dropped(L, 801, ini, mn), extremes(L, 900)]
    return [c for c in t if c is not None]
