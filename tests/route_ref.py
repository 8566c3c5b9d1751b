"""A restatement of the route field's contract that shares no code with the library: the explicit list of directed edges, scipy's Dijkstra on it
(costs stay below 2^31, so they are exact in float64), every parent by brute force over the edges that arrive at the cell, the info by counting, the goal's snap by
a minimum over ALL cells and the path by following parents in Python."""
import math
import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import dijkstra

COST_NONE = 0xFFFFFFFF
DEFAULTS = dict(moves=8, near_weight=2, comfort=2.0, cell=1.0)
MOVES = ((-1, 0, 5), (1, 0, 5), (0, -1, 5), (0, 1, 5), (-1, -1, 7), (1, -1, 7), (-1, 1, 7), (1, 1, 7))


def comfort2_of(comfort, cell):
    q2 = (comfort / cell) ** 2 if cell else math.inf
    return 1 << 31 if not q2 < 2147483648.0 else int(math.floor(q2))


def params_of(kw):
    P = dict(DEFAULTS)
    bad = set(kw) - set(P)
    assert not bad, bad
    P.update(kw)
    return P


def source_index(source, nx):
    if source is None:
        return -1
    if isinstance(source, (tuple, list)):
        return int(source[1]) * nx + int(source[0])
    return int(source)


def edges(reach, dist2, P):
    """-> (from, to, cost) of every move that exists, both directions listed"""
    ny, nx = reach.shape
    inn = reach == 2
    c2 = comfort2_of(P["comfort"], P["cell"])
    w = np.where(dist2.astype(np.int64) <= c2, 1 + P["near_weight"], 1).astype(np.int64)
    ys, xs = np.mgrid[0:ny, 0:nx]
    A, B, V = [], [], []
    for dx, dy, step in MOVES[:P["moves"]]:
        bx, by = xs + dx, ys + dy
        ok = (bx >= 0) & (bx < nx) & (by >= 0) & (by < ny) & inn
        bxc, byc = np.clip(bx, 0, nx - 1), np.clip(by, 0, ny - 1)
        ok &= inn[byc, bxc]
        if dx and dy:
            ok &= inn[ys, bxc] & inn[byc, xs]          # both cells that share an edge with the two ends
        a = (ys * nx + xs)[ok]; b = (byc * nx + bxc)[ok]
        A.append(a); B.append(b); V.append(step * (w.ravel()[a] + w.ravel()[b]))
    return np.concatenate(A), np.concatenate(B), np.concatenate(V), w, c2


def run(reach, dist2, source=None, **kw):
    """-> (cost uint32, parent int32, info) as ssm.route_cells_host gives them"""
    P = params_of(kw)
    reach = np.asarray(reach, np.uint8); dist2 = np.asarray(dist2, np.uint32)
    ny, nx = reach.shape
    n = nx * ny
    src = source_index(source, nx)
    a, b, v, w, c2 = edges(reach, dist2, P)
    cost = np.full(n, COST_NONE, np.uint32); parent = np.full(n, -1, np.int32)
    if src >= 0:
        assert reach.ravel()[src] == 2
        d = dijkstra(csr_matrix((v.astype(np.float64), (a, b)), shape=(n, n)), directed=True, indices=src)
        ok = np.isfinite(d)
        assert d[ok].max() < 2 ** 31
        cost[ok] = d[ok].astype(np.uint32)
        # parents: over every edge a -> b whose start is routed, the smallest (cost(a) + edge) << 24 | a
        use = cost[a] != COST_NONE
        key = ((cost[a[use]].astype(np.int64) + v[use]) << 24) | a[use]
        best = np.full(n, np.iinfo(np.int64).max, np.int64)
        np.minimum.at(best, b[use], key)
        has = (best != np.iinfo(np.int64).max)
        has[src] = False
        parent[has] = (best[has] & 0xFFFFFF).astype(np.int32)
        assert np.array_equal(best[has] >> 24, cost[has].astype(np.int64))          # the best way in costs what Dijkstra said
        assert np.array_equal(has | (np.arange(n) == src), cost != COST_NONE)
    inn = reach.ravel() == 2
    routed = cost != COST_NONE
    near = dist2.ravel().astype(np.int64) <= c2
    info = dict(routed=int(routed.sum()), unrouted=int((inn & ~routed).sum()), near_cells=int((routed & near).sum()), max_cost=0, far_cell=-1, source_cell=src, comfort2=c2,
                moves=P["moves"])
    if routed.any():
        info["max_cost"] = int(cost[routed].max())
        info["far_cell"] = int(np.flatnonzero(routed & (cost == info["max_cost"]))[0])
    return cost.reshape(ny, nx), parent.reshape(ny, nx), info


def path(cost, parent, dist2, goal, goal_snap=0, **kw):
    """-> (cells int32 from the source to the snapped goal, path info) as ssm.route_path_host gives them (max_path: unbounded)"""
    P = params_of(kw)
    ny, nx = cost.shape
    c2 = comfort2_of(P["comfort"], P["cell"])
    ys, xs = np.mgrid[0:ny, 0:nx]
    d2 = (xs - goal[0]).astype(np.int64) ** 2 + (ys - goal[1]).astype(np.int64) ** 2
    ok = (cost != COST_NONE) & (d2 <= goal_snap * goal_snap)
    info = dict(len=0, goal_cell=-1, cost=-1, n_axial=0, n_diag=0, near_steps=0, min_d2=-1)
    if not ok.any():
        return np.zeros(0, np.int32), info
    g = int((((d2 << 24) | (ys * nx + xs))[ok]).min() & 0xFFFFFF)
    cells = [g]
    while parent.ravel()[cells[-1]] >= 0:
        cells.append(int(parent.ravel()[cells[-1]]))
        assert len(cells) <= nx * ny
    cells = cells[::-1]
    dd = dist2.ravel()[cells].astype(np.int64)
    diag = sum(1 for p, q in zip(cells, cells[1:]) if p % nx != q % nx and p // nx != q // nx)
    info.update(len=len(cells), goal_cell=g, cost=int(cost.ravel()[g]), n_axial=len(cells) - 1 - diag, n_diag=diag, near_steps=int((dd <= c2).sum()), min_d2=int(dd.min()))
    return np.array(cells, np.int32), info


def check_path(cells, info, reach, dist2, source, **kw):
    """the properties of a path, from the contract alone: it starts at the source, ends at the goal cell, consecutive cells are moves that exist, the edge costs sum
    to the cost, the step counts add up"""
    P = params_of(kw)
    ny, nx = reach.shape
    if info["len"] == 0:
        assert len(cells) == 0 and info["goal_cell"] == -1
        return
    a, b, v, w, c2 = edges(np.asarray(reach, np.uint8), np.asarray(dist2, np.uint32), P)
    table = {(int(p), int(q)): int(c) for p, q, c in zip(a, b, v)}
    assert len(cells) == info["len"] and cells[0] == source_index(source, nx) and cells[-1] == info["goal_cell"], (cells[:3], cells[-3:], info)
    assert all((int(p), int(q)) in table for p, q in zip(cells, cells[1:]))
    assert sum(table[(int(p), int(q))] for p, q in zip(cells, cells[1:])) == info["cost"]
    assert info["n_axial"] + info["n_diag"] == info["len"] - 1
    assert 5 * 2 * info["n_axial"] + 7 * 2 * info["n_diag"] <= info["cost"]
    assert len(set(cells.tolist())) == len(cells)
