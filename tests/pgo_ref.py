"""An independent numpy float64 restatement of the pose-graph optimiser's contract: SE3 vertices, edges e = toMQT(Z^-1 Xi^-1 Xj) with
Huber kernels, Levenberg as g2o's OptimizationAlgorithmLevenberg.  It shares nothing with include/ssm/pgo_core.h: matrices are ordinary row-major 4 x 4,
the Jacobians come from quaternion algebra (the product differentiates the rotation-matrix-to-quaternion branch), assembly is dense, the solve is
numpy.linalg.cholesky, sums are numpy's.  Plus the seeded scene generator of the tests."""
import numpy as np

MAX_TRIALS = 10


def quat_to_rot(x, y, z, w):
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def from_mqt(v):
    v = np.asarray(v, np.float64)
    w2 = 1.0 - float(v[3:] @ v[3:])
    w = np.sqrt(w2) if w2 > 0 else 0.0
    T = np.eye(4)
    T[:3, :3] = quat_to_rot(v[3], v[4], v[5], w)
    T[:3, 3] = v[:3]
    return T


def rot_to_quat(R):
    """Eigen's branches -> ((x, y, z, w), branch): 3 = trace > 0, i = the largest diagonal is R[i, i]"""
    q = np.zeros(4)
    t = R[0, 0] + R[1, 1] + R[2, 2]
    if t > 0:
        s = np.sqrt(t + 1.0)
        q[3] = 0.5 * s
        s = 0.5 / s
        q[0], q[1], q[2] = (R[2, 1] - R[1, 2]) * s, (R[0, 2] - R[2, 0]) * s, (R[1, 0] - R[0, 1]) * s
        return q, 3
    i = 0
    if R[1, 1] > R[0, 0]:
        i = 1
    if R[2, 2] > R[i, i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    s = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
    q[i] = 0.5 * s
    s = 0.5 / s
    q[3] = (R[k, j] - R[j, k]) * s
    q[j] = (R[j, i] + R[i, j]) * s
    q[k] = (R[k, i] + R[i, k]) * s
    return q, i


def unit_quat(R):
    q, br = rot_to_quat(R)
    q = q / np.linalg.norm(q)
    return (-q if q[3] < 0 else q), br


def to_mqt(T):
    q, _ = unit_quat(T[:3, :3])
    return np.concatenate([T[:3, 3], q[:3]])


def inv(T):
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


def edge_error(Z, Xi, Xj):
    return to_mqt(inv(Z) @ inv(Xi) @ Xj)


def branch_of(Z, Xi, Xj):
    return rot_to_quat((inv(Z) @ inv(Xi) @ Xj)[:3, :3])[1]


def numeric_jacobians(Z, Xi, Xj, h=1e-6):
    """central differences of e with respect to the updates X <- X fromMQT(d) of Xi and Xj"""
    Ji, Jj = np.zeros((6, 6)), np.zeros((6, 6))
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        Ji[:, k] = (edge_error(Z, Xi @ from_mqt(d), Xj) - edge_error(Z, Xi @ from_mqt(-d), Xj)) / (2 * h)
        Jj[:, k] = (edge_error(Z, Xi, Xj @ from_mqt(d)) - edge_error(Z, Xi, Xj @ from_mqt(-d))) / (2 * h)
    return Ji, Jj


def _skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def _qleft(q):
    """q (x) p = _qleft(q) p, quaternions as (x, y, z, w)"""
    x, y, z, w = q
    return np.array([[w, -z, y, x], [z, w, -x, y], [-y, x, w, z], [-x, -y, -z, w]])


def _qright(q):
    """p (x) q = _qright(q) p"""
    x, y, z, w = q
    return np.array([[w, z, -y, x], [-z, w, x, y], [y, -x, w, z], [-x, -y, -z, w]])


def analytic_jacobians(Z, Xi, Xj):
    """exact, by quaternion algebra: q(E) = q(A) (x) conj(q(di)) (x) q(B) (x) q(dj), A = Z^-1, B = Xi^-1 Xj"""
    A, B = inv(Z), inv(Xi) @ Xj
    E = A @ B
    qa, _ = unit_quat(A[:3, :3])
    qb, _ = unit_quat(B[:3, :3])
    qe = _qleft(qa) @ qb
    qe_ref, _ = unit_quat(E[:3, :3])
    sg = 1.0 if qe @ qe_ref > 0 else -1.0               # the sign toMQT picks (w >= 0)
    Ji, Jj = np.zeros((6, 6)), np.zeros((6, 6))
    Ji[:3, :3] = -A[:3, :3]
    Ji[:3, 3:] = 2 * A[:3, :3] @ _skew(B[:3, 3])
    Jj[:3, :3] = E[:3, :3]
    Ji[3:, 3:] = sg * (-(_qleft(qa) @ _qright(qb))[:3, :3])
    Jj[3:, 3:] = sg * _qleft(qe)[:3, :3]
    return Ji, Jj


def info_matrix(info21):
    if info21 is None:
        return 100.0 * np.eye(6)
    M = np.zeros((6, 6))
    M[np.triu_indices(6)] = info21
    return M + np.triu(M, 1).T


def huber(e2):
    if e2 <= 1.0:
        return e2, 1.0
    s = np.sqrt(e2)
    return 2 * s - 1.0, 1.0 / s


class Graph:
    """poses: n x 4 x 4; fixed: n flags; edges: (from, to) vertex INDICES; Z: m x 4 x 4; omega: m x 6 x 6; robust: m flags"""

    def __init__(self, poses, fixed, edges, Z, omega=None, robust=None):
        self.X = np.array(poses, np.float64)
        self.fixed = np.array(fixed, bool)
        self.edges = np.array(edges, np.int64).reshape(-1, 2)
        self.Z = np.array(Z, np.float64).reshape(-1, 4, 4)
        m = len(self.edges)
        self.omega = np.array(omega, np.float64) if omega is not None else np.tile(100.0 * np.eye(6), (m, 1, 1))
        self.robust = np.array(robust, bool) if robust is not None else np.ones(m, bool)

    def set_mode(self, local):
        n = len(self.X)
        if not local:
            self.fixed[:] = False
            self.fixed[0] = True
            return
        self.fixed[:] = True
        if n >= 6:                                       # the reference's unsigned `i > size() - 6` frees nothing below six vertices
            self.fixed[n - 5:] = False

    def active(self):
        free = ~self.fixed
        act = [k for k, (i, j) in enumerate(self.edges) if free[i] or free[j]]
        touched = set()
        for k in act:
            touched.update(self.edges[k])
        verts = [v for v in range(len(self.X)) if free[v] and v in touched]
        return act, verts

    def plain_chi2(self, k):
        i, j = self.edges[k]
        e = edge_error(self.Z[k], self.X[i], self.X[j])
        return float(e @ self.omega[k] @ e)

    def chi2(self, act):
        tot = 0.0
        for k in act:
            c = self.plain_chi2(k)
            tot += huber(c)[0] if self.robust[k] else c
        return tot

    def system(self, act, verts):
        slot = {v: r for r, v in enumerate(verts)}
        N = 6 * len(verts)
        H, b = np.zeros((N, N)), np.zeros(N)
        for k in act:
            i, j = self.edges[k]
            e = edge_error(self.Z[k], self.X[i], self.X[j])
            Ji, Jj = analytic_jacobians(self.Z[k], self.X[i], self.X[j])
            w = huber(float(e @ self.omega[k] @ e))[1] if self.robust[k] else 1.0
            W = w * self.omega[k]
            for (va, Ja) in ((i, Ji), (j, Jj)):
                if va not in slot:
                    continue
                a = 6 * slot[va]
                b[a:a + 6] -= Ja.T @ W @ e
                for (vb, Jb) in ((i, Ji), (j, Jj)):
                    if vb in slot:
                        c = 6 * slot[vb]
                        H[a:a + 6, c:c + 6] += Ja.T @ W @ Jb
        return H, b

    def optimize(self, iterations, reverse=False):
        """-> dict(iterations, trials, accepted (bit masks), gains (per iteration: the trials' gains), chi2_before, chi2_after, lam).  reverse: the unknowns in
        reversed vertex order (another elimination order: the measure of what ordering alone does to the result)"""
        act, verts = self.active()
        out = dict(iterations=0, trials=[], accepted=[], gains=[], chi2_before=[], chi2_after=[], lam=0.0, active_vertices=len(verts), active_edges=len(act))
        if not act or not verts:
            return out
        if reverse:
            verts = verts[::-1]
        lam, nu = 0.0, 2.0
        for it in range(iterations):
            chi = self.chi2(act)
            H, b = self.system(act, verts)
            if it == 0:
                lam, nu = 1e-5 * float(np.max(np.abs(np.diag(H)))), 2.0
            out["chi2_before"].append(chi)
            trials, bits, gains, gain = 0, 0, [], 0.0
            while True:
                saved = self.X.copy()
                try:
                    Lc = np.linalg.cholesky(H + lam * np.eye(len(b)))
                    x = np.linalg.solve(Lc.T, np.linalg.solve(Lc, b))
                    ok = True
                except np.linalg.LinAlgError:
                    x, ok = np.zeros(len(b)), False
                if ok:
                    for r, v in enumerate(verts):
                        self.X[v] = self.X[v] @ from_mqt(x[6 * r:6 * r + 6])
                chi_new = self.chi2(act) if ok else np.finfo(np.float64).max
                gain = (chi - chi_new) / (float(x @ (lam * x + b)) + 1e-3)
                gains.append(gain)
                if gain > 0 and np.isfinite(chi_new):
                    t = 2 * gain - 1
                    lam *= max(1.0 / 3.0, min(1.0 - t * t * t, 2.0 / 3.0))
                    nu = 2.0
                    chi = chi_new
                    bits |= 1 << trials
                    accepted = True
                else:
                    lam *= nu
                    nu *= 2
                    self.X = saved
                    accepted = False
                trials += 1
                if not accepted and not np.isfinite(lam):
                    break
                if not (gain < 0 and trials < MAX_TRIALS):
                    break
            out["trials"].append(trials)
            out["accepted"].append(bits)
            out["gains"].append(gains)
            out["chi2_after"].append(chi)
            out["iterations"] = it + 1
            out["lam"] = lam
            if trials == MAX_TRIALS or gain == 0:
                break
        return out


# ---------------------------------------------------------------- scenes
def _small(rng, t_sigma, r_sigma):
    v = np.concatenate([rng.normal(0, t_sigma, 3), rng.normal(0, r_sigma, 3) * 0.5])
    return from_mqt(v)


def make_scene(seed, n, drift, noise_t, noise_r, nearby=2, loops=(), radius=10.0):
    """n key-frames once around a circle of `radius` m (the last one is back near the first).  Estimates: the odometry chain with a systematic drift of `drift`
    (rad of yaw per step, and as much in metres) plus noise.  Edges, in the order tryInsertKeyFrame / mainLoop add them: for vertex k the edge (k - 1 -> k)
    "from state" (its measurement IS the estimate's relative pose: zero error at the start), then `nearby` edges (k - 1 - m -> k), m = 1 .. nearby, measured
    from the truth with noise (noise_t m, noise_r rad); then the loop edges (i, j, sigma_t, sigma_r), measured from the truth with their own noise.
    -> dict(poses, edges, Z)"""
    rng = np.random.default_rng(seed)
    G = []
    for k in range(n):
        a = 2 * np.pi * k / n
        T = np.eye(4)
        T[:3, :3] = quat_to_rot(0.0, 0.0, np.sin((a + np.pi / 2) / 2), np.cos((a + np.pi / 2) / 2))
        T[:3, 3] = [radius * np.cos(a), radius * np.sin(a), 0.1 * np.sin(3 * a)]
        G.append(T)
    X = [G[0].copy()]
    D = from_mqt([drift * 0.5, drift * 0.25, 0.0, 0.0, 0.0, np.sin(drift / 2)])
    for k in range(1, n):
        X.append(X[-1] @ inv(G[k - 1]) @ G[k] @ D @ _small(rng, noise_t * 0.2, noise_r * 0.2))
    edges, Z = [], []
    for k in range(1, n):
        edges.append((k - 1, k))
        Z.append(inv(X[k - 1]) @ X[k])
        for m in range(1, nearby + 1):
            if k - 1 - m < 0:
                break
            edges.append((k - 1 - m, k))
            Z.append(inv(G[k - 1 - m]) @ G[k] @ _small(rng, noise_t, noise_r))
    for (i, j, st, sr) in loops:
        edges.append((i, j))
        Z.append(inv(G[i]) @ G[j] @ _small(rng, st, sr))
    return dict(poses=np.array(X), edges=np.array(edges, np.int64), Z=np.array(Z))


SCENES = {
    "mild": dict(seed=11, n=40, drift=0.02, noise_t=0.05, noise_r=0.01, nearby=2, loops=((39, 0, 0.05, 0.01),)),
    "huber": dict(seed=12, n=24, drift=0.3, noise_t=0.05, noise_r=0.01, nearby=2, loops=((23, 0, 0.05, 0.01),)),
    "reject": dict(seed=13, n=16, drift=0.5, noise_t=0.05, noise_r=0.01, nearby=2, loops=((15, 0, 2.0, 0.4),)),
}


def scene_graph(scene, local=False):
    g = Graph(scene["poses"], np.zeros(len(scene["poses"]), bool), scene["edges"], scene["Z"])
    g.set_mode(local)
    return g
