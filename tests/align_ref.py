"""Dense alignment restated from DESIGN.md s.18 in numpy float64 and Python integers.  Written from the section, not from include/ssm/align_core.h: the normal
map and one iteration's terms as vectorised float64 passes in the section's operation order (numpy never contracts a multiply and an add), the sums as Python
integers, and the 6 x 6 solve, the exponential and the pose algebra in plain Python floats -- sin / cos by the section's polynomial (Cody-Waite reduction and the
fdlibm kernels, the contract of the PnP solve), so that the pose too can be compared byte for byte.  `accumulate` also hands out why each point was or was not
used, so that tests/test_align.py can assert that the case list still hits what it was written for."""
import math
import numpy as np
import carve_ref as CR

POINT_DTYPE = CR.POINT_DTYPE
EYE = CR.EYE
DEFAULTS = dict(max_iterations=10, stride=1, z_min=0.1, z_max=80.0, dist_max=0.25, delta=0.05, damping=1.0e-6, eps_rot=1.0e-4, eps_trans=1.0e-4, min_inliers=1000,
                max_shift=1.0, max_angle=0.2, tol_abs=0.05, tol_rel_ppm=20000)
MAX_ITER, CONVERGED, TOO_FEW, DEGENERATE, DIVERGED = range(5)
S_HB, S_CHI = 20, 30
NSUM, I_B, I_CHI, I_TESTED, I_INLIER = 30, 21, 27, 28, 29
INFO_FIELDS = ("status", "iterations", "n_in", "tested_first", "inliers_first", "tested_last", "inliers_last", "chi2_first", "chi2_last")
WHY = ("not_finite", "z_range", "outside", "invalid", "far", "tail", "quadratic")


def normal_map(depth, camera, tol_abs=0.05, tol_rel_ppm=20000):
    """-> (valid h x w uint8, normals h x w x 4 float32: the double normal rounded once, an invalid pixel all zero)"""
    cx, cy, fx, fy, scale = (float(v) for v in camera)
    d = np.asarray(depth, np.uint16).astype(np.int64)
    h, w = d.shape
    valid = np.zeros((h, w), bool)
    normals = np.zeros((h, w, 4), np.float32)
    if h < 3 or w < 3:
        return valid.astype(np.uint8), normals
    tol_units = round(float(tol_abs) * scale)          # half-even, as llrint
    c = d[1:-1, 1:-1]
    nb = dict(l=d[1:-1, :-2], r=d[1:-1, 2:], u=d[:-2, 1:-1], dn=d[2:, 1:-1])
    tol = tol_units + (c * int(tol_rel_ppm)) // 1000000
    ok = c > 0
    for n in nb.values():
        ok &= (n > 0) & (np.abs(n - c) <= tol)
    ys, xs = np.mgrid[1:h - 1, 1:w - 1]

    def vertex(x, y, dd):
        z = dd.astype(np.float64) / scale
        return ((x.astype(np.float64) - cx) * z) / fx, ((y.astype(np.float64) - cy) * z) / fy, z

    with np.errstate(all="ignore"):
        Vl, Vr, Vu, Vd, V = vertex(xs - 1, ys, nb["l"]), vertex(xs + 1, ys, nb["r"]), vertex(xs, ys - 1, nb["u"]), vertex(xs, ys + 1, nb["dn"]), vertex(xs, ys, c)
        a = [Vr[i] - Vl[i] for i in range(3)]
        b = [Vd[i] - Vu[i] for i in range(3)]
        c0 = a[1] * b[2] - a[2] * b[1]
        c1 = a[2] * b[0] - a[0] * b[2]
        c2 = a[0] * b[1] - a[1] * b[0]
        len2 = (c0 * c0 + c1 * c1) + c2 * c2
        ok &= np.isfinite(len2) & (len2 > 0.0)
        ln = np.sqrt(len2)
        n0, n1, n2 = c0 / ln, c1 / ln, c2 / ln
        dot = (n0 * V[0] + n1 * V[1]) + n2 * V[2]
        ok &= np.isfinite(dot) & (dot != 0.0)
        flip = dot > 0.0
        f = [np.where(flip, -n, n).astype(np.float32) for n in (n0, n1, n2)]
    ok &= ~((f[0] == 0) & (f[1] == 0) & (f[2] == 0))
    valid[1:-1, 1:-1] = ok
    for i in range(3):
        normals[1:-1, 1:-1, i] = np.where(ok, f[i], np.float32(0))
    return valid.astype(np.uint8), normals


def accumulate(depth, camera, normals, clouds, Ms, E, P, why=False):
    """one iteration -> the NSUM sums as Python integers (with why: also, per cloud, an array naming what became of each used point: an index into WHY)"""
    cx, cy, fx, fy, scale = (float(v) for v in camera)
    depth = np.asarray(depth, np.uint16)
    h, w = depth.shape
    sums = [0] * NSUM
    whys = []
    E = [[float(v) for v in row] for row in E]
    for pts, M in zip(clouds, Ms):
        pts = pts[::int(P["stride"])]
        x, y, z = (pts[f].astype(np.float64) for f in "xyz")
        reason = np.full(len(pts), -1)
        with np.errstate(all="ignore"):
            a = [M[i][0] * x + M[i][1] * y + M[i][2] * z + M[i][3] for i in range(3)]
            q = [E[i][0] * a[0] + E[i][1] * a[1] + E[i][2] * a[2] + E[i][3] for i in range(3)]
            fin = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & np.isfinite(q[0]) & np.isfinite(q[1]) & np.isfinite(q[2])
            reason[~fin] = 0
            inz = ~(q[2] < float(P["z_min"])) & ~(q[2] > float(P["z_max"]))
            reason[fin & ~inz] = 1
            ok = fin & inz
            u = fx * (q[0] / q[2]) + cx
            v = fy * (q[1] / q[2]) + cy
            px = np.floor(u + 0.5)
            py = np.floor(v + 0.5)
            inside = (px >= 0) & (px <= w - 1) & (py >= 0) & (py <= h - 1)          # (false for NaN)
        reason[ok & ~inside] = 2
        ok &= inside
        idx = np.nonzero(ok)[0]
        ix, iy = px[idx].astype(np.int64), py[idx].astype(np.int64)
        nf = normals[iy, ix, :3]
        val = ~((nf[:, 0] == 0) & (nf[:, 1] == 0) & (nf[:, 2] == 0))
        reason[idx[~val]] = 3
        idx, ix, iy, nf = idx[val], ix[val], iy[val], nf[val]
        sums[I_TESTED] += len(idx)
        d = depth[iy, ix].astype(np.float64)
        vz = d / scale
        V = [((ix.astype(np.float64) - cx) * vz) / fx, ((iy.astype(np.float64) - cy) * vz) / fy, vz]
        n = [nf[:, i].astype(np.float64) for i in range(3)]
        qq = [q[i][idx] for i in range(3)]
        with np.errstate(all="ignore"):
            r = (n[0] * (qq[0] - V[0]) + n[1] * (qq[1] - V[1])) + n[2] * (qq[2] - V[2])
            near = np.abs(r) <= float(P["dist_max"])
        reason[idx[~near]] = 4
        idx, r = idx[near], r[near]
        n = [c[near] for c in n]
        qq = [c[near] for c in qq]
        e2 = r * r
        delta = float(P["delta"])
        d2 = delta * delta
        quad = e2 <= d2
        s = np.sqrt(e2)
        with np.errstate(all="ignore"):
            rho0 = np.where(quad, e2, 2 * s * delta - d2)
            wt = np.where(quad, 1.0, delta / s)
        reason[idx] = np.where(quad, 6, 5)
        J = [qq[1] * n[2] - qq[2] * n[1], qq[2] * n[0] - qq[0] * n[2], qq[0] * n[1] - qq[1] * n[0], n[0], n[1], n[2]]
        wr = -(wt * r)
        units = lambda t, S: sum(np.rint(t * float(1 << S)).astype(np.int64).tolist())          # noqa: E731  (rint: half-even, as llrint; the sum is a Python integer)
        sums[I_INLIER] += len(idx)
        sums[I_CHI] += units(rho0, S_CHI)
        k = 0
        for i in range(6):
            wj = wt * J[i]
            sums[I_B + i] += units(wr * J[i], S_HB)
            for j in range(i + 1):
                sums[k] += units(wj * J[j], S_HB)
                k += 1
        whys.append(reason)
    return (sums, whys) if why else sums


# ---- the host side of the section: plain Python floats
def sincos64(x):
    fn = float(round(x * 6.36619772367581382433e-01))          # half-even, as rint
    r = x - fn * 1.57079632673412561417e+00
    r = r - fn * 6.07710050650619224932e-11
    r = r - fn * 2.02226624879595063154e-21
    z = r * r
    ps = 8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 + z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)))
    sr = r + (r * z) * (-1.66666666666666324348e-01 + z * ps)
    pc = 4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * (2.48015872894767294178e-05 + z * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11))))
    cr = (1.0 - 0.5 * z) + (z * z) * pc
    return [(sr, cr), (cr, -sr), (-sr, -cr), (-cr, sr)][int(fn) & 3]


def mat3_mul(A, B):
    return [[A[r][0] * B[0][c] + A[r][1] * B[1][c] + A[r][2] * B[2][c] for c in range(3)] for r in range(3)]


def pose_oplus(R, t, d):
    """(R, t) <- exp(d) (R, t), d = (omega, upsilon): Rodrigues; below 1e-5 rad R = I + W + W W"""
    th = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    W = [[0.0, -d[2], d[1]], [d[2], 0.0, -d[0]], [-d[1], d[0], 0.0]]
    W2 = mat3_mul(W, W)
    eye = lambda r, c: 1.0 if r == c else 0.0          # noqa: E731
    if th < 0.00001:
        dR = [[eye(r, c) + W[r][c] + W2[r][c] for c in range(3)] for r in range(3)]
        V = [row[:] for row in dR]
    else:
        sn, cs = sincos64(th)
        a, b, c3 = sn / th, (1 - cs) / (th * th), (th - sn) / (th * th * th)
        dR = [[eye(r, c) + a * W[r][c] + b * W2[r][c] for c in range(3)] for r in range(3)]
        V = [[eye(r, c) + b * W[r][c] + c3 * W2[r][c] for c in range(3)] for r in range(3)]
    nR = mat3_mul(dR, R)
    nt = []
    for r in range(3):
        vt = V[r][0] * d[3] + V[r][1] * d[4] + V[r][2] * d[5]
        nt.append(dR[r][0] * t[0] + dR[r][1] * t[1] + dR[r][2] * t[2] + vt)
    return nR, nt


def solve_ldlt(Hl, lam, b):
    """(H + lam I) x = b, H by its lower triangle row by row, un-pivoted L D L^T; None on a pivot that is not > 0"""
    A = [[0.0] * 6 for _ in range(6)]
    q = 0
    for a in range(6):
        for c in range(a + 1):
            A[a][c] = A[c][a] = Hl[q]
            q += 1
    for i in range(6):
        A[i][i] += lam
    L = [[0.0] * 6 for _ in range(6)]
    D = [0.0] * 6
    for j in range(6):
        d = A[j][j]
        for k in range(j):
            d -= L[j][k] * L[j][k] * D[k]
        if not d > 0:
            return None
        D[j] = d
        L[j][j] = 1.0
        for i in range(j + 1, 6):
            s = A[i][j]
            for k in range(j):
                s -= L[i][k] * L[j][k] * D[k]
            L[i][j] = s / d
    y = [0.0] * 6
    for i in range(6):
        s = b[i]
        for k in range(i):
            s -= L[i][k] * y[k]
        y[i] = s
    for i in range(6):
        y[i] /= D[i]
    x = [0.0] * 6
    for i in range(5, -1, -1):
        s = y[i]
        for k in range(i + 1, 6):
            s -= L[k][i] * x[k]
        x[i] = s
    return x


def iso_mul(A, B):
    out = np.zeros((4, 4))
    for i in range(4):
        for j in range(4):
            s = 0.0
            for k in range(4):
                s += float(A[i][k]) * float(B[k][j])
            out[i, j] = s
    return out


def iso_inverse(M):
    out = np.eye(4)
    for i in range(3):
        for j in range(3):
            out[i, j] = float(M[j][i])
    for i in range(3):
        out[i, 3] = -(out[i, 0] * float(M[0][3]) + out[i, 1] * float(M[1][3]) + out[i, 2] * float(M[2][3]))
    return out


def align(depth, camera, T_view, clouds, T_clouds, why=False, **params):
    """-> dict(T_view, info (with E as 4 x 4), valid, normals, record: per iteration dict(sums, E 3 x 4), H: the last iteration's as a 6 x 6 array; why: the
    first iteration's per-cloud reasons)"""
    P = dict(DEFAULTS, **params)
    T_view = np.asarray(T_view, np.float64)
    valid, normals = normal_map(depth, camera, P["tol_abs"], P["tol_rel_ppm"])
    Ms = [CR.rel_pose(T_view, Tc).tolist() for Tc in T_clouds]
    R = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    t = [0.0, 0.0, 0.0]
    info = dict(status=MAX_ITER, iterations=0, n_in=sum(len(c[::int(P["stride"])]) for c in clouds))
    record = []
    first_why = None
    cos_max = sincos64(float(P["max_angle"]))[1]
    hb, ch = 1.0 / float(1 << S_HB), 1.0 / float(1 << S_CHI)
    for it in range(int(P["max_iterations"])):
        E = [R[r] + [t[r]] for r in range(3)]
        res = accumulate(depth, camera, normals, clouds, Ms, E, P, why=why and it == 0)
        if why and it == 0:
            res, first_why = res
        record.append(dict(sums=res, E=np.array(E)))
        tested, inl, chi2 = res[I_TESTED], res[I_INLIER], float(res[I_CHI]) * ch
        if it == 0:
            info.update(tested_first=tested, inliers_first=inl, chi2_first=chi2)
        info.update(tested_last=tested, inliers_last=inl, chi2_last=chi2, iterations=it + 1)
        if inl < int(P["min_inliers"]):
            info["status"] = TOO_FEW
            break
        H = [float(v) * hb for v in res[:21]]
        b = [float(v) * hb for v in res[I_B:I_B + 6]]
        x = solve_ldlt(H, float(P["damping"]) * float(inl), b)
        if x is None:
            info["status"] = DEGENERATE
            break
        R, t = pose_oplus(R, t, x)
        fin = all(math.isfinite(v) for row in R for v in row) and all(math.isfinite(v) for v in t)
        shift = math.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]) if fin else math.inf
        cs = (((R[0][0] + R[1][1]) + R[2][2]) - 1.0) * 0.5
        if not fin or shift > float(P["max_shift"]) or cs < cos_max:
            info["status"] = DIVERGED
            break
        rot = math.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])
        tr = math.sqrt((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5])
        if rot < float(P["eps_rot"]) and tr < float(P["eps_trans"]):
            info["status"] = CONVERGED
            break
    E4 = np.eye(4)
    if info["status"] in (MAX_ITER, CONVERGED):
        E4[:3, :3] = R
        E4[:3, 3] = t
        T_out = iso_mul(T_view, iso_inverse(E4))
    else:
        T_out = T_view.copy()
    info["E"] = E4
    Hm = np.zeros((6, 6))
    k = 0
    for a in range(6):
        for c in range(a + 1):
            Hm[a, c] = Hm[c, a] = float(record[-1]["sums"][k]) * hb
            k += 1
    return dict(T_view=T_out, info=info, valid=valid, normals=normals, record=record, H=Hm, why=first_why)


def pose_error(T, T_true):
    """(translation in metres, rotation in radians) of inverse(T) . T_true"""
    D = np.linalg.inv(np.asarray(T, np.float64)) @ np.asarray(T_true, np.float64)
    c = min(1.0, max(-1.0, (np.trace(D[:3, :3]) - 1.0) * 0.5))
    return float(np.linalg.norm(D[:3, 3])), float(math.acos(c))
