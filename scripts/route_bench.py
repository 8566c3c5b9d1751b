#!/usr/bin/env python3
"""Times the route field (ssm_route_field, ssm_debug_route_cells, ssm_route_path; csrc/kernels_route.hip) and writes the next free profiles/rNN_route.md: on the built
grid of scripts/objects_bench.py's street scene (five full device-resident 640 x 480 clouds into the default 512 x 512 cells of 0.2 m, then the clearance map) and on
hand-made 512 x 512 and 2048 x 2048 inputs -- open, 30 % blocked, a serpentine and a spiral -- each in both forms (0: sweeps of one thread per cell in batches, 1:
active tiles relaxed to their fixed points) with the rounds each needed, against ssm_route_cells_host on one core, results equal; then the path query at paths of
about 100, 1000 and 10000 cells against downloading the field and walking on the host.
Usage, from the repository root:  python3 scripts/route_bench.py [--reps N] [--out FILE]
Wall times of whole calls only (a call ends in its own wait); no per-kernel trace and no hardware counters are collected.  Form 0 is not run where its sweeps alone
would number more than SWEEP_LIMIT (one launch each): the table says so."""
import argparse
import ctypes as C
import glob
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
FORMS = {0: "sweeps", 1: "active tiles"}
SWEEP_LIMIT = 300000


def serpentine(n):
    import numpy as np
    r = np.full((n, n), 2, np.uint8)
    for y in range(1, n, 2):
        r[y, :] = 0
        r[y, n - 1 if y % 4 == 1 else 0] = 2
    return r


def spiral(n):
    """square rings two cells apart, each cut just below its top-left corner and joined to the next one inwards: one corridor wound to the middle"""
    import numpy as np
    r = np.zeros((n, n), np.uint8)
    for k in range(0, n // 2 - 2, 2):
        m = n - 1 - k
        r[k, k:m + 1] = 2; r[m, k:m + 1] = 2; r[k:m + 1, k] = 2; r[k:m + 1, m] = 2
        r[k + 1, k] = 0
        r[k + 2, k + 1] = 2
    return r


def hand_made(which, n):
    import numpy as np
    rng = np.random.default_rng(27)
    if which == "open":
        r = np.full((n, n), 2, np.uint8)
    elif which == "30 % blocked":
        r = np.where(rng.random((n, n)) < 0.3, 0, 2).astype(np.uint8)
        r[n // 2, n // 2] = 2
    elif which == "serpentine":
        r = serpentine(n)
    else:
        r = spiral(n)
    d = rng.integers(1, 200, (n, n)).astype(np.uint32)
    source = (0, 0) if which in ("serpentine", "spiral") else (n // 2, n // 2)
    return r, d, source


def timed(fn, ctx, reps):
    ms = []
    for r in range(reps + 1):                                  # one untimed pass: the first allocates
        ctx.sync()
        t0 = time.perf_counter()
        fn()                                                   # (ends in the call's wait)
        dt = (time.perf_counter() - t0) * 1e3
        if r >= 1:
            ms.append(dt)
        if dt > 500.0 and r >= 1:
            break
    return ms


def med(ms):
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import objects_bench as OB
    import semantic_slam_mapping_amd as ssm
    from semantic_slam_mapping_amd._lib import RouteInfo
    ctx = OB.context("640x480")
    T = OB.poses()
    clouds = [ctx.backproject_dev(*OB.frame(k, "640x480")) for k in range(OB.M)]
    gt = ctx.grid_target(512, 512)
    ctx.grid_clouds(gt, clouds, T)
    ct = ctx.clearance_target(512, 512)
    cinfo = ctx.clearance_grid(gt, ct, radius=1.0, seed=(256, 40), seed_snap=50)
    d2, _, reach = ctx.clearance_fetch(ct)
    small, big = ctx.route_target(512, 512, 512 * 512), ctx.route_target(2048, 2048, 65536)
    I = RouteInfo(); P = ssm.route_params()
    rows = []

    def measure(name, call, target, shape, host_args, sweeps_needed, **host_kw):
        host_ms = []
        for _ in range(2):
            t0 = time.perf_counter()
            want = ssm.route_cells_host(*host_args, **host_kw)
            host_ms.append((time.perf_counter() - t0) * 1e3)
        row = dict(name=name, host_ms=min(host_ms), info=want[2])
        for form in FORMS:
            if form == 0 and sweeps_needed > SWEEP_LIMIT:
                row[form] = None
                continue
            ctx.route_form(form)
            ms = timed(call, ctx, a.reps)
            got = ctx.route_fetch(target, shape=shape)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and {k: getattr(I, k) for k in want[2]} == want[2], "device != host"
            row[form] = (med(ms), min(ms), len(ms), ctx.route_rounds())
        ctx.route_form(-1)
        rows.append(row)
        print(row, flush=True)
        return want

    def chk(rc):
        assert rc == 0, (rc, ctx.lib.ssm_last_error(ctx.h))

    built = measure("built 512x512 (%d reachable)" % cinfo["reachable"], lambda: chk(ctx.lib.ssm_route_field(ctx.h, ct, C.byref(P), small, C.byref(I))), small, (512, 512),
                    (reach, d2, cinfo["seed_cell"]), 0, cell=ssm.grid_params().cell)          # (the field takes the grid's cell size)
    del built
    keep = None
    for n, target in ((512, small), (2048, big)):
        for which in ("open", "30 % blocked", "serpentine", "spiral"):
            r, d, source = hand_made(which, n)
            src = source[1] * n + source[0]
            # the longest path's cells bound form 0's sweeps: about n^2 / 2 on the one-way scenes
            sweeps = n * n // 2 if which in ("serpentine", "spiral") else 4 * n
            want = measure("%dx%d %s" % (n, n, which), lambda: chk(ctx.lib.ssm_debug_route_cells(ctx.h, target, r.ctypes.data, d.ctypes.data, n, n, src, C.byref(P), C.byref(I))), target, (n, n),
                           (r, d, src), sweeps)
            if n == 512 and which == "serpentine":
                keep = (r, d, src, want)
    # the path query on the 512 x 512 serpentine: goals about 100, 1000 and 10000 cells along the one way
    r, d, src, want = keep
    ctx.route_cells(small, r, d, src)
    paths = []
    from semantic_slam_mapping_amd._lib import RoutePathInfo
    buf = np.zeros(512 * 512, np.int32); PI = RoutePathInfo()
    for goal in ((100, 0), (24, 2), (250, 38)):
        ms = timed(lambda: chk(ctx.lib.ssm_route_path(ctx.h, small, goal[0], goal[1], 0, buf.ctypes.data, C.byref(PI))), ctx, a.reps)
        cells, pi = ctx.route_path(small, goal, 0)
        hc, hpi = ssm.route_path_host(want[0], want[1], d, goal, 0, max_path=512 * 512)
        assert np.array_equal(cells, hc) and pi == hpi, "device path != host path"

        def on_host():
            cost, parent = ctx.route_fetch(small)
            ssm.route_path_host(cost, parent, d, goal, 0, max_path=512 * 512)
        hms = timed(on_host, ctx, a.reps)
        paths.append((pi["len"], med(ms), min(ms), med(hms), min(hms)))
        print(paths[-1], flush=True)
    out = a.out
    if out is None:
        used = [int(m.group(1)) for f in glob.glob(os.path.join(ROOT, "profiles", "r*_*.md")) for m in [re.match(r"r(\d+)_", os.path.basename(f))] if m]
        out = os.path.join(ROOT, "profiles", "r%02d_route.md" % (max(used + [0]) + 1))
    with open(out, "w") as f:
        f.write("# Route field: both forms, the host function, the path query\n\n")
        f.write("MI355X, wall time of a whole call in ms (median / best of up to %d calls after one untimed; a call slower than 0.5 s is timed once), `rounds`: how often the call asked the\n"
                "device whether it was done (form 0: batches of %d sweeps; form 1: rounds of active tiles).  Defaults: 8 moves, near_weight 2, comfort 2.0 m (cell 0.2 m on the built grid, 1 m\n"
                "on the hand-made ones, whose dist2 is random).  Every device result equals the host function's.  No per-kernel trace was taken.\n\n" % (a.reps, ssm.load().ssm_debug_route_batch()))
        f.write("| scene | routed | max cost | form 0 ms (median / best) | form 0 rounds | form 1 ms (median / best) | form 1 rounds | host, one core, ms |\n|---|---|---|---|---|---|---|---|\n")
        for row in rows:
            cellf = lambda v: "not run (over %d sweeps) | -" % SWEEP_LIMIT if v is None else "%.3f / %.3f | %d" % (v[0], v[1], v[3])  # noqa: E731
            f.write("| %s | %d | %d | %s | %s | %.1f |\n" % (row["name"], row["info"]["routed"], row["info"]["max_cost"], cellf(row[0]), cellf(row[1]), row["host_ms"]))
        f.write("\nThe path query on the 512 x 512 serpentine's field (ssm_route_path: the snap, the walk by one lane, two downloads) against ssm_route_fetch of cost and parent followed by\n"
                "ssm_route_path_host:\n\n| path cells | device ms (median / best) | fetch + host walk ms (median / best) |\n|---|---|---|\n")
        for p in paths:
            f.write("| %d | %.3f / %.3f | %.3f / %.3f |\n" % p)
    print("wrote", out)
    ctx.route_target_free(small); ctx.route_target_free(big); ctx.clearance_target_free(ct); ctx.grid_target_free(gt)
    for c in clouds:
        ctx.cloud_free(c)
    ctx.close()


if __name__ == "__main__":
    main()
