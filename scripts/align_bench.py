#!/usr/bin/env python3
"""Times dense alignment (ssm_align_view_create, ssm_align_clouds, csrc/kernels_align.hip) at the pipeline's shape -- one view against 5 device-resident clouds --
and writes profiles/r20_align.md.  Scenes: the analytic ones of tests/align_cases.py (a room corner with a box at 640 x 480, a road with a box under KITTI's
camera at 1241 x 376; the five clouds are the scene seen from five poses a few centimetres apart, the view's pose carries a planted error), every scene synthetic.
Usage, from the repository root:  python3 scripts/align_bench.py [--reps N] [--out FILE]
Steps, each a process of its own under its own time limit, and the driver stops at the first that fails: `run` (the device calls' wall time, the host function on
one core, equality of every iteration's sums, the pose and the info) and `trace` (rocprofv3 --kernel-trace: the time per kernel)."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

M = 5
SIZES = {"rgbd": (640, 480), "stereo": (1241, 376)}
CAM = {"rgbd": (319.5, 239.5, 520.0, 520.0, 1000.0), "stereo": (607.2, 185.2, 718.9, 718.9, 1000.0)}
KERNELS = ("align_normals_kernel", "align_accumulate_kernel")
ITERATIONS = 4          # fixed: eps 0, so that every call runs the same number of accumulations
PARAMS = dict(max_iterations=ITERATIONS, eps_rot=0.0, eps_trans=0.0)
BYTES_PER_POINT = 48 + 16 + 2          # the point's 48-byte record (its lines are read whole), the pixel's normal and depth
HBM_TBS = 8.0                          # the chip's HBM roof, TB/s


def scene(which):
    """-> (view depth, planted view pose, [cloud depth images], [cloud poses]) """
    import numpy as np
    import align_cases as AC
    w, h = SIZES[which]
    if which == "rgbd":
        scn, Tt = AC.ROOM, AC.VIEW
        poses = [Tt @ AC.se3(tx=0.03 * (k - 2), ty=0.01 * k, ry=0.004 * (k - 2)) for k in range(M)]
    else:
        scn, Tt = AC.ROAD, AC.se3(tz=1.0)
        poses = [AC.se3(tz=0.2 * k, tx=0.02 * k) for k in range(M)]
    planted = AC.se3(rx=0.004, ry=-0.005, rz=0.003, tx=0.01, ty=0.02, tz=0.03)
    return AC.ray_cast(scn, Tt, CAM[which], w, h), Tt @ planted, [AC.ray_cast(scn, T, CAM[which], w, h) for T in poses], poses


def context(which):
    import semantic_slam_mapping_amd as ssm
    w, h = SIZES[which]
    return ssm.Context(0, width=w, height=h, orb_features=500, max_batch=1, voxel_capacity_log2=12, camera=CAM[which])


def clouds_of(ctx, which, deps):
    import numpy as np
    w, h = SIZES[which]
    bgr = np.full((h, w, 3), 90, np.uint8); sem = np.zeros((h, w, 3), np.uint8); sem[:] = (128, 64, 128)
    return [ctx.backproject_dev(d, bgr, sem, max_distance=60.0) for d in deps]


class Call:
    """the device call through the library itself, with everything converted beforehand"""
    def __init__(self, ctx, view, Tv, Tc):
        import numpy as np
        from semantic_slam_mapping_amd._lib import AlignInfo
        from semantic_slam_mapping_amd.api import _cm16, align_params
        self.ctx, self.view = ctx, view
        self.P = align_params(**PARAMS); self.I = AlignInfo(); self.out = np.zeros(16)
        self.Tv = _cm16(Tv); self.Tc = np.ascontiguousarray(np.stack([_cm16(T) for T in Tc]))

    def align(self, clouds):
        arr = (C.c_void_p * len(clouds))(*clouds)
        rc = self.ctx.lib.ssm_align_clouds(self.ctx.h, self.view, self.Tv.ctypes.data, arr, self.Tc.ctypes.data, len(clouds), C.byref(self.P), self.out.ctypes.data, C.byref(self.I))
        assert rc == 0, rc


def step_run(reps):
    import semantic_slam_mapping_amd as ssm
    out = {}
    for which in SIZES:
        vdep, Tv, deps, Tc = scene(which)
        ctx = context(which)
        cl = clouds_of(ctx, which, deps)
        pts = [ctx.cloud_fetch(c).copy() for c in cl]
        res = {"points": [len(p) for p in pts], "view_ms": [], "align_ms": [], "host_ms": []}
        for r in range(reps + 3):                              # three untimed passes: the first allocates
            ctx.sync()
            t0 = time.perf_counter()
            v = ctx.align_view(vdep, CAM[which])
            t1 = time.perf_counter()
            call = Call(ctx, v, Tv, Tc)
            t2 = time.perf_counter()
            call.align(cl)                                     # (ends in the last iteration's wait)
            t3 = time.perf_counter()
            if r >= 3:
                res["view_ms"].append((t1 - t0) * 1e3); res["align_ms"].append((t3 - t2) * 1e3)
            ctx.align_view_free(v)
        v = ctx.align_view(vdep, CAM[which])
        dev = ctx.align_clouds(v, Tv, cl, Tc, **PARAMS)
        rec = ctx.align_record()
        valid, normals = ctx.align_normals(v)
        ctx.align_view_free(v)
        for r in range(3):
            t0 = time.perf_counter()
            host = ssm.align_host(vdep, CAM[which], Tv, pts, Tc, **PARAMS)
            res["host_ms"].append((time.perf_counter() - t0) * 1e3)
        assert rec.tobytes() == host["record"].tobytes() and dev["T_view"].tobytes() == host["T_view"].tobytes(), "device != host"
        assert all(dev["info"][f] == host["info"][f] for f in ssm.api.ALIGN_INFO_FIELDS) and normals.tobytes() == host["normals"].tobytes() and (valid == host["valid"]).all(), "device != host"
        res["info"] = {f: dev["info"][f] for f in ssm.api.ALIGN_INFO_FIELDS}
        out[which] = res
        for c in cl:
            ctx.cloud_free(c)
        ctx.close()
    print(json.dumps(out))


def step_trace(reps):
    """what the rocprofv3 run executes: per scene `reps` views and alignments"""
    for which in SIZES:
        vdep, Tv, deps, Tc = scene(which)
        ctx = context(which)
        cl = clouds_of(ctx, which, deps)
        for r in range(reps):
            v = ctx.align_view(vdep, CAM[which])
            Call(ctx, v, Tv, Tc).align(cl)
            ctx.align_view_free(v)
        for c in cl:
            ctx.cloud_free(c)
        ctx.close()
    print(json.dumps({}))


STEPS = {"run": step_run, "trace": step_trace}


def run_step(name, reps, limit, prefix=()):
    cmd = ["timeout", "-k", "10", str(limit), *prefix, sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(reps)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit(f"align_bench: step {name} failed with status {r.returncode}; nothing further is started\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def kernel_split(reps):
    """-> per scene {kernel: µs per launch (median)} from one traced run; the scenes run one after the other, `reps` views and reps x ITERATIONS accumulations each"""
    d = tempfile.mkdtemp(prefix="align_trace_")
    run_step("trace", reps, 420, prefix=("rocprofv3", "--kernel-trace", "-d", d, "-o", "align", "--output-format", "csv", "--"))
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += [(int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3) for r in csv.DictReader(open(f))]
    rows.sort()
    out = {}
    for k in KERNELS:
        mine = [us for _, name, us in rows if k in name]
        per = len(mine) // len(SIZES)
        for i, which in enumerate(SIZES):
            out.setdefault(which, {})[k] = statistics.median(mine[i * per:(i + 1) * per][1:])          # the first launch of a scene is left out
    return out


def med(x, fmt="{:.3f}"):
    return fmt.format(statistics.median(x)) + " (" + fmt.format(min(x)) + " – " + fmt.format(max(x)) + ")"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS)); ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_align.md"))
    a = ap.parse_args()
    if a.step:
        return STEPS[a.step](a.reps)
    res = run_step("run", a.reps, 540)
    split = kernel_split(min(a.reps, 8))
    o = ["# r20: dense alignment -- point-to-plane ICP of map clouds to a key-frame\n",
         f"`python3 scripts/align_bench.py` on one MI355X.  One view against {M} device-resident clouds; every scene is synthetic (analytic planes and a box, ray-cast).  "
         f"`ssm_align_view_create`: the depth image's upload, the normal map, one wait.  `ssm_align_clouds`: {ITERATIONS} iterations (eps 0, so that the count is fixed), each "
         f"one launch, one download of 30 integers, one wait and the 6 x 6 solve on the host.  Median (min – max) of {a.reps} calls after three untimed passes, wall time in ms; "
         "the host function: 3 passes on one core, through the Python binding (it also builds the normal map).  Device == host function: every iteration's raw sums, counts "
         "and E, the valid mask and normals, the pose and every info field (asserted by the script).\n",
         "| view | points in the 5 clouds | inliers first / last | `ssm_align_view_create`, ms | `ssm_align_clouds`, ms | per iteration, ms | `ssm_align_host`, one core, ms |\n|---|---|---|---|---|---|---|"]
    for which, r in res.items():
        w, h = SIZES[which]
        o.append(f"| {which} {w} x {h} | {sum(r['points'])} | {r['info']['inliers_first']} / {r['info']['inliers_last']} | {med(r['view_ms'])} | {med(r['align_ms'])} | "
                 f"{statistics.median(r['align_ms']) / ITERATIONS:.3f} | {med(r['host_ms'], '{:.1f}')} |")
    o.append("\n## The kernels (rocprofv3 --kernel-trace, a run of its own; µs per launch, median)\n")
    o.append(f"| view | normals | accumulate | bytes the accumulate kernel moves ({BYTES_PER_POINT} per point: the 48-byte record, 16 of normal, 2 of depth) | at that time, GB/s | share of the HBM roof ({HBM_TBS:.0f} TB/s) |\n|---|---|---|---|---|---|")
    for which, r in res.items():
        g = split[which]
        b = sum(r["points"]) * BYTES_PER_POINT
        gbs = b / max(g["align_accumulate_kernel"], 1e-9) / 1e3
        o.append(f"| {which} | {g['align_normals_kernel']:.1f} | {g['align_accumulate_kernel']:.1f} | {b} | {gbs:.0f} | {gbs / (HBM_TBS * 1e3):.3f} |")
    o.append("\nThe byte count is an upper bound of the traffic from HBM: the points are streamed once, but the view's depth and normals (18 bytes per pixel, "
             "5 - 8 MB) are gathered by five clouds' points and stay in L2 / the Infinity Cache between them.  No counters were collected, so what follows is SUPPOSITION: "
             "at about a fifth of the HBM roof by that upper bound, with about a hundred double-precision operations and 28 conversions to 64-bit integers per inlier and two dependent gathers in front "
             "of them, the accumulate kernel looks bound by the latency of those gathers and by the FP64 / integer-conversion rate at its occupancy (104 VGPRs: 4 waves per "
             "SIMD), not by memory bandwidth; per call the iteration's launch, download and wait add a fixed cost that the table's `per iteration` column contains.")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(o) + "\n")
    print("\n".join(o))


if __name__ == "__main__":
    main()
