#!/usr/bin/env python3
"""Times the semantic-motion fusion (ssm_motion_fuse_dev, csrc/kernels_motion_fuse.hip) at KITTI size and writes profiles/r16_motion_fuse.md.
Configuration: 1241 x 376, one call of 64 frames.  The frames carry the two boxes of the U/V-disparity bench's scenes (scripts/uvd_bench.py: one drifting right,
one drifting left) painted in the Car colour, a pedestrian, an outlined car (a hole to fill) and sparse class noise; the motion mask is painted over the first
box and a little noise -- it is not computed by UVDisparity here.
Usage, from the repository root:  python3 scripts/motion_fuse_bench.py [--reps N] [--parent DIR] [--out FILE]
Steps, each a process of its own under its own time limit, and the driver stops at the first that fails: `run` (the device call, the host function on one
core, the per-frame back-projection with the class mask and with the fusion), `trace` (rocprofv3 --kernel-trace --stats: the per-kernel split), then bench.py
alternated with the parent commit's tree (--parent DIR: a built checkout of the parent; left out when not given)."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
W, H, N = 1241, 376, 64
CAR, PED, ROAD = (128, 0, 64), (0, 64, 64), (128, 64, 128)


def frames():
    import numpy as np
    rng = np.random.default_rng(0x16)
    sem = np.zeros((N, H, W, 3), np.uint8); sem[:] = ROAD
    motion = np.zeros((N, H, W), np.uint8)
    for f in range(N):
        a, b = 300 + 3 * f, 800 - 2 * f
        sem[f, 120:210, a:a + 150] = CAR; motion[f, 110:200, a - 5:a + 155] = 255
        sem[f, 150:230, b:b + 200] = CAR
        sem[f, 140:230, 60 + f:80 + f] = PED
        sem[f, 250:330, 500:640] = CAR; sem[f, 253:327, 503:637] = ROAD
        u = rng.random((H, W))
        sem[f][u < 0.001] = CAR
        motion[f][rng.random((H, W)) < 0.01] = 255
    return sem, motion


def step_run(reps):
    import numpy as np
    import semantic_slam_mapping_amd as ssm
    sem, motion = frames()
    ctx = ssm.Context(0, width=W, height=H, orb_features=1000, max_batch=1, voxel_capacity_log2=12)
    px = W * H
    d_sem, d_mot, d_mask = ctx.dev_alloc(N * px * 3), ctx.dev_alloc(N * px), ctx.dev_alloc(N * px)
    ctx.h2d(d_sem, sem); ctx.h2d(d_mot, motion)
    import ctypes as C
    from semantic_slam_mapping_amd._lib import MotionFuseParams
    P = MotionFuseParams(1000, 0, 0.143); info = np.zeros(N, ssm.MOTION_FUSE_INFO_DTYPE)
    res = {"dev_ms": [], "host_ms": [], "plain_ms": [], "fused_ms": []}
    for r in range(reps + 1):                         # the first pass allocates
        ctx.sync()
        t0 = time.perf_counter()
        ctx._chk(ctx.lib.ssm_motion_fuse_dev(ctx.h, d_sem, d_mot, N, W, H, C.byref(P), d_mask, info.ctypes.data))       # ends in the call's one wait
        if r:
            res["dev_ms"].append((time.perf_counter() - t0) * 1e3 / N)
    mask = ctx.d2h(d_mask, (N, H, W), np.uint8)
    # the host function on one core, and device == host on the frames timed
    hf = 4
    for r in range(2):
        t0 = time.perf_counter()
        host = [ssm.motion_fuse_host(sem[f], motion[f]) for f in range(hf)]
        res["host_ms"].append((time.perf_counter() - t0) * 1e3 / hf)
    assert all(np.array_equal(host[f][0], mask[f]) and host[f][1] == {k: int(info[f][k]) for k in info.dtype.names} for f in range(hf)), "device != host"
    # per key-frame, host images in and points out: the class mask + back-projection of the parent (ssm_backproject) against the fused form
    depth = rng_depth()
    bf = 16
    for r in range(reps + 1):
        for key, fn in (("plain_ms", lambda f: ctx.generate_point_cloud(depth, sem[f], sem[f])), ("fused_ms", lambda f: ctx.backproject_fused(depth, sem[f], sem[f], motion[f]))):
            t0 = time.perf_counter()
            npts = [len(fn(f)) for f in range(bf)]
            if r:
                res[key].append((time.perf_counter() - t0) * 1e3 / bf)
            res[key + "_points"] = int(sum(npts))
    res.update(blobs=int(info["blobs"].sum()), large=int(info["large"].sum()), confirmed=int(info["confirmed"].sum()), added=int(info["added"].sum()), host_frames=hf, bp_frames=bf)
    ctx.close()
    print(json.dumps(res))


def rng_depth():
    import numpy as np
    return np.random.default_rng(7).integers(500, 30000, (H, W)).astype(np.uint16)


def step_trace(reps):
    """what the rocprofv3 run executes: three calls of 64 frames"""
    import numpy as np
    import semantic_slam_mapping_amd as ssm
    sem, motion = frames()
    ctx = ssm.Context(0, width=W, height=H, orb_features=1000, max_batch=1, voxel_capacity_log2=12)
    for r in range(3):
        ctx.motion_fuse(sem, motion)
    ctx.close()
    print(json.dumps({"ok": True}))


STEPS = {"run": step_run, "trace": step_trace}


def run_step(name, reps, limit, prefix=()):
    cmd = ["timeout", "-k", "10", str(limit), *prefix, sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(reps)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit(f"motion_fuse_bench: step {name} failed with status {r.returncode}; nothing further is started\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def kernel_stats(reps):
    d = tempfile.mkdtemp(prefix="mf_trace_")
    run_step("trace", reps, 420, prefix=("rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "mf", "--output-format", "csv", "--"))
    per = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "mf_" in r["Kernel_Name"]:
                name = r["Kernel_Name"].split("(")[0].replace("void ", "").replace(".kd", "").strip()          # (template arguments hold blanks)
                per.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: (len(v), sum(v[1:]) / max(len(v) - 1, 1), min(v), max(v)) for k, v in per.items()}          # the mean leaves out the first launch


def bench_line(tree, limit=900):
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "bench.py"], capture_output=True, text=True, cwd=tree)
    if r.returncode != 0:
        raise SystemExit(f"motion_fuse_bench: bench.py in {tree} failed with status {r.returncode}\n{r.stderr[-3000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def rng_of(x, fmt="{:.4f}"):
    return fmt.format(min(x)) + " – " + fmt.format(max(x))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS)); ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: bench.py runs there and here in alternation")
    ap.add_argument("--bench-rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_motion_fuse.md"))
    a = ap.parse_args()
    if a.step:
        return STEPS[a.step](a.reps)
    res = run_step("run", a.reps, 540)
    ks = kernel_stats(a.reps)
    bench = {"parent": [], "new": []}
    if a.parent:
        for _ in range(a.bench_rounds):
            for who, tree in (("parent", a.parent), ("new", ROOT)):
                bench[who].append(bench_line(tree))
    o = []
    o.append("# r16: the semantic-motion fusion at KITTI size\n")
    o.append(f"`python3 scripts/motion_fuse_bench.py` on one MI355X.  {W} x {H}; the device call is one `ssm_motion_fuse_dev` of {N} device-resident frames (eight launches, one wait); "
             f"{a.reps} timed repetitions after one untimed pass; ranges are min – max over the repetitions; times in ms PER FRAME.  The frames: the two boxes of the "
             "U/V-disparity bench painted as cars, a pedestrian, an outlined car, class noise; the motion mask is painted over the first box (not computed by UVDisparity here).  "
             f"Over the {N} frames: {res['blobs']} blobs, {res['large']} large, {res['confirmed']} confirmed, {res['added']} pixels added to the class mask.  "
             f"Device == host function on the first {res['host_frames']} frames (asserted by the script).\n")
    o.append("| what | ms per frame (min – max) |\n|---|---|")
    o.append(f"| `ssm_motion_fuse_dev`, {N} frames per call: wall time of the call / {N} (counters fetched, one wait) | {rng_of(res['dev_ms'])} |")
    o.append(f"| `ssm_motion_fuse_host` on one core ({res['host_frames']} frames, through the Python binding) | {rng_of(res['host_ms'], '{:.2f}')} |")
    o.append(f"| `ssm_backproject` per frame (the parent's `k_moving_mask` + back-projection; host images in, {res['plain_ms_points'] // res['bp_frames']} points out) | {rng_of(res['plain_ms'], '{:.3f}')} |")
    o.append(f"| `ssm_backproject_fused` per frame (the same with the fusion and the motion mask's upload; {res['fused_ms_points'] // res['bp_frames']} points out) | {rng_of(res['fused_ms'], '{:.3f}')} |")
    md, mh = sum(res["dev_ms"]) / len(res["dev_ms"]), sum(res["host_ms"]) / len(res["host_ms"])
    mp, mf = sum(res["plain_ms"]) / len(res["plain_ms"]), sum(res["fused_ms"]) / len(res["fused_ms"])
    o.append(f"\nThe batched device call is {mh / md:.0f} x the host function on one core.  Per key-frame the fused back-projection costs {mf - mp:+.3f} ms over the plain one "
             f"({mp:.3f} -> {mf:.3f} ms; both are dominated by the copies of the images in and the points out; it returns fewer points).\n")
    o.append(f"## The kernels (rocprofv3 --kernel-trace, a run of its own: three calls of {N} frames; µs per launch of {N} frames)\n")
    o.append("| kernel | launches | mean (first left out) | min | max |\n|---|---|---|---|---|")
    tot = 0.0
    for k in sorted(ks, key=lambda k: -ks[k][1]):
        n, mean, lo, hi = ks[k]; tot += mean
        o.append(f"| `{k}` | {n} | {mean:.1f} | {lo:.1f} | {hi:.1f} |")
    o.append(f"\nSum of the means: {tot:.1f} µs per call = {tot / N:.2f} µs per frame; the call's wall time per frame above also holds the counters' copy, the wait and eight launches.\n")
    if a.parent:
        o.append("## `python bench.py` (default line), parent commit and this tree alternated in one call\n")
        o.append("| tree | " + " | ".join(f"run {i + 1}" for i in range(a.bench_rounds)) + " | range |\n|---|" + "---|" * (a.bench_rounds + 1))
        for who in ("parent", "new"):
            vals = [b.get("value") for b in bench[who]]
            o.append(f"| {who} | " + " | ".join(f"{x:.1f}" for x in vals) + f" | {rng_of(vals, '{:.1f}')} |")
        o.append(f"\n(`{bench['new'][0].get('metric', 'value')}`, {bench['new'][0].get('unit', '')}; nothing on the benchmark's path is touched: the fusion runs only where it is asked for.)\n")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(o) + "\n")
    print("\n".join(o))


if __name__ == "__main__":
    main()
