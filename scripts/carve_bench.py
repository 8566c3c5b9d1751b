#!/usr/bin/env python3
"""Times free-space carving (ssm_carve, csrc/kernels_carve.hip) at the pipeline's shape -- one view against the clouds of the 5 key-frames before it -- and writes
profiles/r18_carve.md.  Scenes: frame 0 of the bench's synthetic stream at 640 x 480 and the stereo-style road scene of scripts/sor_bench.py at 1241 x 376; the five
clouds are that frame seen from five poses a few centimetres apart, the view is the frame with one region pushed back (seen through there) and depth noise.
Usage, from the repository root:  python3 scripts/carve_bench.py [--reps N] [--out FILE]
Steps, each a process of its own under its own time limit, and the driver stops at the first that fails: `run` (the device-resident call, the host function on
one core, equality) and `trace` (rocprofv3 --kernel-trace: the split per kernel)."""
import argparse
import csv
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from sor_bench import CAM, SIZES, frame, contexts  # noqa: E402

M = 5
KERNELS = ("carve_init_kernel", "carve_verdict_kernel", "scan", "carve_base_kernel", "carve_compact_kernel", "carve_store_kernel")


def scene(which):
    """-> (depth, bgr, sem) of the key-frames, the view's depth, the view's pose, the M cloud poses"""
    import numpy as np
    dep, bgr, sem = frame(which)
    rng = np.random.default_rng(18)
    view = dep.astype(np.int64) + rng.integers(-8, 9, dep.shape)
    h, w = dep.shape
    view[:, w // 4: w // 3] += 1500
    view = np.clip(view, 1, 65535)
    view[dep == 0] = 0
    poses = []
    for k in range(M + 1):
        T = np.eye(4)
        T[0, 3] = 0.02 * k
        T[2, 3] = 0.01 * k
        poses.append(T)
    return (dep, bgr, sem), view.astype(np.uint16), poses[M], poses[:M]


def clouds_of(ctx, imgs):
    return [ctx.backproject_dev(*imgs) for _ in range(M)]


def step_run(reps):
    import semantic_slam_mapping_amd as ssm
    out = {}
    for which in SIZES:
        imgs, vdep, Tv, Tc = scene(which)
        ctx = contexts(which)
        pts = ctx.generate_point_cloud(*imgs)
        view = ctx.carve_view(vdep, CAM[which])
        res = {"points": len(pts), "call_ms": [], "host_ms": []}
        for r in range(reps + 1):                          # the first pass allocates
            cl = clouds_of(ctx, imgs)
            ctx.sync()
            t0 = time.perf_counter()
            infos = ctx.carve(view, Tv, cl, Tc)              # (ends in the call's one wait)
            if r:
                res["call_ms"].append((time.perf_counter() - t0) * 1e3)
            if r == reps:
                kept = [ctx.cloud_fetch(c).tobytes() for c in cl]
                runs = [ctx.cloud_run(c).tobytes() for c in cl]
            for c in cl:
                ctx.cloud_free(c)
        for r in range(3):
            t0 = time.perf_counter()
            host = [ssm.carve_host(vdep, CAM[which], Tv, pts, Tc[k]) for k in range(M)]
            res["host_ms"].append((time.perf_counter() - t0) * 1e3)
        assert all(infos[k] == host[k][2] and kept[k] == host[k][0].tobytes() and runs[k] == host[k][1].tobytes() for k in range(M)), "device != host"
        res["infos"] = infos
        out[which] = res
        ctx.carve_view_free(view)
        ctx.close()
    print(json.dumps(out))


def step_trace(reps):
    """what the rocprofv3 run executes: per scene, `reps` device-resident calls"""
    for which in SIZES:
        imgs, vdep, Tv, Tc = scene(which)
        ctx = contexts(which)
        view = ctx.carve_view(vdep, CAM[which])
        for r in range(reps):
            cl = clouds_of(ctx, imgs)
            ctx.carve(view, Tv, cl, Tc)
            for c in cl:
                ctx.cloud_free(c)
        ctx.carve_view_free(view)
        ctx.close()
    print(json.dumps({}))


STEPS = {"run": step_run, "trace": step_trace}


def run_step(name, reps, limit, prefix=()):
    cmd = ["timeout", "-k", "10", str(limit), *prefix, sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(reps)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit(f"carve_bench: step {name} failed with status {r.returncode}; nothing further is started\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def kernel_split(reps):
    """-> per scene {kernel: µs per call (median over the calls)} from one traced run; a call's kernels lie between two carve_init_kernel launches"""
    d = tempfile.mkdtemp(prefix="carve_trace_")
    run_step("trace", reps, 420, prefix=("rocprofv3", "--kernel-trace", "-d", d, "-o", "carve", "--output-format", "csv", "--"))
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += [(int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3) for r in csv.DictReader(open(f))]
    rows.sort()
    calls, cur = [], None
    for _, name, us in rows:
        if "carve_init_kernel" in name:
            cur = []; calls.append(cur)
        elif cur is not None and "carve_" not in name and "rocprim" not in name and "scan" not in name.lower():
            cur = None                                     # the next key-frame's back-projection: the call is over
        if cur is not None:
            cur.append((name, us))
    out, at = {}, 0
    for which in SIZES:
        mine, at = calls[at:at + reps], at + reps
        per = {k: [] for k in KERNELS}
        for c in mine[1:] or mine:                        # the first call allocates
            tot = {k: 0.0 for k in KERNELS}
            for name, us in c:
                tot[next((k for k in KERNELS if k in name), "scan")] += us
            for k in tot:
                per[k].append(tot[k])
        out[which] = {k: statistics.median(v) for k, v in per.items()}
    return out


def med(x, fmt="{:.3f}"):
    return fmt.format(statistics.median(x)) + " (" + fmt.format(min(x)) + " – " + fmt.format(max(x)) + ")"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS)); ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_carve.md"))
    a = ap.parse_args()
    if a.step:
        return STEPS[a.step](a.reps)
    res = run_step("run", a.reps, 540)
    split = kernel_split(min(a.reps, 6))
    o = ["# r18: free-space carving of key-frame clouds\n",
         f"`python3 scripts/carve_bench.py` on one MI355X.  One view against {M} device-resident clouds (`ssm_carve`), default parameters; median (min – max) of {a.reps} calls "
         "after one untimed pass, wall time of the call in ms (the table's upload, the kernels, the infos' download, one wait); the host function: 3 passes over the same "
         f"{M} clouds on one core, through the Python binding.  Device == host function on every cloud: points, counters and infos (asserted by the script).\n",
         f"| view | points per cloud | kept / seen through / supported / occluded / unknown (cloud 0) | `ssm_carve`, {M} clouds, ms | `ssm_carve_host`, {M} clouds, one core, ms |\n|---|---|---|---|---|"]
    for which, r in res.items():
        w, h = SIZES[which]
        i = r["infos"][0]
        o.append(f"| {which} {w} x {h} | {r['points']} | {i['n_kept']} / {i['seen_through']} / {i['supported']} / {i['occluded']} / {i['unknown']} | {med(r['call_ms'])} | {med(r['host_ms'], '{:.1f}')} |")
    for which, r in res.items():
        g = split[which]
        n = M * r["points"]
        kept = sum(i["n_kept"] for i in r["infos"])
        # what the algorithm has to move, from the shapes: the verdict kernel reads a point's 32-byte record (x, y, z share its line with the rest) and its counter and
        # writes three bytes; the compaction reads two flags per point and moves 33 bytes per kept point into the scratch copy, the store moves them back
        need = n * (32 + 1 + 3) + n * 2 + kept * (33 + 33) + kept * (33 + 33)
        total = sum(g.values())
        o.append(f"\n## {which}: the kernels (rocprofv3 --kernel-trace, a run of its own; µs per call, median)\n")
        o.append("| kernel | µs per call | share |\n|---|---|---|")
        for k in KERNELS:
            o.append(f"| {k if k != 'scan' else 'rocPRIM exclusive scan over the blocks'} | {g[k]:.1f} | {g[k] / max(total, 1e-9):.2f} |")
        o.append(f"\nThe kernels sum to {total / 1e3:.3f} ms for {n} points, {kept} kept.  Bytes the algorithm needs (the depth window comes from L2 and is not counted): "
                 f"{need / 1e6:.1f} MB, {need / n:.0f} per point; over the kernels' time that is {need / max(total, 1e-9) / 1e6:.2f} TB/s against 6.3 TB/s of achievable HBM "
                 f"bandwidth.  The verdict kernel alone: {n * 36 / max(g['carve_verdict_kernel'], 1e-9) / 1e6:.2f} TB/s of its own {n * 36 / 1e6:.1f} MB.")
    o.append("\nOpen: the kept points cross memory three times (cloud -> scratch copy -> cloud); a decoupled look-back over the blocks would let the compaction write the "
             "cloud in place in one pass.  The verdict kernel reads x, y, z out of 32-byte records; a structure-of-arrays copy of the positions is not kept.  Neither was tried.")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(o) + "\n")
    print("\n".join(o))


if __name__ == "__main__":
    main()
