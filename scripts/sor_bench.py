#!/usr/bin/env python3
"""Times the statistical outlier removal (ssm_cloud_sor / ssm_sor_filter, csrc/kernels_sor.hip) on key-frame clouds and writes profiles/r17_sor.md.
Clouds: frame 0 of the bench's synthetic stream at 640 x 480 (back-projected by ssm_backproject_dev) and a stereo-style road scene at 1241 x 376 (a road plane,
two boxes, a far wall, depth speckles), k = 30, stddev_mul = 1.0, automatic first cell size.
Usage, from the repository root:  python3 scripts/sor_bench.py [--reps N] [--out FILE]
Steps, each a process of its own under its own time limit, and the driver stops at the first that fails: `run` (the device-resident call, the call with host
arrays, the host function on one core, the ladder's figures) and `trace` (rocprofv3 --kernel-trace: the split per kernel and per level)."""
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
CAM = {"rgbd": (318.6, 255.3, 517.3, 516.5, 1000.0), "stereo": (609.5, 172.8, 721.5, 721.5, 1000.0)}
SIZES = {"rgbd": (640, 480), "stereo": (1241, 376)}


def frame(which):
    """-> (depth u16, bgr, sem) of the scene"""
    import numpy as np
    w, h = SIZES[which]
    if which == "rgbd":
        from oracle.binding import Oracle
        bgr, dep, sem, _, _ = Oracle().synth_frame(0x5EED0000, 0)
        return dep, bgr, sem
    cx, cy, fx, fy, _ = CAM[which]
    rng = np.random.default_rng(0x17)
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    z = np.full((h, w), 38.0)
    road = v > cy + 2
    z[road] = np.minimum(z[road], 1.65 * fy / (v[road] - cy))
    for (x0, x1, y0, y1, zz) in ((300, 450, 120, 210, 14.0), (800, 1000, 150, 230, 9.0)):
        z[y0:y1, x0:x1] = np.minimum(z[y0:y1, x0:x1], zz)
    disp = np.maximum(np.rint(fx * 0.54 / z * 16.0) / 16.0, 1.0 / 16.0)          # SGBM's sixteenths of a pixel
    dep = np.rint(fx * 0.54 / disp * 1000.0)
    dep[dep > 40000] = 0
    at = rng.choice(w * h, 400, replace=False)
    dep.reshape(-1)[at] = rng.integers(3000, 30000, 400)
    bgr = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    sem = np.zeros((h, w, 3), np.uint8); sem[:] = (128, 64, 128)
    return dep.astype(np.uint16), bgr, sem


def contexts(which):
    import semantic_slam_mapping_amd as ssm
    w, h = SIZES[which]
    return ssm.Context(0, width=w, height=h, orb_features=500, max_batch=1, voxel_capacity_log2=12, camera=CAM[which])


def step_run(reps):
    import numpy as np
    import semantic_slam_mapping_amd as ssm
    out = {}
    for which in SIZES:
        dep, bgr, sem = frame(which)
        ctx = contexts(which)
        pts = ctx.generate_point_cloud(dep, bgr, sem)
        res = {"points": len(pts), "cloud_ms": [], "arrays_ms": [], "host_ms": []}
        for r in range(reps + 1):                          # the first pass allocates
            cl = ctx.backproject_dev(dep, bgr, sem)
            ctx.sync()
            t0 = time.perf_counter()
            info = ctx.cloud_sor(cl)
            if r:
                res["cloud_ms"].append((time.perf_counter() - t0) * 1e3)
            kept_dev = ctx.cloud_fetch(cl)
            ctx.cloud_free(cl)
        res["level_queries"] = ctx.sor_levels()
        for r in range(reps + 1):
            t0 = time.perf_counter()
            kept, info2 = ctx.sor_filter(pts)
            if r:
                res["arrays_ms"].append((time.perf_counter() - t0) * 1e3)
        for r in range(3):
            t0 = time.perf_counter()
            hk, hinfo = ssm.sor_filter_host(pts)
            res["host_ms"].append((time.perf_counter() - t0) * 1e3)
        assert info == info2 == hinfo and kept.tobytes() == hk.tobytes() == kept_dev.tobytes(), "device != host"
        res.update(kept=info["n_kept"], levels=info["levels"], mean=info["mean"], stddev=info["stddev"], threshold=info["threshold"])
        out[which] = res
        ctx.close()
    print(json.dumps(out))


def step_trace(reps):
    """what the rocprofv3 run executes: per scene, `reps` device-resident calls"""
    out = {}
    for which in SIZES:
        dep, bgr, sem = frame(which)
        ctx = contexts(which)
        for r in range(reps):
            cl = ctx.backproject_dev(dep, bgr, sem)
            ctx.cloud_sor(cl)
            ctx.cloud_free(cl)
        out[which] = ctx.sor_levels()
        ctx.close()
    print(json.dumps(out))


STEPS = {"run": step_run, "trace": step_trace}
GROUPS = (("search", ("sor_search_kernel",)), ("statistics", ("sor_stats_kernel",)), ("compaction", ("sor_keep_kernel", "sor_compact_kernel", "scan")),
          ("sort", ("sor_keys_kernel", "sor_gather_kernel", "sort", "radix", "onesweep", "histogram", "partition", "select", "lookback")), ("bounds", ("sor_init_kernel", "sor_bounds_kernel")))


def run_step(name, reps, limit, prefix=()):
    cmd = ["timeout", "-k", "10", str(limit), *prefix, sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(reps)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit(f"sor_bench: step {name} failed with status {r.returncode}; nothing further is started\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def kernel_split(reps):
    """-> per scene: {group: µs per call (median over the calls)}, [µs of the search kernel per level], from one traced run; the two scenes run one after the other,
    and a call's kernels lie between two sor_init_kernel launches"""
    d = tempfile.mkdtemp(prefix="sor_trace_")
    levels = run_step("trace", reps, 420, prefix=("rocprofv3", "--kernel-trace", "-d", d, "-o", "sor", "--output-format", "csv", "--"))
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += [(int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3) for r in csv.DictReader(open(f))]
    rows.sort()
    calls, cur = [], None
    for _, name, us in rows:
        if "sor_init_kernel" in name:
            cur = []; calls.append(cur)
        if cur is not None and ("sor_" in name or "rocprim" in name):
            cur.append((name, us))
    out, at = {}, 0
    for which in SIZES:
        mine, at = calls[at:at + reps], at + reps
        groups = {g: [] for g, _ in GROUPS}; per_level = []
        for c in mine[1:] or mine:                        # the first call allocates
            tot = {g: 0.0 for g, _ in GROUPS}
            for name, us in c:
                g = next((g for g, keys in GROUPS if any(k in name for k in keys)), "sort")
                tot[g] += us
            for g in tot:
                groups[g].append(tot[g])
            per_level.append([us for name, us in c if "sor_search_kernel" in name])
        out[which] = ({g: statistics.median(v) for g, v in groups.items()}, [statistics.median(x) for x in zip(*per_level)], levels[which])
    return out


def med(x, fmt="{:.3f}"):
    return fmt.format(statistics.median(x)) + " (" + fmt.format(min(x)) + " – " + fmt.format(max(x)) + ")"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS)); ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_sor.md"))
    a = ap.parse_args()
    if a.step:
        return STEPS[a.step](a.reps)
    res = run_step("run", a.reps, 540)
    split = kernel_split(min(a.reps, 6))
    o = ["# r17: statistical outlier removal of key-frame clouds\n",
         f"`python3 scripts/sor_bench.py` on one MI355X.  k = 30, stddev_mul = 1.0, automatic first cell size; median (min – max) of {a.reps} calls after one untimed pass, wall time of the "
         "call in ms; the host function: 3 calls on one core, through the Python binding.  Device == host function on every cloud (asserted by the script).\n",
         "| cloud | points | kept | levels | `ssm_cloud_sor` (device-resident) | `ssm_sor_filter` (host arrays) | `ssm_sor_filter_host`, one core |\n|---|---|---|---|---|---|---|"]
    for which, r in res.items():
        w, h = SIZES[which]
        o.append(f"| {which} {w} x {h} | {r['points']} | {r['kept']} | {r['levels']} | {med(r['cloud_ms'])} | {med(r['arrays_ms'])} | {med(r['host_ms'], '{:.0f}')} |")
    for which, r in res.items():
        g, per_level, _ = split[which]
        q = r["level_queries"] + [0]
        o.append(f"\n## {which}: the ladder and the kernels (rocprofv3 --kernel-trace, a run of its own; µs per call, median)\n")
        o.append("| level | points still unsettled | settled here (share of all) | `sor_search_kernel` µs |\n|---|---|---|---|")
        for l in range(len(q) - 1):
            o.append(f"| {l} | {q[l]} | {(q[l] - q[l + 1]) / max(q[0], 1):.4f} | {per_level[l] if l < len(per_level) else float('nan'):.1f} |")
        o.append("\n| part | µs per call |\n|---|---|")
        for name in ("bounds", "sort", "search", "statistics", "compaction"):
            o.append(f"| {name}{' (keys, rocPRIM radix sort and select, gather; all levels)' if name == 'sort' else ''} | {g[name]:.1f} |")
        o.append(f"\nThe kernels sum to {sum(g.values()) / 1e3:.3f} ms; the call's wall time above also holds {r['levels'] + 3} small reads with a wait each and the launches.")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(o) + "\n")
    print("\n".join(o))


if __name__ == "__main__":
    main()
