#!/usr/bin/env python3
"""Times object extraction (ssm_objects_grid, ssm_objects_clouds, ssm_objects_points; csrc/kernels_objects.hip) at the pipeline's shape -- five full device-resident
clouds of a street scene (a camera 1.5 m above a ground plane, road and pavement, a wall 30 m ahead, a box labelled Vehicle on the road; the five key-frames two
metres apart, back-projected on the device from their depth and semantic images) into the default 512 x 512 cells of 0.2 m -- at 640 x 480 and 1241 x 376, and
writes profiles/r24_objects.md.  Stage 2 runs in both accumulate forms: one atomic per point and figure, and one per run of adjacent lanes with the same object.
Usage, from the repository root:  python3 scripts/objects_bench.py [--reps N] [--out FILE]      (python3 scripts/objects_bench.py --build-probe: only builds the probe)
Steps, each a process of its own under its own time limit, and the driver stops at the first that fails: `run` (the device calls' wall time on device clouds -- the
Mapper's route -- and on host arrays, the host chain ssm_objects_host on one core, equality), `trace` (rocprofv3 --kernel-trace: the split per kernel) and `probe`
(scripts/objects_probe, a build of the kernels with one debug counter: the atomics the point pass issues in each form -- the library has none).  No hardware
counters are collected."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import statistics
import struct
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = {"640x480": (640, 480), "1241x376": (1241, 376)}
M = 5
FORMS = {0: "per point", 1: "per run"}
STAGE1 = ("obj_begin_kernel", "obj_local_kernel", "obj_merge_kernel", "obj_flatten_kernel", "obj_clear_records_kernel", "obj_figures_kernel", "obj_keep_kernel", "obj_compact_kernel",
          "obj_paint_kernel")
STAGE2 = ("obj_points_begin_kernel", "obj_points_kernel", "obj_points_runs_kernel")
PROBE = os.path.join(ROOT, "scripts", "objects_probe")


def build_probe():
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-DOBJECTS_PROBE", os.path.join(ROOT, "scripts", "objects_probe.hip"), "-o", PROBE]
    subprocess.run(cmd, check=True)


def camera(which):
    w, h = SIZES[which]
    return (w / 2 - 0.3, h / 2 + 0.2, 0.8 * w, 0.8 * w, 1000.0)


def frame(k, which):
    """key-frame k of the street: (depth in mm, colour, semantic BGR)"""
    import numpy as np
    import semantic_slam_mapping_amd as ssm
    w, h = SIZES[which]
    cx, cy, f, _, scale = camera(which)
    rng = np.random.default_rng(900 + k)
    v, u = np.mgrid[0:h, 0:w]
    with np.errstate(divide="ignore"):
        z = np.where(v > cy, 1.5 * f / np.maximum(v - cy, 1e-9), 1e9)
    wall = z > 30.0
    z = np.where(wall, 30.0, z)
    box = (u > 0.62 * w) & (u < 0.75 * w) & (v > 0.4 * h) & (z > 6.0)
    z = np.where(box, 6.0, z) + rng.normal(0, 0.004, (h, w))
    x = (u - cx) * z / f
    label = np.where(box, 9, np.where(wall, 1, np.where(np.abs(x) < 3.0, 4, 5))).astype(np.uint8)
    return np.rint(z * scale).astype(np.uint16), rng.integers(0, 256, (h, w, 3), dtype=np.uint8), ssm.label_colours(label)


def poses():
    import numpy as np
    out = []
    for k in range(M):
        T = np.eye(4); T[2, 3] = 2.0 * k; T[0, 3] = 0.01 * k
        out.append(T)
    return out


def context(which):
    import semantic_slam_mapping_amd as ssm
    w, h = SIZES[which]
    return ssm.Context(0, width=w, height=h, orb_features=500, max_batch=1, voxel_capacity_log2=12, camera=camera(which))


class Chain:
    """the scene on the device and the calls through the library itself: the Python API's methods also download records and images, which is not what is timed"""
    def __init__(self, which):
        from semantic_slam_mapping_amd._lib import ObjectsInfo
        from semantic_slam_mapping_amd.api import _pack_clouds, objects_params
        self.ctx = ctx = context(which)
        self.T = poses()
        self.cl = [ctx.backproject_dev(*frame(k, which)) for k in range(M)]
        self.pts = [ctx.cloud_fetch(c).copy() for c in self.cl]
        self.keep, self.ptrs, self.n, self.Tc, self.m = _pack_clouds(self.pts, self.T, True)
        self.arr = (C.c_void_p * M)(*self.cl)
        self.gt = ctx.grid_target(512, 512); self.ot = ctx.objects_target(512, 512)
        self.P = objects_params(); self.I = ObjectsInfo()
        ctx.grid_clouds(self.gt, self.cl, self.T)
        ctx.objects_grid(self.gt, self.ot)                     # (through the binding once: it remembers the target's grid size for objects_fetch)

    def stage1(self):
        rc = self.ctx.lib.ssm_objects_grid(self.ctx.h, self.gt, C.byref(self.P), self.ot, C.byref(self.I))
        assert rc == 0, rc

    def stage2_clouds(self):
        rc = self.ctx.lib.ssm_objects_clouds(self.ctx.h, self.gt, self.ot, self.arr, self.Tc.ctypes.data, self.m, C.byref(self.I))
        assert rc == 0, rc

    def stage2_points(self):
        rc = self.ctx.lib.ssm_objects_points(self.ctx.h, self.gt, self.ot, self.ptrs, self.n.ctypes.data, self.Tc.ctypes.data, self.m, None, C.byref(self.I))
        assert rc == 0, rc

    def close(self):
        self.ctx.objects_target_free(self.ot); self.ctx.grid_target_free(self.gt)
        for c in self.cl:
            self.ctx.cloud_free(c)
        self.ctx.close()


def timed(fn, ctx, reps):
    ms = []
    for r in range(reps + 3):                                  # three untimed passes: the first allocates
        ctx.sync()
        t0 = time.perf_counter()
        fn()                                                   # (ends in the call's last wait)
        if r >= 3:
            ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def step_run(reps):
    import numpy as np
    import semantic_slam_mapping_amd as ssm
    out = {}
    for which in SIZES:
        ch = Chain(which)
        res = {"points": [len(p) for p in ch.pts], "host_ms": []}
        for r in range(3):
            t0 = time.perf_counter()
            rec, oid, ids, info = ssm.objects_host(ch.pts, ch.T)
            res["host_ms"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        ssm.grid_host(ch.pts, ch.T)
        res["grid_host_ms"] = (time.perf_counter() - t0) * 1e3
        assert len(rec) > 0 and info["object_points"] > 1000, "the scene holds no object"
        res["ms_stage1"] = timed(ch.stage1, ch.ctx, reps)
        for form in FORMS:
            ch.ctx.objects_form(form)
            for route, fn in (("clouds", ch.stage2_clouds), ("points", ch.stage2_points)):
                res[f"ms_{route}_{form}"] = timed(fn, ch.ctx, reps)
                got, goid = ch.ctx.objects_fetch(ch.ot)
                assert got.tobytes() == rec.tobytes() and np.array_equal(goid, oid) and np.array_equal(ch.ctx.objects_point_ids(len(ids)), ids), "device != host"
                assert {k: getattr(ch.I, k) for k in info} == info, "device != host"
        ch.ctx.objects_form(-1)
        res["info"] = info; res["objects"] = [[int(o["label"]), int(o["cells"]), int(o["n_points"])] for o in rec]
        out[which] = res
        ch.close()
    print(json.dumps(out))


def step_trace(reps):
    """what the rocprofv3 run executes: per scene, `reps` stage-1 calls, then `reps` stage-2 calls on the device clouds per form"""
    for which in SIZES:
        ch = Chain(which)
        for r in range(reps):
            ch.stage1()
        for form in FORMS:
            ch.ctx.objects_form(form)
            for r in range(reps):
                ch.stage2_clouds()
        ch.close()
    print(json.dumps({}))


def step_probe(reps):
    """the scenes as files for scripts/objects_probe, one run of it each: the clouds, and the grid's cells, object_id and records as the host functions give them"""
    import numpy as np
    import semantic_slam_mapping_amd as ssm
    from semantic_slam_mapping_amd.api import _cm16, grid_params
    if not os.path.exists(PROBE):
        build_probe()
    scenes = {}
    for which in SIZES:
        ch = Chain(which)
        scenes[which] = (ch.pts, ch.T)
        ch.close()          # (the probe is a process of its own: this one holds no context while it runs)
    out = {}
    d = tempfile.mkdtemp(prefix="objects_probe_")
    for which, (pts, T) in scenes.items():
        g = ssm.grid_host(pts, T, cells=True)
        rec, oid, _ = ssm.objects_cells_host(g["cls"], g["obstacle_label"], g["ground_q"], g["top_q"], g["n_high"])
        P = grid_params()
        path = os.path.join(d, f"{which}.bin")
        with open(path, "wb") as f:
            f.write(struct.pack("<4i", len(pts), P.nx, P.ny, len(rec))); f.write(bytes(P))
            f.write(np.ascontiguousarray(g["cells"]).tobytes()); f.write(np.ascontiguousarray(oid, np.int32).tobytes()); f.write(rec.tobytes())
            for p, Tk in zip(pts, T):
                f.write(struct.pack("<2i", len(p), 0)); f.write(_cm16(Tk).tobytes()); f.write(p.tobytes())
        r = subprocess.run(["timeout", "-k", "10", "120", PROBE, path], capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(f"objects_probe failed with status {r.returncode}; nothing further is started\n{r.stdout[-500:]}\n{r.stderr[-2000:]}")
        out[which] = json.loads(r.stdout.strip().splitlines()[-1])
        os.remove(path)
    print(json.dumps(out))


STEPS = {"run": step_run, "trace": step_trace, "probe": step_probe}


def run_step(name, reps, limit, prefix=()):
    cmd = ["timeout", "-k", "10", str(limit), *prefix, sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(reps)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit(f"objects_bench: step {name} failed with status {r.returncode}; nothing further is started\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def kernel_split(reps):
    """-> per scene {kernel: µs per launch (median)} from one traced run; the scenes run one after the other, each with the same number of launches per kernel"""
    d = tempfile.mkdtemp(prefix="objects_trace_")
    run_step("trace", reps, 420, prefix=("rocprofv3", "--kernel-trace", "-d", d, "-o", "objects", "--output-format", "csv", "--"))
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += [(int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3) for r in csv.DictReader(open(f))]
    rows.sort()
    per = {k: [] for k in STAGE1 + STAGE2 + ("scan",)}
    for _, name, us in rows:
        k = next((k for k in sorted(STAGE1 + STAGE2, key=len, reverse=True) if k in name), None)
        if k is None and "rocprim" in name and "scan" in name:
            k = "scan"
        if k is not None:
            per[k].append(us)
    out = {}
    for i, which in enumerate(SIZES):
        out[which] = {}
        for k, v in per.items():
            half = len(v) // len(SIZES)
            mine = v[i * half:(i + 1) * half]
            out[which][k] = [statistics.median(mine) if mine else 0.0, len(mine)]
    return out


def med(x, fmt="{:.3f}"):
    return fmt.format(statistics.median(x)) + " (" + fmt.format(min(x)) + " – " + fmt.format(max(x)) + ")"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS)); ap.add_argument("--reps", type=int, default=20); ap.add_argument("--build-probe", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_objects.md"))
    a = ap.parse_args()
    if a.build_probe:
        return build_probe()
    if a.step:
        return STEPS[a.step](a.reps)
    res = run_step("run", a.reps, 540)
    split = kernel_split(min(a.reps, 8))
    probe = run_step("probe", 1, 300)
    o = ["# r24: object extraction -- labelled obstacle instances from the ground grid\n",
         f"`python3 scripts/objects_bench.py` on one MI355X.  {M} full device-resident clouds of the street scene into 512 x 512 cells of 0.2 m, the default parameters of the grid "
         f"and of the objects; median (min – max) of {a.reps} calls after three untimed passes, wall time of each call in ms.  Stage 1 is `ssm_objects_grid` (nothing uploaded, "
         "two waits).  Stage 2 is `ssm_objects_clouds` on the device clouds (the Mapper's route: the table's upload, two launches, the info's download, one wait) and, beside it, "
         "`ssm_objects_points` on the same points as host arrays, whose wall time includes their upload (32 bytes per point).  The host chain is `ssm_objects_host` (the grid, "
         "then both stages) on one core through the Python binding, `ssm_grid_host` alone beside it.  Device == host on both routes and in both forms: records, object_id, "
         "per-point ids, info (asserted by the script).  No hardware counters were collected.\n",
         "| scene | points in the five clouds | objects (label, cells, points) | object points | stage 1, ms | `_clouds` per point, ms | `_clouds` per run, ms | `_points` per point, ms | `_points` per run, ms | "
         "`ssm_objects_host`, ms | of which `ssm_grid_host`, ms |\n|---|---|---|---|---|---|---|---|---|---|---|"]
    for which, r in res.items():
        o.append(f"| {which} | {sum(r['points'])} | {r['objects']} | {r['info']['object_points']} | {med(r['ms_stage1'])} | {med(r['ms_clouds_0'])} | {med(r['ms_clouds_1'])} | "
                 f"{med(r['ms_points_0'])} | {med(r['ms_points_1'])} | {med(r['host_ms'], '{:.1f}')} | {r['grid_host_ms']:.1f} |")
    o.append("\n## The kernels (rocprofv3 --kernel-trace, a run of its own on the device clouds; µs per launch, median over the launches)\n")
    o.append("| scene | " + " | ".join(k.replace("_kernel", "") for k in STAGE1 + ("scan",) + STAGE2) + " |\n|---|" + "---|" * (len(STAGE1) + 1 + len(STAGE2)))
    for which in res:
        g = split[which]
        o.append(f"| {which} | " + " | ".join(f"{g[k][0]:.1f}" for k in STAGE1 + ("scan",) + STAGE2) + " |")
    o.append("\n(`scan`: every rocPRIM scan launch of the run, two scans per stage 1 with several launches each; `obj_points_kernel` is form 0, `obj_points_runs_kernel` form 1.)")
    o.append("\n## The atomics of the point pass (a probe build with one debug counter, a run of its own)\n")
    o.append("| scene | points | object points | atomics per point form | per object point | atomics per run form | per object point |\n|---|---|---|---|---|---|---|")
    for which in res:
        p = probe[which]
        assert p["forms_agree"] and p["object_points"] == res[which]["info"]["object_points"]
        n = max(p["object_points"], 1)
        o.append(f"| {which} | {p['points']} | {p['object_points']} | {p['atomics_points']} | {p['atomics_points'] / n:.3f} | {p['atomics_runs']} | {p['atomics_runs'] / n:.3f} |")
    o.append("\nThe run form's min / max atomics depend on the order the waves happen to run in (a plain load first skips the atomic that cannot change the record); the records do "
             "not.  The probe's counter is an atomic of its own, so the probe build's times are not quoted.")
    for which in res:
        g = split[which]; r = res[which]
        p0, p1 = g["obj_points_kernel"][0], g["obj_points_runs_kernel"][0]
        o.append(f"\n{which}: the point pass takes {p0:.1f} µs per point and {p1:.1f} µs per run ({p0 / max(p1, 1e-9):.2f} x); `ssm_objects_clouds` takes "
                 f"{statistics.median(r['ms_clouds_0']):.3f} ms against {statistics.median(r['ms_clouds_1']):.3f} ms; stage 1 takes {statistics.median(r['ms_stage1']):.3f} ms; the device "
                 f"chain of the default form after the grid (stage 1 + `ssm_objects_clouds`) takes {statistics.median(r['ms_stage1']) + statistics.median(r['ms_clouds_1']):.3f} ms, "
                 f"the host chain {statistics.median(r['host_ms']):.1f} ms on one core, {r['grid_host_ms']:.1f} ms of it the grid.")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(o) + "\n")
    print("\n".join(o))


if __name__ == "__main__":
    main()
