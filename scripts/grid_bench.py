#!/usr/bin/env python3
"""Times the ground grid (ssm_grid_clouds, csrc/kernels_grid.hip) at the pipeline's shape -- one build from 5 device-resident clouds into 512 x 512 cells of 0.2 m --
and writes profiles/r21_grid.md.  Scenes: those of scripts/carve_bench.py (frame 0 of the bench's synthetic stream at 640 x 480, the stereo-style road scene at
1241 x 376; the five clouds are that frame seen from five poses a few centimetres apart), each in both accumulate forms: one atomic per point and address, and
one per run of adjacent lanes with the same destination.
Usage, from the repository root:  python3 scripts/grid_bench.py [--reps N] [--out FILE]      (python3 scripts/grid_bench.py --build-probe: only builds the probe)
Steps, each a process of its own under its own time limit, and the driver stops at the first that fails: `run` (the device call's wall time in both forms, the host
function on one core, equality), `trace` (rocprofv3 --kernel-trace: the split per kernel) and `probe` (scripts/grid_probe, a build of the kernels with two debug
counters: the atomics passes A and B issue in each form -- the library has neither).  No hardware counters are collected."""
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from sor_bench import SIZES, contexts  # noqa: E402
from carve_bench import scene, clouds_of, M  # noqa: E402

PROBE = os.path.join(ROOT, "scripts", "grid_probe")
KERNELS = ("grid_clear_kernel", "grid_pass_a_kernel", "grid_pass_a_runs_kernel", "grid_ground_kernel", "grid_pass_b_kernel", "grid_pass_b_runs_kernel", "grid_resolve_kernel")
FORMS = {0: "per point", 1: "per run"}
NX = NY = 512


def build_probe():
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-DGRID_PROBE", os.path.join(ROOT, "scripts", "grid_probe.hip"), "-o", PROBE]
    subprocess.run(cmd, check=True)


class Call:
    """the device call through the library itself: the Python API's methods also download the arrays, which is not what is timed here"""
    def __init__(self, ctx, Tc):
        from semantic_slam_mapping_amd._lib import GridInfo
        from semantic_slam_mapping_amd.api import _cm16, grid_params
        import numpy as np
        self.ctx = ctx
        self.t = ctx.grid_target(NX, NY)
        self.P = grid_params(); self.I = GridInfo()
        self.Tc = np.ascontiguousarray(np.stack([_cm16(T) for T in Tc]))

    def build(self, clouds):
        arr = (C.c_void_p * len(clouds))(*clouds)
        rc = self.ctx.lib.ssm_grid_clouds(self.ctx.h, self.t, arr, self.Tc.ctypes.data, len(clouds), C.byref(self.P), C.byref(self.I))
        assert rc == 0, rc


def step_run(reps):
    import semantic_slam_mapping_amd as ssm
    out = {}
    for which in SIZES:
        imgs, vdep, Tv, Tc = scene(which)
        ctx = contexts(which)
        cl = clouds_of(ctx, imgs)
        pts = [ctx.cloud_fetch(c).copy() for c in cl]
        call = Call(ctx, Tc)
        res = {"points": len(pts[0]), "host_ms": []}
        for r in range(3):
            t0 = time.perf_counter()
            host = ssm.grid_host(pts, Tc, cells=True)
            res["host_ms"].append((time.perf_counter() - t0) * 1e3)
        for form in FORMS:
            ctx.grid_form(form)
            ms = []
            for r in range(reps + 3):                          # three untimed passes: the first allocates
                ctx.sync()
                t0 = time.perf_counter()
                call.build(cl)                                 # (ends in the call's one wait)
                if r >= 3:
                    ms.append((time.perf_counter() - t0) * 1e3)
            dev = ctx.grid_clouds(call.t, cl, Tc, cells=True)
            assert dev["info"] == host["info"] and dev["cells"].tobytes() == host["cells"].tobytes(), "device != host"
            assert all(dev[k].tobytes() == host[k].tobytes() for k in ("cls", "ground_label", "obstacle_label", "ground_q", "top_q", "n", "n_high")), "device != host"
            res[f"ms_{form}"] = ms
        ctx.grid_form(-1)
        res["info"] = host["info"]; res["n_max"] = int(host["n"].max())
        out[which] = res
        ctx.grid_target_free(call.t)
        for c in cl:
            ctx.cloud_free(c)
        ctx.close()
    print(json.dumps(out))


def step_trace(reps):
    """what the rocprofv3 run executes: per scene and form, `reps` builds"""
    for which in SIZES:
        imgs, vdep, Tv, Tc = scene(which)
        ctx = contexts(which)
        cl = clouds_of(ctx, imgs)
        call = Call(ctx, Tc)
        for form in FORMS:
            ctx.grid_form(form)
            for r in range(reps):
                call.build(cl)
        ctx.grid_target_free(call.t)
        for c in cl:
            ctx.cloud_free(c)
        ctx.close()
    print(json.dumps({}))


def step_probe(reps):
    """the scenes as files for scripts/grid_probe, one run of it each"""
    from semantic_slam_mapping_amd.api import _cm16, grid_params
    if not os.path.exists(PROBE):
        build_probe()
    scenes = {}
    for which in SIZES:
        imgs, vdep, Tv, Tc = scene(which)
        ctx = contexts(which)
        cl = clouds_of(ctx, imgs)
        scenes[which] = ([ctx.cloud_fetch(c).copy() for c in cl], Tc)
        for c in cl:
            ctx.cloud_free(c)
        ctx.close()          # (the probe is a process of its own: this one holds no context while it runs)
    out = {}
    d = tempfile.mkdtemp(prefix="grid_probe_")
    for which, (pts, Tc) in scenes.items():
        path = os.path.join(d, f"{which}.bin")
        with open(path, "wb") as f:
            f.write(struct.pack("<2i", len(pts), 0)); f.write(bytes(grid_params()))
            for p, T in zip(pts, Tc):
                f.write(struct.pack("<2i", len(p), 0)); f.write(_cm16(T).tobytes()); f.write(p.tobytes())
        r = subprocess.run(["timeout", "-k", "10", "120", PROBE, path], capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(f"grid_probe failed with status {r.returncode}; nothing further is started\n{r.stderr[-2000:]}")
        out[which] = json.loads(r.stdout.strip().splitlines()[-1])
        os.remove(path)
    print(json.dumps(out))


STEPS = {"run": step_run, "trace": step_trace, "probe": step_probe}


def run_step(name, reps, limit, prefix=()):
    cmd = ["timeout", "-k", "10", str(limit), *prefix, sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(reps)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit(f"grid_bench: step {name} failed with status {r.returncode}; nothing further is started\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def kernel_split(reps):
    """-> per scene and form {kernel: µs per build (median over the builds)} from one traced run; a build's kernels begin with a grid_clear_kernel launch"""
    d = tempfile.mkdtemp(prefix="grid_trace_")
    run_step("trace", reps, 420, prefix=("rocprofv3", "--kernel-trace", "-d", d, "-o", "grid", "--output-format", "csv", "--"))
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += [(int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3) for r in csv.DictReader(open(f))]
    rows.sort()
    calls = []
    for _, name, us in rows:
        k = next((k for k in sorted(KERNELS, key=len, reverse=True) if k in name), None)
        if k is None:
            continue
        if k == "grid_clear_kernel":
            calls.append({})
        if calls:
            calls[-1][k] = calls[-1].get(k, 0.0) + us
    out, at = {}, 0
    for which in SIZES:
        for form in FORMS:
            mine, at = calls[at:at + reps], at + reps
            out[f"{which} {form}"] = {k: statistics.median([c.get(k, 0.0) for c in (mine[1:] or mine)]) for k in KERNELS}          # the first build allocates
    return out


def med(x, fmt="{:.3f}"):
    return fmt.format(statistics.median(x)) + " (" + fmt.format(min(x)) + " – " + fmt.format(max(x)) + ")"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS)); ap.add_argument("--reps", type=int, default=20); ap.add_argument("--build-probe", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_grid.md"))
    a = ap.parse_args()
    if a.build_probe:
        return build_probe()
    if a.step:
        return STEPS[a.step](a.reps)
    res = run_step("run", a.reps, 540)
    split = kernel_split(min(a.reps, 8))
    probe = run_step("probe", 1, 300)
    o = ["# r21: ground grid -- bird's-eye semantic elevation map of clouds\n",
         f"`python3 scripts/grid_bench.py` on one MI355X.  One build from {M} device-resident clouds (`ssm_grid_clouds`) into {NX} x {NY} cells of 0.2 m, the default "
         f"parameters; median (min – max) of {a.reps} calls after three untimed passes, wall time of each call in ms (the table's upload, clear, pass A, ground, pass B, "
         "resolve, the info's download, one wait); the host function: 3 passes on one core, through the Python binding.  Device == host function in both forms: every raw "
         "cell, the seven arrays, the info (asserted by the script).  No hardware counters were collected.\n",
         "| scene | points per cloud | used points / cells hit / most points in a cell | `ssm_grid_clouds` per point, ms | `ssm_grid_clouds` per run, ms | `ssm_grid_host`, one core, ms |\n|---|---|---|---|---|---|"]
    for which, r in res.items():
        w, h = SIZES[which]
        hit = NX * NY - r["info"]["unobserved"]
        o.append(f"| {which} {w} x {h} | {r['points']} | {r['info']['n_used']} / {hit} / {r['n_max']} | {med(r['ms_0'])} | {med(r['ms_1'])} | {med(r['host_ms'], '{:.1f}')} |")
    o.append("\n## The kernels (rocprofv3 --kernel-trace, a run of its own; µs per build, median) and the atomics of passes A and B (a probe build with two debug counters, a run of its own)\n")
    o.append("| scene, form | clear | pass A | ground | pass B | resolve | sum | atomics pass A | per used point | atomics pass B | per used point |\n|---|---|---|---|---|---|---|---|---|---|---|")
    for which in res:
        p = probe[which]
        for form, name in FORMS.items():
            g = split[f"{which} {form}"]
            a_us = g["grid_pass_a_runs_kernel" if form else "grid_pass_a_kernel"]; b_us = g["grid_pass_b_runs_kernel" if form else "grid_pass_b_kernel"]
            na, nb = (p["a_runs"], p["b_runs"]) if form else (p["a_points"], p["b_points"])
            total = g["grid_clear_kernel"] + a_us + g["grid_ground_kernel"] + b_us + g["grid_resolve_kernel"]
            o.append(f"| {which}, {name} | {g['grid_clear_kernel']:.1f} | {a_us:.1f} | {g['grid_ground_kernel']:.1f} | {b_us:.1f} | {g['grid_resolve_kernel']:.1f} | {total:.1f} | "
                     f"{na} | {na / max(p['used'], 1):.3f} | {nb} | {nb / max(p['used'], 1):.3f} |")
    o.append("\nPass A's min / max atomics depend on the order the waves happen to run in (a plain load first skips the atomic that cannot change the cell); the cells do not.  "
             "The probe's counters are atomics of their own, so the probe build's times are not quoted.")
    for which in res:
        g0, g1 = split[f"{which} 0"], split[f"{which} 1"]
        ab0 = g0["grid_pass_a_kernel"] + g0["grid_pass_b_kernel"]; ab1 = g1["grid_pass_a_runs_kernel"] + g1["grid_pass_b_runs_kernel"]
        o.append(f"\n{which}: passes A + B take {ab0:.1f} µs per point and {ab1:.1f} µs per run ({ab0 / max(ab1, 1e-9):.2f} x); "
                 f"the call's wall time {statistics.median(res[which]['ms_0']):.3f} ms against {statistics.median(res[which]['ms_1']):.3f} ms; "
                 f"the host function takes {statistics.median(res[which]['host_ms']):.1f} ms on one core.")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(o) + "\n")
    print("\n".join(o))


if __name__ == "__main__":
    main()
