#!/usr/bin/env python3
"""Times the clearance map (ssm_clearance_grid, ssm_debug_clearance_cells; csrc/kernels_clearance.hip) and writes profiles/r26_clearance.md: on the built grid of
scripts/objects_bench.py's street scene (five full device-resident 640 x 480 clouds into the default 512 x 512 cells of 0.2 m) and on hand-made 2048 x 2048 class
images with one blocked cell (the outward scan's worst case), 0.1 % and 5 % blocked -- each in both row-pass forms (0: the whole row staged through LDS, 1: an
outward scan that stops at the best distance) and against ssm_clearance_cells_host on one core, results equal.
Usage, from the repository root:  python3 scripts/clearance_bench.py [--reps N] [--out FILE]
Steps, each a process of its own under its own time limit, and the driver stops at the first that fails: `run` (the calls' wall time, the host function, equality)
and `trace` (rocprofv3 --kernel-trace: the split per kernel).  No hardware counters are collected."""
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))
SCENES = ("built 512x512", "2048x2048 one blocked", "2048x2048 0.1 %", "2048x2048 5 %")
FORMS = {0: "whole row through LDS", 1: "outward scan"}
KERNELS = ("clr_begin_kernel", "clr_mask_kernel", "clr_column_kernel", "clr_row_lds_kernel", "clr_row_scan_kernel", "clr_seed_kernel", "clr_local_kernel", "clr_merge_kernel", "clr_flatten_kernel",
           "clr_finish_kernel")
OTHERS = tuple(k for k in KERNELS if "row" not in k)
RADIUS = 1.0


def hand_made(which):
    import numpy as np
    rng = np.random.default_rng(26)
    c = np.full((2048, 2048), 1, np.uint8)
    if which.endswith("one blocked"):
        c[1024, 1024] = 4
    else:
        c[rng.random(c.shape) < (0.001 if "0.1" in which else 0.05)] = 4
    return c, dict(radius=RADIUS, cell=0.2, seed=(5, 5), seed_snap=50)


class Bench:
    """the scenes on the device and the calls through the library itself: the binding's fetch downloads the images, which is not what is timed"""
    def __init__(self):
        import objects_bench as OB
        import semantic_slam_mapping_amd as ssm
        from semantic_slam_mapping_amd._lib import ClearanceInfo
        self.ctx = ctx = OB.context("640x480")
        self.T = OB.poses()
        self.cl = [ctx.backproject_dev(*OB.frame(k, "640x480")) for k in range(OB.M)]
        self.gt = ctx.grid_target(512, 512)
        self.grid = ctx.grid_clouds(self.gt, self.cl, self.T)
        self.cell = ssm.grid_params().cell
        self.small, self.big = ctx.clearance_target(512, 512), ctx.clearance_target(2048, 2048)
        self.I = ClearanceInfo()
        self.built = dict(radius=RADIUS, seed=(256, 40), seed_snap=50)

    def scene(self, which):
        """-> (the call, the target, the class image, the host function's keywords)"""
        import numpy as np
        import semantic_slam_mapping_amd as ssm
        if which.startswith("built"):
            P = ssm.clearance_params(**self.built)
            return (lambda: self._chk(self.ctx.lib.ssm_clearance_grid(self.ctx.h, self.gt, C.byref(P), self.small, C.byref(self.I)))), self.small, self.grid["cls"], dict(self.built, cell=self.cell), (512, 512)
        cls, kw = hand_made(which)
        P = ssm.clearance_params(**kw); a = np.ascontiguousarray(cls)
        return (lambda: self._chk(self.ctx.lib.ssm_debug_clearance_cells(self.ctx.h, self.big, a.ctypes.data, 2048, 2048, C.byref(P), C.byref(self.I)))), self.big, cls, kw, (2048, 2048)

    @staticmethod
    def _chk(rc):
        assert rc == 0, rc

    def close(self):
        self.ctx.clearance_target_free(self.small); self.ctx.clearance_target_free(self.big); self.ctx.grid_target_free(self.gt)
        for c in self.cl:
            self.ctx.cloud_free(c)
        self.ctx.close()


def timed(fn, ctx, reps):
    ms = []
    for r in range(reps + 3):                                  # three untimed passes: the first allocates
        ctx.sync()
        t0 = time.perf_counter()
        fn()                                                   # (ends in the call's wait)
        if r >= 3:
            ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def step_run(reps):
    import numpy as np
    import semantic_slam_mapping_amd as ssm
    from semantic_slam_mapping_amd.api import CLEARANCE_INFO_FIELDS
    b = Bench()
    out = {}
    for which in SCENES:
        call, target, cls, kw, (nx, ny) = b.scene(which)
        res = {"host_ms": []}
        for r in range(3):
            t0 = time.perf_counter()
            want = ssm.clearance_cells_host(cls, **kw)
            res["host_ms"].append((time.perf_counter() - t0) * 1e3)
        for form in FORMS:
            b.ctx.clearance_form(form)
            res[f"ms_{form}"] = timed(call, b.ctx, reps)
            b.ctx._clearance_sizes[target] = (nx, ny)
            got = b.ctx.clearance_fetch(target)
            assert all(np.array_equal(g, w) for g, w in zip(got, want[:3])) and {k: getattr(b.I, k) for k in CLEARANCE_INFO_FIELDS} == want[3], "device != host"
        b.ctx.clearance_form(-1)
        res["info"] = want[3]
        out[which] = res
    b.close()
    print(json.dumps(out))


def step_trace(reps):
    """what the rocprofv3 run executes: per scene and form, `reps` calls"""
    b = Bench()
    for which in SCENES:
        call = b.scene(which)[0]
        for form in FORMS:
            b.ctx.clearance_form(form)
            for r in range(reps):
                call()
    b.close()
    print(json.dumps({}))


STEPS = {"run": step_run, "trace": step_trace}


def run_step(name, reps, limit, prefix=()):
    cmd = ["timeout", "-k", "10", str(limit), *prefix, sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(reps)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit(f"clearance_bench: step {name} failed with status {r.returncode}; nothing further is started\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def kernel_split(reps):
    """-> per scene {kernel: µs per launch (median)} from one traced run; the scenes run one after the other, each with the same number of launches per kernel (a
    row kernel runs under its own form only, the seed kernel in every call: every scene has a seed)"""
    d = tempfile.mkdtemp(prefix="clearance_trace_")
    run_step("trace", reps, 420, prefix=("rocprofv3", "--kernel-trace", "-d", d, "-o", "clearance", "--output-format", "csv", "--"))
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += [(int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3) for r in csv.DictReader(open(f))]
    rows.sort()
    per = {k: [] for k in KERNELS}
    for _, name, us in rows:
        k = next((k for k in KERNELS if k in name), None)
        if k is not None:
            per[k].append(us)
    out = {}
    for i, which in enumerate(SCENES):
        out[which] = {}
        for k, v in per.items():
            share = len(v) // len(SCENES)
            mine = v[i * share:(i + 1) * share]
            out[which][k] = [statistics.median(mine) if mine else 0.0, len(mine)]
    return out


def med(x, fmt="{:.3f}"):
    return fmt.format(statistics.median(x)) + " (" + fmt.format(min(x)) + " – " + fmt.format(max(x)) + ")"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS)); ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_clearance.md"))
    a = ap.parse_args()
    if a.step:
        return STEPS[a.step](a.reps)
    res = run_step("run", a.reps, 540)
    split = kernel_split(min(a.reps, 8))
    o = ["# r26: clearance map -- obstacle distance and reachable free space of the ground grid\n",
         f"`python3 scripts/clearance_bench.py` on one MI355X.  `built 512x512`: `ssm_clearance_grid` on the grid of five full device-resident 640 x 480 clouds of the street scene "
         f"(`scripts/objects_bench.py`) in the default 512 x 512 cells of 0.2 m -- nothing uploaded, one download (the info), one wait.  `2048x2048 ...`: `ssm_debug_clearance_cells` on a "
         f"hand-made class image, every cell drivable but the blocked ones; its wall time includes the image's upload (4 MiB).  radius {RADIUS} m, cells of 0.2 m (r2 = 25), "
         f"connectivity 4, a seed.  Median (min – max) of {a.reps} calls after three untimed passes, wall time of each call in ms, in both row-pass forms; "
         "`ssm_clearance_cells_host` on one core through the Python binding beside them (median of 3).  Device == host in both forms on every scene: dist2, nearest, reach, info "
         "(asserted by the script).  No hardware counters were collected: not measured.\n",
         "| scene | blocked | traversable | reachable | components | form 0 (whole row through LDS), ms | form 1 (outward scan), ms | `ssm_clearance_cells_host`, ms |\n|---|---|---|---|---|---|---|---|"]
    for which, r in res.items():
        i = r["info"]
        o.append(f"| {which} | {i['blocked']} | {i['traversable']} | {i['reachable']} | {i['components']} | {med(r['ms_0'])} | {med(r['ms_1'])} | {med(r['host_ms'], '{:.1f}')} |")
    o.append("\n## The kernels (rocprofv3 --kernel-trace, a run of its own; µs per launch, median over the launches of both forms; a row kernel runs under its own form only)\n")
    o.append("| scene | " + " | ".join(k.replace("_kernel", "") for k in KERNELS) + " |\n|---|" + "---|" * len(KERNELS))
    for which in res:
        g = split[which]
        o.append(f"| {which} | " + " | ".join(f"{g[k][0]:.1f}" for k in KERNELS) + " |")
    for which in res:
        g = split[which]; r = res[which]
        rest = sum(g[k][0] for k in OTHERS)
        o.append(f"\n{which}: the row pass takes {g['clr_row_lds_kernel'][0]:.1f} µs as form 0 and {g['clr_row_scan_kernel'][0]:.1f} µs as form 1, the other kernels {rest:.1f} µs together; a call "
                 f"takes {statistics.median(r['ms_0']):.3f} / {statistics.median(r['ms_1']):.3f} ms where the host function takes {statistics.median(r['host_ms']):.1f} ms on one core.")
    b0, b1 = statistics.median(res[SCENES[0]]["ms_0"]), statistics.median(res[SCENES[0]]["ms_1"])
    k0, k1 = split[SCENES[0]]["clr_row_lds_kernel"][0], split[SCENES[0]]["clr_row_scan_kernel"][0]
    fast = 0 if k0 <= k1 else 1
    worst = max(SCENES, key=lambda w: split[w][("clr_row_lds_kernel", "clr_row_scan_kernel")[fast]][0] / max(split[w][("clr_row_scan_kernel", "clr_row_lds_kernel")[fast]][0], 1e-9))
    w0, w1 = split[worst]["clr_row_lds_kernel"][0], split[worst]["clr_row_scan_kernel"][0]
    o.append(f"\nOn the built grid form {fast} is the faster row pass ({k0:.1f} against {k1:.1f} µs per launch; {b0:.3f} against {b1:.3f} ms per call): it is the default.  Its worst case "
             f"against the other form is `{worst}`: {w0:.1f} µs as form 0 against {w1:.1f} µs as form 1.  Form 0 evaluates, for every cell, every column of the row that holds a blocked "
             "cell, however near the nearest one is -- its cost grows with the row's length and with how many columns hold something; form 1 stops at the best distance, so it wins where "
             "blocked cells are dense and loses where rows hold little or nothing (`one blocked`: it walks the whole row from every cell, one global load per step).")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(o) + "\n")
    print("\n".join(o))


if __name__ == "__main__":
    main()
