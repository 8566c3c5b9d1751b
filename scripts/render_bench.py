#!/usr/bin/env python3
"""Times map rendering (ssm_render_clouds, ssm_render_compare, csrc/kernels_render.hip) at the pipeline's shape -- one view against 5 device-resident clouds -- and
writes profiles/r19_render.md.  Scenes: those of scripts/carve_bench.py (frame 0 of the bench's synthetic stream at 640 x 480, the stereo-style road scene at
1241 x 376; the five clouds are that frame seen from five poses a few centimetres apart), each at point_size 0 (one pixel per point) and at a size that gives
splats of radius 1 - 2.
Usage, from the repository root:  python3 scripts/render_bench.py [--reps N] [--out FILE]      (python3 scripts/render_bench.py --build-probe: only builds the probe)
Steps, each a process of its own under its own time limit, and the driver stops at the first that fails: `run` (the device calls' wall time, the host functions on
one core, equality), `trace` (rocprofv3 --kernel-trace: the split per kernel) and `probe` (scripts/render_probe, a build of the splat kernel with two debug
counters: footprint pixels offered and atomics issued -- the library has neither)."""
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
from sor_bench import CAM, SIZES, contexts  # noqa: E402
from carve_bench import scene, clouds_of, M  # noqa: E402

PROBE = os.path.join(ROOT, "scripts", "render_probe")
KERNELS = ("render_clear_kernel", "render_splat_kernel", "render_resolve_kernel", "render_counts_clear_kernel", "render_compare_kernel")
SPLATS = {"rgbd": (0.0, 0.012), "stereo": (0.0, 0.08)}          # point_size per scene: one pixel, and a size that gives radius 1 - 2 at the scene's depths
MAX_RADIUS = 2


def build_probe():
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-DRENDER_PROBE", os.path.join(ROOT, "scripts", "render_probe.hip"), "-o", PROBE]
    subprocess.run(cmd, check=True)


class Call:
    """the two device calls through the library itself: the Python API's methods also download the images, which is not what is timed here"""
    def __init__(self, ctx, which, Tv, Tc, ps):
        from semantic_slam_mapping_amd._lib import RenderParams, RenderInfo, RenderCompareInfo
        from semantic_slam_mapping_amd.api import _cm16, _render_params
        import numpy as np
        self.ctx, self.w, self.h = ctx, *SIZES[which]
        self.t = ctx.render_target(self.w, self.h)
        self.P = _render_params(dict(point_size=ps, max_radius=MAX_RADIUS)); self.I = RenderInfo(); self.J = RenderCompareInfo()
        self.Tv = _cm16(Tv); self.Tc = np.ascontiguousarray(np.stack([_cm16(T) for T in Tc]))

    def render(self, clouds):
        arr = (C.c_void_p * len(clouds))(*clouds)
        rc = self.ctx.lib.ssm_render_clouds(self.ctx.h, self.t, C.byref(self.ctx.cfg.camera), self.Tv.ctypes.data, arr, self.Tc.ctypes.data, len(clouds), C.byref(self.P), C.byref(self.I))
        assert rc == 0, rc

    def compare(self, dep, sem):
        rc = self.ctx.lib.ssm_render_compare(self.ctx.h, self.t, dep.ctypes.data, sem.ctypes.data, float(self.ctx.cfg.camera.scale), C.byref(self.P), C.byref(self.J), None)
        assert rc == 0, rc


def step_run(reps):
    import numpy as np
    import semantic_slam_mapping_amd as ssm
    out = {}
    for which in SIZES:
        imgs, vdep, Tv, Tc = scene(which)
        w, h = SIZES[which]
        sem = np.ascontiguousarray(imgs[2])
        ctx = contexts(which)
        cl = clouds_of(ctx, imgs)
        pts = [ctx.cloud_fetch(c).copy() for c in cl]
        for ps in SPLATS[which]:
            call = Call(ctx, which, Tv, Tc, ps)
            res = {"points": len(pts[0]), "render_ms": [], "compare_ms": [], "host_render_ms": [], "host_compare_ms": []}
            for r in range(reps + 3):                          # three untimed passes: the first allocates
                ctx.sync()
                t0 = time.perf_counter()
                call.render(cl)                                # (ends in the call's one wait)
                t1 = time.perf_counter()
                call.compare(vdep, sem)
                t2 = time.perf_counter()
                if r >= 3:
                    res["render_ms"].append((t1 - t0) * 1e3); res["compare_ms"].append((t2 - t1) * 1e3)
            dev = ctx.render_clouds(call.t, CAM[which], Tv, cl, Tc, keys=True, point_size=ps, max_radius=MAX_RADIUS)
            dcounts, dcls = ctx.render_compare(call.t, vdep, sem, CAM[which][4], class_image=True)
            for r in range(3):
                t0 = time.perf_counter()
                host = ssm.render_host(w, h, CAM[which], Tv, pts, Tc, keys=True, point_size=ps, max_radius=MAX_RADIUS)
                t1 = time.perf_counter()
                hcounts, hcls = ssm.render_compare_host(host["depth"], host["label"], vdep, sem, CAM[which][4], class_image=True)
                res["host_render_ms"].append((t1 - t0) * 1e3); res["host_compare_ms"].append((time.perf_counter() - t1) * 1e3)
            assert dev["info"] == host["info"] and all(dev[f].tobytes() == host[f].tobytes() for f in ("keys", "depth", "bgr", "label", "index")), "device != host"
            assert dcounts == hcounts and dcls.tobytes() == hcls.tobytes(), "device comparison != host"
            res["info"] = dev["info"]; res["counts"] = hcounts
            out[f"{which} {ps}"] = res
            ctx.render_target_free(call.t)
        for c in cl:
            ctx.cloud_free(c)
        ctx.close()
    print(json.dumps(out))


def step_trace(reps):
    """what the rocprofv3 run executes: per scene and size, `reps` renderings and comparisons"""
    import numpy as np
    for which in SIZES:
        imgs, vdep, Tv, Tc = scene(which)
        sem = np.ascontiguousarray(imgs[2])
        ctx = contexts(which)
        cl = clouds_of(ctx, imgs)
        for ps in SPLATS[which]:
            call = Call(ctx, which, Tv, Tc, ps)
            for r in range(reps):
                call.render(cl); call.compare(vdep, sem)
            ctx.render_target_free(call.t)
        for c in cl:
            ctx.cloud_free(c)
        ctx.close()
    print(json.dumps({}))


def step_probe(reps):
    """the scenes as files for scripts/render_probe, one run of it each"""
    import numpy as np
    from semantic_slam_mapping_amd.api import _cm16, _render_params
    if not os.path.exists(PROBE):
        build_probe()
    scenes = {}
    for which in SIZES:
        imgs, vdep, Tv, Tc = scene(which)
        ctx = contexts(which)
        cl = clouds_of(ctx, imgs)
        scenes[which] = ([ctx.cloud_fetch(c).copy() for c in cl], Tv, Tc)
        for c in cl:
            ctx.cloud_free(c)
        ctx.close()          # (the probe is a process of its own: this one holds no context while it runs)
    out = {}
    d = tempfile.mkdtemp(prefix="render_probe_")
    for which, (pts, Tv, Tc) in scenes.items():
        w, h = SIZES[which]
        for ps in SPLATS[which]:
            path = os.path.join(d, f"{which}_{ps}.bin")
            with open(path, "wb") as f:
                f.write(struct.pack("<4i", w, h, len(pts), 0)); f.write(np.asarray(CAM[which], np.float64).tobytes()); f.write(_cm16(Tv).tobytes())
                f.write(bytes(_render_params(dict(point_size=ps, max_radius=MAX_RADIUS))))
                for p, T in zip(pts, Tc):
                    f.write(struct.pack("<2i", len(p), 0)); f.write(_cm16(T).tobytes()); f.write(p.tobytes())
            r = subprocess.run(["timeout", "-k", "10", "120", PROBE, path], capture_output=True, text=True)
            if r.returncode != 0:
                raise SystemExit(f"render_probe failed with status {r.returncode}; nothing further is started\n{r.stderr[-2000:]}")
            out[f"{which} {ps}"] = json.loads(r.stdout.strip().splitlines()[-1])
            os.remove(path)
    print(json.dumps(out))


STEPS = {"run": step_run, "trace": step_trace, "probe": step_probe}


def run_step(name, reps, limit, prefix=()):
    cmd = ["timeout", "-k", "10", str(limit), *prefix, sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(reps)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit(f"render_bench: step {name} failed with status {r.returncode}; nothing further is started\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def kernel_split(reps):
    """-> per scene and size {kernel: µs per call (median over the calls)} from one traced run; a call's kernels begin with a render_clear_kernel launch"""
    d = tempfile.mkdtemp(prefix="render_trace_")
    run_step("trace", reps, 420, prefix=("rocprofv3", "--kernel-trace", "-d", d, "-o", "render", "--output-format", "csv", "--"))
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += [(int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3) for r in csv.DictReader(open(f))]
    rows.sort()
    calls = []
    for _, name, us in rows:
        k = next((k for k in KERNELS if k in name), None)
        if k is None:
            continue
        if k == "render_clear_kernel":
            calls.append({})
        if calls:
            calls[-1][k] = calls[-1].get(k, 0.0) + us
    out, at = {}, 0
    for which in SIZES:
        for ps in SPLATS[which]:
            mine, at = calls[at:at + reps], at + reps
            out[f"{which} {ps}"] = {k: statistics.median([c.get(k, 0.0) for c in (mine[1:] or mine)]) for k in KERNELS}          # the first call allocates
    return out


def med(x, fmt="{:.3f}"):
    return fmt.format(statistics.median(x)) + " (" + fmt.format(min(x)) + " – " + fmt.format(max(x)) + ")"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS)); ap.add_argument("--reps", type=int, default=20); ap.add_argument("--build-probe", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_render.md"))
    a = ap.parse_args()
    if a.build_probe:
        return build_probe()
    if a.step:
        return STEPS[a.step](a.reps)
    res = run_step("run", a.reps, 540)
    split = kernel_split(min(a.reps, 8))
    probe = run_step("probe", 1, 300)
    o = ["# r19: map rendering -- z-buffered point splats into a camera view\n",
         f"`python3 scripts/render_bench.py` on one MI355X.  One view against {M} device-resident clouds (`ssm_render_clouds`, then `ssm_render_compare` with the frame's host "
         f"images), max_radius {MAX_RADIUS}; median (min – max) of {a.reps} calls after three untimed passes, wall time of each call in ms (render: the table's upload, clear, "
         "splat, resolve, the info's download, one wait; compare: the upload of the frame's depth and semantic image, the kernel, the counts' download, one wait); the host "
         "functions: 3 passes on one core, through the Python binding.  Device == host functions: keys, the four images, the info, the nine counts and the class image "
         "(asserted by the script).\n",
         "| view | point_size, m | points per cloud | visible / covered pixels | `ssm_render_clouds`, ms | `ssm_render_compare`, ms | `ssm_render_host`, one core, ms | `ssm_render_compare_host`, ms |\n|---|---|---|---|---|---|---|---|"]
    for key, r in res.items():
        which, ps = key.split()
        w, h = SIZES[which]
        o.append(f"| {which} {w} x {h} | {ps} | {r['points']} | {r['info']['n_visible']} / {r['info']['n_covered']} | {med(r['render_ms'])} | {med(r['compare_ms'])} | "
                 f"{med(r['host_render_ms'], '{:.1f}')} | {med(r['host_compare_ms'], '{:.2f}')} |")
    o.append("\n## The kernels (rocprofv3 --kernel-trace, a run of its own; µs per call, median) and the splat kernel's atomics (a probe build with two debug counters, a run of its own)\n")
    o.append("| view, point_size | clear | splat | resolve | compare (+ its counts' clear) | footprint pixels offered | per visible point | atomics issued | per point given | share of the offers the plain load removes |\n|---|---|---|---|---|---|---|---|---|---|")
    for key in res:
        g, p = split[key], probe[key]
        o.append(f"| {key} | {g['render_clear_kernel']:.1f} | {g['render_splat_kernel']:.1f} | {g['render_resolve_kernel']:.1f} | {g['render_compare_kernel'] + g['render_counts_clear_kernel']:.1f} | "
                 f"{p['offered']} | {p['offered'] / max(p['visible'], 1):.2f} | {p['atomics']} | {p['atomics'] / max(p['points'], 1):.3f} | {1 - p['atomics'] / max(p['offered'], 1):.3f} |")
    o.append("\nThe atomics issued depend on the order the waves happen to run in (a later, nearer point finds a larger key and must issue its atomic); the images do not.  "
             "The probe's counters are atomics of their own, so the probe build's times are not quoted.")
    for key in res:
        g, p = split[key], probe[key]
        o.append(f"\n{key}: the splat kernel takes {g['render_splat_kernel']:.1f} µs for {p['points']} points and {p['atomics']} 64-bit integer min atomics: "
                 f"{p['points'] / max(g['render_splat_kernel'], 1e-9):.0f} points and {p['atomics'] / max(g['render_splat_kernel'], 1e-9):.0f} atomics per µs.")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(o) + "\n")
    print("\n".join(o))


if __name__ == "__main__":
    main()
