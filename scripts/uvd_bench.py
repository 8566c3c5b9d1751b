#!/usr/bin/env python3
"""Times the U/V-disparity moving-object stage (ssm_uvd_process_dev, csrc/kernels_uvd.hip) at KITTI size and writes profiles/r13_uvd.md.
Configuration: 1241 x 376, one chunk of 64 pairs, 80 disparities; the pairs are a seeded ground plane with two boxes (tests/uvd_ref.py), warped into a right image,
so that the SGBM stage of the same run (ssm_stereo_seq_process, depth stage only) has real work and its stage time stands beside the three phases.
Usage, from the repository root:  python3 scripts/uvd_bench.py [--reps N] [--parent DIR] [--out FILE]
The driver starts the device step as a process of its own under its own time limit and stops if it fails; then bench.py alternated with the parent commit's
tree (--parent DIR: a built checkout of the parent; left out when not given).  `--step run` runs the device step alone and prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
W, H, N, CAP = 1241, 376, 64, 1000
SGBM_REF_MS = 0.147          # profiles/r06_*: SGBM per pair in the batched stereo path


def step_run(reps):
    import numpy as np
    import semantic_slam_mapping_amd as ssm
    import uvd_ref as R
    lefts, rights, disps, Ms, FLs, NMs = [], [], [], np.zeros((N, CAP), R.PMATCH), np.zeros((N, CAP), np.uint8), np.zeros(N, np.int32)
    rng = np.random.default_rng(0x13)
    for f in range(N):
        left, disp, m, fl = R.make_scene(1000 + f, w=W, h=H, v_h=170, slope=0.38, boxes=((300 + 3 * f, 150, 120, 45), (800 - 2 * f, 200, 150, 30)), outliers_on=(0, 1), n_out=10,
                                         inliers_on=(1,) if f % 8 == 7 else (), n_in=5, n_ground_inliers=40, holes=60, zero_pixels=500)
        right = rng.integers(0, 256, (H, W)).astype(np.uint8)
        d = np.maximum(disp.astype(np.int32), 0) // 16
        for r in range(H):
            xr = np.arange(W) - d[r]; ok = xr >= 0
            right[r, xr[ok]] = left[r, ok]
        lefts.append(left); rights.append(right); disps.append(disp)
        Ms[f, :len(m)] = m; FLs[f, :len(m)] = fl; NMs[f] = len(m)
    P = R.scene_params(f=718.856, cu=607.1928, cv=170.0, base=0.54, roi_x=20.0, roi_y=5.0, roi_z=40.0)
    ctx = ssm.Context(0, width=W, height=H, orb_features=1000, max_batch=32, voxel_capacity_log2=12, stereo_batch=N)
    px = W * H
    d_left, d_right, d_disp = ctx.dev_alloc(N * px), ctx.dev_alloc(N * px), ctx.dev_alloc(N * px * 2)
    ctx.h2d(d_left, np.stack(lefts)); ctx.h2d(d_right, np.stack(rights)); ctx.h2d(d_disp, np.stack(disps))
    u = ssm.UVDisparity(ctx, **P)
    ctx.set_profiling(2)
    res = {"e2e_ms": [], "host1_ms": [], "host2_ms": [], "stages": []}
    for r in range(reps + 1):                         # the first pass allocates
        u.reset()
        ctx.stereo_seq_process(d_left, d_right, N, W, H, stages=ssm.api.STEREO_DEPTH, baseline=0.54, cu=607.1928, cv=170.0, f=718.856, roix=20.0, roiy=5.0, roiz=40.0, scale=1000.0)
        ctx.sync()
        t0 = time.perf_counter()
        info, _, _ = u.process_dev(d_left, d_disp, N, W, H, Ms, NMs, FLs)
        e2e = (time.perf_counter() - t0) * 1e3
        st = ctx.stage_times()                       # name -> (ms, launches) since the stereo call began
        if r:
            h1, h2, _ = u.times()
            res["e2e_ms"].append(e2e); res["host1_ms"].append(h1); res["host2_ms"].append(h2); res["stages"].append({k: v[0] for k, v in st.items()})
    with_mask = int(((info["n_masks_kept"] > 0) & (info["n_moving"] > 0)).sum())
    assert with_mask >= N * 3 // 4, f"only {with_mask} of {N} pairs keep a mask: the segment phase and the union upload would be measured on their no-mask path"
    res.update(pairs_with_mask=with_mask, matches=int(NMs.sum()), status_ok=int((info["status"] == 0).sum()), masks_kept=int(info["n_masks_kept"].sum()), moving=int(info["n_moving"].sum()), seeds=int(info["n_seeds"].sum()),
               u_rows=int(info["u_rows"].max()))
    u.close(); ctx.close()
    print(json.dumps(res))


def run_step(reps, limit=540):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", "run", "--reps", str(reps)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit(f"uvd_bench: the device step failed with status {r.returncode}; nothing further is started\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def bench_line(tree, limit=900):
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "bench.py"], capture_output=True, text=True, cwd=tree)
    if r.returncode != 0:
        raise SystemExit(f"uvd_bench: bench.py in {tree} failed with status {r.returncode}\n{r.stderr[-3000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def rng_of(x, fmt="{:.3f}"):
    return fmt.format(min(x)) + " – " + fmt.format(max(x))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["run"]); ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: bench.py runs there and here in alternation")
    ap.add_argument("--bench-rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_uvd.md"))
    a = ap.parse_args()
    if a.step:
        return step_run(a.reps)
    res = run_step(a.reps)
    bench = {"parent": [], "new": []}
    if a.parent:
        for _ in range(a.bench_rounds):
            for who, tree in (("parent", a.parent), ("new", ROOT)):
                bench[who].append(bench_line(tree))
    per = lambda xs: [x / N for x in xs]
    o = []
    o.append("# r13: the U/V-disparity moving-object stage at KITTI size\n")
    o.append(f"`python3 scripts/uvd_bench.py` on one MI355X.  {W} x {H}, one chunk of {N} pairs (seeded ground plane + two boxes, 80 disparities, 60 - 65 matches per pair, 20 of them outliers on the boxes); "
             f"{a.reps} timed repetitions after one untimed pass; ranges are min – max over the repetitions; all times in ms PER PAIR (chunk time / {N}).  "
             "Device times are hipEvent stage times (`ssm_get_stage_times`, profiling mode 2); host steps are wall time inside the call (`ssm_debug_uvd_times`); "
             "end to end is the wall time of `ssm_uvd_process_dev` (three waits).\n")
    o.append("| part | ms per pair (min – max) |\n|---|---|")
    for key, label in (("uvd_vdisp", "device phase 1: `uvd_vdisp_kernel`"), ("uvd_classify", "device phase 2: `uvd_classify_kernel` + `uvd_probe_kernel`"), ("uvd_segment", "device phase 3: `uvd_segment_kernel`")):
        o.append(f"| {label} | {rng_of(per([s.get(key, 0.0) for s in res['stages']]), '{:.4f}')} |")
    dev = [sum(s.get(k, 0.0) for k in ("uvd_vdisp", "uvd_classify", "uvd_segment")) for s in res["stages"]]
    o.append(f"| the three device phases together | {rng_of(per(dev), '{:.4f}')} |")
    o.append(f"| host step 1 (lines, pitch, Kalman) | {rng_of(per(res['host1_ms']), '{:.4f}')} |")
    o.append(f"| host step 2 (filterInOut, seeds, fills, merge, verify) | {rng_of(per(res['host2_ms']), '{:.4f}')} |")
    o.append(f"| end to end (`ssm_uvd_process_dev`, copies and three waits included) | {rng_of(per(res['e2e_ms']), '{:.4f}')} |")
    sg = [s.get("sgbm", 0.0) for s in res["stages"]]
    o.append(f"| SGBM stage of the same run (`ssm_stereo_seq_process`, depth stage) | {rng_of(per(sg), '{:.4f}')} |")
    o.append(f"\nThe scenes: {res['status_ok']} of {N} pairs with a ground line, {res['matches']} matches, {res['seeds']} flood fills, {res['pairs_with_mask']} of {N} pairs keep a mask (asserted: at least three quarters, so that `uvd_segment_kernel` and the union upload do their work), {res['masks_kept']} masks kept, {res['moving']} moving pixels, u_rows up to {res['u_rows']}.\n")
    msg = sum(sg) / len(sg) / N if sg and sum(sg) > 0 else SGBM_REF_MS
    mdev, mh, me = sum(dev) / len(dev) / N, (sum(res["host1_ms"]) + sum(res["host2_ms"])) / len(res["e2e_ms"]) / N, sum(res["e2e_ms"]) / len(res["e2e_ms"]) / N
    o.append("## Against SGBM\n")
    o.append(f"SGBM costs {msg:.3f} ms per pair in this run (profiles/r06_*: {SGBM_REF_MS} ms).  The three device phases take {mdev:.4f} ms per pair = {100 * mdev / msg:.0f} % of it; "
             f"the two host steps {mh:.4f} ms = {100 * mh / msg:.0f} %; the whole call {me:.4f} ms = {100 * me / msg:.0f} %.  "
             f"The expectation was that the device phases are a small fraction of SGBM and that the host steps and the three waits dominate the call: "
             f"device phases / call = {100 * mdev / me:.0f} %, host steps / call = {100 * mh / me:.0f} %, the remainder (copies, waits, launch gaps) = {100 * (me - mdev - mh) / me:.0f} %.\n")
    if a.parent:
        o.append("## `python bench.py` (default line), parent commit and this tree alternated in one call\n")
        o.append("| tree | " + " | ".join(f"run {i + 1}" for i in range(a.bench_rounds)) + " | range |\n|---|" + "---|" * (a.bench_rounds + 1))
        for who in ("parent", "new"):
            vals = [b.get("value") for b in bench[who]]
            o.append(f"| {who} | " + " | ".join(f"{x:.1f}" for x in vals) + f" | {rng_of(vals, '{:.1f}')} |")
        o.append(f"\n(`{bench['new'][0].get('metric', 'value')}`, {bench['new'][0].get('unit', '')}; the stage is off by default and no existing kernel changed.)\n")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(o) + "\n")
    print("\n".join(o))


if __name__ == "__main__":
    main()
