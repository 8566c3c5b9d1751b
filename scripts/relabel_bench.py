#!/usr/bin/env python3
"""Times label fusion (ssm_relabel, csrc/kernels_relabel.hip) at the pipeline's shape -- one device-resident cloud against 10 views -- and writes
profiles/r22_relabel.md.  Scenes: those of scripts/sor_bench.py (frame 0 of the bench's synthetic stream at 640 x 480, the stereo-style road scene at 1241 x 376);
the ten views are that frame seen from ten poses a few centimetres apart, their label images the frame's with 3 % of the pixels relabelled at random; a fifth of the
cloud's own 8 x 8 label blocks are wrong.  Each
scene runs in three forms: a depth and a label image per view, one packed word per pixel, and the packed form with two views in flight.  Per form: the kernel's time (a second run of the same calls, a process of its own under
rocprofv3 --kernel-trace), the call's wall time, and once the host function on one core with the labels compared.  Median of --reps calls, each on a fresh cloud.
Usage, from the repository root:  python3 scripts/relabel_bench.py [--reps N] [--out FILE]
No hardware counters are collected."""
import argparse
import csv
import glob
import os
import subprocess
import tempfile
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from sor_bench import SIZES, CAM, frame, contexts  # noqa: E402

V = 10
FORMS = {0: "two images", 1: "packed", 2: "packed, two views in flight"}


def scene(which):
    import numpy as np
    import semantic_slam_mapping_amd as ssm
    dep, bgr, sem = frame(which)
    rng = np.random.default_rng(22)
    pal = np.array([[128, 128, 128], [0, 0, 128], [128, 192, 192], [0, 69, 255], [128, 64, 128], [222, 40, 60], [0, 128, 128], [128, 128, 192], [128, 64, 64], [128, 0, 64],
                    [0, 64, 64], [192, 128, 0]], np.uint8)
    sems, poses = [], []
    for k in range(V):
        s = sem.copy()
        noise = rng.random(dep.shape) < 0.03
        s[noise] = pal[rng.integers(0, 12, int(noise.sum()))]
        sems.append(s)
        T = np.eye(4)
        T[0, 3] = 0.02 * (k - V // 2); T[2, 3] = 0.01 * (k - V // 2)
        poses.append(T)
    # the cloud's own semantic image: a fifth of its 8 x 8 blocks are painted one of five classes the back-projection neither gates nor masks, so labels change
    own = sem.copy()
    h, w = dep.shape
    keep = pal[[1, 4, 5, 6, 8]]
    for by in range(0, h - 7, 8):
        for bx in range(0, w - 7, 8):
            if rng.random() < 0.2:
                own[by:by + 8, bx:bx + 8] = keep[int(rng.integers(0, 5))]
    return dep, bgr, own, sems, poses, [ssm.relabel_labels_host(s) for s in sems]


def run(reps):
    import numpy as np
    import semantic_slam_mapping_amd as ssm
    out = {}
    for which in SIZES:
        dep, bgr, sem, sems, poses, labs = scene(which)
        ctx = contexts(which)
        Tc = np.eye(4)
        res = {}
        for form in FORMS:
            ctx.relabel_form(form)
            views = [ctx.relabel_view(dep, s, CAM[which]) for s in sems]
            wall = []
            for r in range(reps + 1):                          # the first pass allocates
                cl = ctx.backproject_dev(dep, bgr, sem)
                if r == reps:
                    before = ctx.cloud_fetch(cl).copy()
                t0 = time.perf_counter()
                info = ctx.relabel(views, poses, cl, Tc)
                wall.append((time.perf_counter() - t0) * 1e3)
                if r == reps:
                    after = ctx.cloud_fetch(cl).copy()
                ctx.cloud_free(cl)
            for v in views:
                ctx.relabel_view_free(v)
            t0 = time.perf_counter()
            hl, _, hinfo = ssm.relabel_host([(dep, l, CAM[which]) for l in labs], poses, before, Tc)
            host_ms = (time.perf_counter() - t0) * 1e3
            assert np.array_equal(after["label"], hl) and info == hinfo, (which, form)
            res[form] = dict(wall_ms=statistics.median(wall[1:]), host_ms=host_ms, info=info)
        ctx.relabel_form(-1)
        ctx.close()
        out[which] = res
    return out


def kernel_times(reps):
    """-> {(scene, form): median kernel time in ms} from one traced run of `run`: per scene and form, reps + 1 launches of relabel_kernel in order"""
    d = tempfile.mkdtemp(prefix="relabel_trace_")
    cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "-d", d, "-o", "relabel", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--reps", str(reps), "--traced"]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += [(int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6) for r in csv.DictReader(open(f)) if "relabel_kernel" in r["Kernel_Name"]]
    rows.sort()
    assert len(rows) == len(SIZES) * len(FORMS) * (reps + 1), len(rows)
    out, at = {}, 0
    for which in SIZES:
        for form in FORMS:
            out[(which, form)] = statistics.median([ms for _, ms in rows[at + 1:at + reps + 1]])
            at += reps + 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_relabel.md"))
    ap.add_argument("--traced", action="store_true", help="only make the calls (what the rocprofv3 run executes)")
    a = ap.parse_args()
    res = run(a.reps)
    if a.traced:
        return
    kern = kernel_times(a.reps)
    lines = ["# Label fusion: one cloud against 10 views (scripts/relabel_bench.py)", "",
             f"MI355X, median of {a.reps} calls after one that allocates, each on a fresh device cloud; defaults (radius 1, edge guard on).  `kernel` is relabel_kernel's",
             "time in a rocprofv3 kernel trace of the same calls (a run of its own), `call` the wall time of ssm_relabel (launch, info download, one wait), `host` ssm_relabel_host on one core, once.",
             "The device labels and info equal the host's in every row.  No hardware counters were collected; the label images are the synthetic scene's with 3 % noise,",
             "not SegNet output, and the depth is synthetic.", "",
             "| scene | points | form | kernel ms | call ms | host ms | changed | pairs supported |", "|---|---|---|---|---|---|---|---|"]
    for which, r in res.items():
        w, h = SIZES[which]
        for form, x in r.items():
            lines.append(f"| {w} x {h} | {x['info']['n_in']} | {FORMS[form]} | {kern[(which, form)]:.3f} | {x['wall_ms']:.3f} | {x['host_ms']:.1f} | {x['info']['n_changed']} | {x['info']['pairs_supported']} |")
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
