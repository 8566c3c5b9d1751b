#!/usr/bin/env python3
"""Times the pose-graph optimiser (ssm_pgo_optimize, csrc/kernels_pgo.hip) against its host function (ssm_pgo_optimize_host) on the same machine and writes
profiles/r14_pgo.md.  Graphs (tests/pgo_ref.py's circle scenes): 1000 key-frames with nearby = 5 and 20 loop edges; 200 key-frames (nearby 5, 4 loop edges);
sixteen such 200-vertex graphs through ssm_pgo_optimize_many.  Each measurement is optimize(10) from the same start poses: 3 warm-up runs, then the median and
the range of --reps (>= 20) runs; the device run's phase split comes from ssm_pgo_times (100 MHz stamps written by the block).  Device and host results are
compared bit for bit on the way.  The kernel's registers / spills / scratch come from hipcc's -Rpass-analysis=kernel-resource-usage when hipcc is there.
Usage, from the repository root:  python3 scripts/pgo_bench.py [--reps N] [--out FILE]"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
PHASES = ("linearise", "assemble", "factor + solves", "update + chi2", "decide")


def make(n, n_loops, seed):
    import pgo_ref as R
    loops = tuple((n - 1 - 7 * k, 1 + 11 * k, 0.05, 0.01) for k in range(n_loops))
    return R.make_scene(seed=seed, n=n, drift=0.01, noise_t=0.05, noise_r=0.01, nearby=5, loops=loops)


def build(ssm, ctx, sc):
    g = ssm.PoseGraphOptimizer(ctx)
    for k, T in enumerate(sc["poses"]):
        g.add_vertex(k, T)
    for (i, j), Z in zip(sc["edges"], sc["Z"]):
        g.add_edge(int(i), int(j), Z)
    g.set_mode(False)
    return g


def restore(g, sc):
    for k, T in enumerate(sc["poses"]):
        g.set_pose(k, T)


def timed(fn, prepare, reps):
    out = []
    for r in range(reps + 3):
        prepare()
        t0 = time.perf_counter()
        res = fn()
        dt = (time.perf_counter() - t0) * 1e3
        if r >= 3:
            out.append(dt)
        if r % 5 == 0:
            print(f"  run {r}: {dt:.1f} ms", flush=True)
    return out, res


def fmt(ms):
    return f"{statistics.median(ms):.2f} ({min(ms):.2f} - {max(ms):.2f})"


def resource_usage():
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    csrc = os.path.join(ROOT, "semantic_slam_mapping_amd", "csrc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-c", os.path.join(csrc, "kernels_pgo.hip"), "-o", os.devnull], capture_output=True, text=True, timeout=600)
    return dict(re.findall(r"remark:\s+(VGPRs|AGPRs|VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\d+)", r.stderr)) if r.returncode == 0 else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_pgo.md"))
    a = ap.parse_args()
    assert a.reps >= 20, "the note reports the median of at least 20 runs"
    import numpy as np
    import semantic_slam_mapping_amd as ssm
    ctx = ssm.Context(0, orb_features=1000, max_batch=2, voxel_capacity_log2=12)
    rows, notes = [], []
    for label, n, loops in (("1000 key-frames, nearby 5, 20 loop edges", 1000, 20), ("200 key-frames, nearby 5, 4 loop edges", 200, 4)):
        sc = make(n, loops, 0x14)
        d, h = build(ssm, ctx, sc), build(ssm, None, sc)
        print(label, flush=True)
        td, rd = timed(lambda: d.optimize(10), lambda: restore(d, sc), a.reps)
        phases = d.times()
        th, rh = timed(lambda: h.optimize_host(10), lambda: restore(h, sc), a.reps)
        same = d.poses()[1].tobytes() == h.poses()[1].tobytes() and all(np.asarray(rd[f]).tobytes() == np.asarray(rh[f]).tobytes() for f in ("trials", "accepted", "chi2_after", "lambda"))
        assert same, "device and host differ"
        rows.append((label, len(sc["edges"]), int(rd["envelope_scalars"]), int(rd["iterations"]), int(sum(rd["trials"])), fmt(td), fmt(th), statistics.median(td) / statistics.median(th)))
        notes.append((label, phases))
        d.close(); h.close()
    scs = [make(200, 4, 0x20 + k) for k in range(16)]
    ds, hs = [build(ssm, ctx, sc) for sc in scs], [build(ssm, None, sc) for sc in scs]
    tm, rm = timed(lambda: ssm.PoseGraphOptimizer.optimize_many(ds, 10), lambda: [restore(g, sc) for g, sc in zip(ds, scs)], a.reps)
    th, _ = timed(lambda: [g.optimize_host(10) for g in hs], lambda: [restore(g, sc) for g, sc in zip(hs, scs)], a.reps)
    assert all(g.poses()[1].tobytes() == q.poses()[1].tobytes() for g, q in zip(ds, hs)), "device and host differ"
    rows.append(("16 x 200 key-frames, one launch", sum(len(sc["edges"]) for sc in scs), int(sum(rm["envelope_scalars"])), int(max(rm["iterations"])), int(rm["trials"].sum()), fmt(tm), fmt(th),
                 statistics.median(tm) / statistics.median(th)))
    for g in ds + hs:
        g.close()
    ctx.close()
    ru = resource_usage()
    with open(a.out, "w") as f:
        f.write("# Pose-graph optimiser: device (one 1024-thread block per graph) against the host function\n\n")
        f.write(f"optimize(10) from the same start poses; median (min - max) of {a.reps} runs after 3 warm-ups, wall time of the call in ms (upload, launch, one wait, download).\n")
        f.write("Device and host results were compared bit for bit in every run's last repetition.  The host function runs on one core of the same machine.\n\n")
        f.write("| graph | edges | envelope scalars | iterations | trials | device ms | host ms | device / host |\n|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r[0]} | {r[1]} | {r[2]} | {r[3]} | {r[4]} | {r[5]} | {r[6]} | {r[7]:.2f} |\n")
        f.write("\nPhase split of the last device run (ssm_pgo_times, ms inside the block; the chi2 at the start of an iteration is not stamped):\n\n")
        f.write("| graph | " + " | ".join(PHASES) + " |\n|---|" + "---|" * len(PHASES) + "\n")
        for label, ph in notes:
            f.write(f"| {label} | " + " | ".join(f"{x:.3f}" for x in ph) + " |\n")
        f.write("\nKernel resource usage (`pgo_kernel`, -Rpass-analysis=kernel-resource-usage): " + (", ".join(f"{k} {v}" for k, v in ru.items()) if ru else "hipcc not available where this ran") + ".\n")
    print(open(a.out).read())


if __name__ == "__main__":
    main()
