#!/usr/bin/env python3
"""Times vocabulary training (ssm_vocab_train: csrc/kernels_vocab_train.hip, csrc/ssm_vocab_train.hip) against the host function on one core and writes
profiles/r15_vocab_train.md.  Input: 1000 frames x 1000 seeded random descriptors, k = 10, L = 5, max_iters = 32; median of --reps runs each (default 5) after
one device warm-up; the device's per-level wall times come from ssm_debug_vocab_train_times.  Device and host results are compared byte for byte.
Usage, from the repository root:  python3 scripts/vocab_train_bench.py [--reps N] [--frames F] [--per-frame N] [--out FILE]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K, L, ITERS = 10, 5, 32
RESOURCES = "vt_seed_kernel 32 VGPRs, vt_count_kernel 16 VGPRs + 30800 B LDS, vt_assign_kernel 28 VGPRs, the others <= 11 VGPRs; ScratchSize 0 in all of them"


def main():
    import numpy as np
    import semantic_slam_mapping_amd as ssm
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5); ap.add_argument("--frames", type=int, default=1000); ap.add_argument("--per-frame", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_vocab_train.md"))
    a = ap.parse_args()
    rng = np.random.default_rng(0xB0C5)
    sets = list(rng.integers(0, 256, size=(a.frames, a.per_frame, 32), dtype=np.uint8))
    ctx = ssm.Context(0, orb_features=1000, max_batch=1, voxel_capacity_log2=16)
    lib = ctx.lib

    def device():
        t = time.perf_counter(); v = ssm.Vocabulary.train(sets, K, L, ITERS, ctx=ctx); dt = time.perf_counter() - t
        lv = (C.c_double * 10)(); tot = C.c_double(0)
        ctx._chk(lib.ssm_debug_vocab_train_times(ctx.h, C.byref(lv), C.byref(tot)))
        return dt * 1e3, [float(x) for x in lv], tot.value, v

    def host():
        t = time.perf_counter(); v = ssm.Vocabulary.train(sets, K, L, ITERS); dt = time.perf_counter() - t
        return dt * 1e3, v

    device()[3].close()                                                     # warm-up: code objects, first allocations
    dev_ms, dev_lv, dev_in = [], [], []
    for _ in range(a.reps):
        ms, lv, tot, vd = device()
        dev_ms.append(ms); dev_lv.append(lv); dev_in.append(tot)
        if _ < a.reps - 1:
            vd.close()
    host_ms = []
    for _ in range(a.reps):
        ms, vh = host()
        host_ms.append(ms)
        print(f"host run {_}: {ms:.0f} ms", flush=True)
        if _ < a.reps - 1:
            vh.close()
    same = vd.report == vh.report and all(x.tobytes() == y.tobytes() for x, y in zip(vd.arrays(), vh.arrays())) and vd.word_of_feature.tobytes() == vh.word_of_feature.tobytes()
    med = statistics.median
    rep = vd.report
    o = ["# Vocabulary training: device against the host function on one core", "",
         f"{a.frames} frames x {a.per_frame} seeded random descriptors (N = {a.frames * a.per_frame}), k = {K}, L = {L}, max_iters = {ITERS}; median (min - max) of {a.reps} runs, wall time of the",
         "call in ms as Python sees it (the device call includes the upload of the descriptors, every per-level read-back and the host's weight pass; one warm-up",
         f"run before).  Device and host results byte for byte equal: **{same}**.  Tree: {rep['nodes']} nodes, {rep['words']} words, {rep['levels']} levels, {rep['capped_nodes']} capped nodes,",
         f"passes per level {rep['passes'][:L]}.", "",
         "| path | ms | device / host |", "|---|---|---|",
         f"| device (`ssm_vocab_train`) | {med(dev_ms):.1f} ({min(dev_ms):.1f} - {max(dev_ms):.1f}) | {med(dev_ms) / med(host_ms):.3f} |",
         f"| host (`ssm_vocab_train_host`, one core) | {med(host_ms):.1f} ({min(host_ms):.1f} - {max(host_ms):.1f}) | 1 |", "",
         "Device wall time per level (seeding, passes, partition and the read-backs of the level the nodes of which are being split), median over the runs, ms:", "",
         "| level | " + " | ".join(str(l) for l in range(L)) + " | inside the call |", "|---|" + "---|" * (L + 1),
         "| ms | " + " | ".join(f"{med([lv[l] for lv in dev_lv]):.1f}" for l in range(L)) + f" | {med(dev_in):.1f} |",
         "| passes | " + " | ".join(str(rep["passes"][l]) for l in range(L)) + " | |", "",
         f"Kernel resource usage (-Rpass-analysis=kernel-resource-usage, gfx950): {RESOURCES}."]
    with open(a.out, "w") as f:
        f.write("\n".join(o) + "\n")
    print(open(a.out).read())
    ctx.close()


if __name__ == "__main__":
    main()
