#!/usr/bin/env python3
"""Times the device looper (ssm_looper_*, csrc/kernels_bow.hip) at loop-closure scale and writes profiles/r12_looper.md.
Configuration: the generated k = 10, L = 6 vocabulary (1 111 111 nodes, 35.6 MB of descriptor rows: fits the 256 MiB Infinity Cache, not an XCD's L2),
1000 key-frames x 1000 descriptors.  Usage, from the repository root:  python3 scripts/looper_bench.py [--reps N] [--parent DIR] [--out FILE]
The driver starts every device step as a process of its own under its own time limit and stops at the first step that fails:
  add (both descent kernels) -> query -> kernel trace (rocprofv3 --kernel-trace --stats, a run of its own) -> host path on one core
  -> bench.py alternated with the parent commit's tree (--parent DIR: a built checkout of the parent; left out when not given).
Steps print one JSON line; `--step NAME` runs one of them."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
K, L, FRAMES, NDESC = 10, 6, 1000, 1000
GATHER_TBS = 8.6          # the microarchitecture guide's chip-wide rate for rows gathered at random from a 38 MB (Infinity-Cache-resident) table


def _setup():
    import numpy as np
    import semantic_slam_mapping_amd as ssm
    import looper_ref as R
    arrays = R.make_vocab(K, L, 0x0B0C, dbow_order=False)
    v = ssm.Vocabulary.from_arrays(*arrays)
    rng = np.random.default_rng(0xBE7C)
    desc = rng.integers(0, 256, size=(FRAMES, 1024, 32), dtype=np.uint8)
    back = 700                                                              # frames 800, 810, .. revisit frame f - 700 (half of its descriptors)
    for f in range(800, FRAMES, 10):
        keep = rng.permutation(NDESC)[:NDESC // 2]
        desc[f, keep] = desc[f - back, keep]
    return np, ssm, v, desc


def step_add(reps):
    """the synchronised bulk add of 1000 frames from device descriptors, per descent kernel (SSM_BOW_VARIANT is read when the looper is created)"""
    np, ssm, v, desc = _setup()
    ctx = ssm.Context(0, orb_features=1000, max_batch=1, voxel_capacity_log2=16)
    assert ctx.cap == 1024
    d_desc = ctx.dev_alloc(desc.nbytes); ctx.h2d(d_desc, desc)
    nkp = np.full(FRAMES, NDESC, np.int32); d_nkp = ctx.dev_alloc(nkp.nbytes); ctx.h2d(d_nkp, nkp)
    out = ssm.api.SeqOutDev(); out.desc = d_desc; out.nkp = d_nkp; out.cap = ctx.cap
    res = {}
    for variant in (0, 1):
        os.environ["SSM_BOW_VARIANT"] = str(variant)
        lp = ssm.Looper(ctx, v)
        times = []
        for r in range(reps + 1):                                           # the first pass allocates (staging, database growth)
            lp.clear(); ctx.sync()
            t0 = time.perf_counter()
            lp.add_dev(out, FRAMES, np.arange(FRAMES)); ctx.sync()
            times.append(time.perf_counter() - t0)
        res[f"add_ms_variant{variant}"] = [t * 1e3 for t in times[1:]]
        res[f"vec0_variant{variant}"] = [int(x) for x in lp.bow(0)[0][:4]]
        res["nnz"] = int(sum(len(lp.bow(e)[0]) for e in (0, 499, 999)))
        lp.close()
    os.environ.pop("SSM_BOW_VARIANT", None)
    print(json.dumps(res))


def step_query(reps):
    """the full lower-triangle query (against = -1) of the 1000 entries: scores of 500 500 pairs + the ordered candidate list, one synchronised call"""
    np, ssm, v, desc = _setup()
    ctx = ssm.Context(0, orb_features=1000, max_batch=1, voxel_capacity_log2=16)
    d_desc = ctx.dev_alloc(desc.nbytes); ctx.h2d(d_desc, desc)
    nkp = np.full(FRAMES, NDESC, np.int32); d_nkp = ctx.dev_alloc(nkp.nbytes); ctx.h2d(d_nkp, nkp)
    out = ssm.api.SeqOutDev(); out.desc = d_desc; out.nkp = d_nkp; out.cap = ctx.cap
    lp = ssm.Looper(ctx, v)
    lp.add_dev(out, FRAMES, np.arange(FRAMES)); ctx.sync()
    times = []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        pairs, sc = lp.query(0, FRAMES, 0.1, 60, cap=65536)
        times.append(time.perf_counter() - t0)
    want = [(f, f - 700) for f in range(800, FRAMES, 10)]
    print(json.dumps({"query_ms": [t * 1e3 for t in times[1:]], "candidates": len(pairs), "planted_found": [tuple(p) for p in pairs.tolist()] == want,
                      "score_min": float(sc.min()) if len(sc) else None, "score_max": float(sc.max()) if len(sc) else None}))


def step_trace(reps):
    """what the rocprofv3 run executes: one add per descent kernel and one query"""
    np, ssm, v, desc = _setup()
    ctx = ssm.Context(0, orb_features=1000, max_batch=1, voxel_capacity_log2=16)
    d_desc = ctx.dev_alloc(desc.nbytes); ctx.h2d(d_desc, desc)
    nkp = np.full(FRAMES, NDESC, np.int32); d_nkp = ctx.dev_alloc(nkp.nbytes); ctx.h2d(d_nkp, nkp)
    out = ssm.api.SeqOutDev(); out.desc = d_desc; out.nkp = d_nkp; out.cap = ctx.cap
    for variant in (1, 0):
        os.environ["SSM_BOW_VARIANT"] = str(variant)
        lp = ssm.Looper(ctx, v)
        for r in range(3):
            lp.clear(); lp.add_dev(out, FRAMES, np.arange(FRAMES)); ctx.sync()
        if variant == 0:
            for r in range(3):
                lp.query(0, FRAMES, 0.1, 60, cap=65536)
        lp.close()
    print(json.dumps({"ok": True}))


def step_host(reps):
    """the host path on one core: vocab.transform of 100 of the frames, vocab.score of 20 000 of the pairs (scaled to the whole job)"""
    np, ssm, v, desc = _setup()
    t0 = time.perf_counter()
    vecs = [v.transform(desc[f, :NDESC])[1:] for f in range(100)]
    t_tr = (time.perf_counter() - t0) / 100
    import ctypes as C
    lib = ssm.load(); s = C.c_double(0)
    t0 = time.perf_counter(); n = 0
    for q in range(100):
        for e in range(100):
            a, b = vecs[q], vecs[e]
            lib.ssm_bow_score_host(a[0].ctypes.data, a[1].ctypes.data, len(a[0]), b[0].ctypes.data, b[1].ctypes.data, len(b[0]), C.byref(s)); n += 1
    t_sc = (time.perf_counter() - t0) / n
    print(json.dumps({"host_transform_ms_per_frame": t_tr * 1e3, "host_score_us_per_pair": t_sc * 1e6, "host_query_ms_500500_pairs": t_sc * 500500 * 1e3}))


STEPS = {"add": step_add, "query": step_query, "trace": step_trace, "host": step_host}


def run_step(name, reps, limit, prefix=()):
    cmd = ["timeout", "-k", "10", str(limit), *prefix, sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(reps)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit(f"looper_bench: step {name} failed with status {r.returncode}; nothing further is started\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}")
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    return json.loads(lines[-1])


def kernel_stats(reps):
    d = tempfile.mkdtemp(prefix="looper_trace_")
    run_step("trace", reps, 420, prefix=("rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "looper", "--output-format", "csv", "--"))
    per = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "bow_" in r["Kernel_Name"]:
                name = r["Kernel_Name"].split("(")[0].split()[-1].replace(".kd", "")
                per.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: (len(v), sum(v) / len(v), min(v), max(v)) for k, v in per.items()}


def bench_line(tree, limit=900):
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "bench.py"], capture_output=True, text=True, cwd=tree)
    if r.returncode != 0:
        raise SystemExit(f"looper_bench: bench.py in {tree} failed with status {r.returncode}\n{r.stderr[-3000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def rng_of(x):
    return f"{min(x):.2f} – {max(x):.2f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS)); ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: bench.py runs there and here in alternation")
    ap.add_argument("--bench-rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_looper.md"))
    a = ap.parse_args()
    if a.step:
        return STEPS[a.step](a.reps)
    add = run_step("add", a.reps, 420)
    qry = run_step("query", a.reps, 420)
    ks = kernel_stats(a.reps)
    host = run_step("host", a.reps, 420)
    bench = {"parent": [], "new": []}
    if a.parent:
        for _ in range(a.bench_rounds):
            for who, tree in (("parent", a.parent), ("new", ROOT)):
                bench[who].append(bench_line(tree))
    levels_bytes = L * K * 32                                                # bytes the descent of one descriptor needs
    total = FRAMES * NDESC * levels_bytes
    o = []
    o.append("# r12: the device looper at loop-closure scale\n")
    o.append(f"`python3 scripts/looper_bench.py` on one MI355X.  Vocabulary: generated k = {K}, L = {L} tree ({sum(K ** l for l in range(L + 1)):,} nodes, "
             f"{sum(K ** l for l in range(L + 1)) * 32 / 1e6:.1f} MB of descriptor rows); {FRAMES} key-frames x {NDESC} descriptors; {a.reps} timed repetitions per figure "
             "after one untimed pass; ranges are min – max over the repetitions.  Every device step ran as its own process under its own time limit.\n")
    o.append("## Synchronised calls (wall time of the call + `ssm_sync`)\n")
    o.append("| call | ms (min – max) | per frame / pair |\n|---|---|---|")
    for var, nm in ((0, "16 lanes per descriptor (default)"), (1, "one lane per descriptor (`SSM_BOW_VARIANT=1`)")):
        t = add[f"add_ms_variant{var}"]
        o.append(f"| `ssm_looper_add_dev`, {FRAMES} frames, descent with {nm} | {rng_of(t)} | {min(t) * 1e3 / FRAMES:.2f} – {max(t) * 1e3 / FRAMES:.2f} µs per frame |")
    t = qry["query_ms"]
    o.append(f"| `ssm_looper_query`, first = 0, n = {FRAMES}, against = -1 (500 500 pairs) | {rng_of(t)} | {min(t) * 1e6 / 500500:.1f} – {max(t) * 1e6 / 500500:.1f} ns per pair |")
    o.append(f"\nThe query returned {qry['candidates']} candidates at (0.1, 60), scores {qry['score_min']:.3f} – {qry['score_max']:.3f}; they are exactly the planted revisits: {qry['planted_found']}.  "
             f"Both descent kernels produced the same first vector ({add['vec0_variant0'] == add['vec0_variant1']}).\n")
    o.append("## Kernels (`rocprofv3 --kernel-trace --stats`, a run of its own: three adds per descent kernel, three queries)\n")
    o.append("| kernel | calls | average µs | min µs | max µs |\n|---|---|---|---|---|")
    for k in sorted(ks):
        c, av, mn, mx = ks[k]
        o.append(f"| `{k}` | {c} | {av:.1f} | {mn:.1f} | {mx:.1f} |")
    o.append("\n## The descent against the gather rate\n")
    o.append(f"One descriptor reads {L} sibling groups of {K} rows of 32 B: {levels_bytes} B; the whole add {total / 1e9:.2f} GB.  "
             f"The microarchitecture guide gives {GATHER_TBS} TB/s chip-wide for rows gathered at random from a 38 MB (Infinity-Cache-resident) table.\n")
    o.append("| descent kernel | average µs | bytes needed / time | share of the gather rate |\n|---|---|---|---|")
    for k in ("bow_words_sg_kernel", "bow_words_lane_kernel"):
        if k in ks:
            tb = total / (ks[k][1] * 1e-6) / 1e12
            o.append(f"| `{k}` | {ks[k][1]:.1f} | {tb:.2f} TB/s | {100 * tb / GATHER_TBS:.0f} % |")
    o.append("\nThe upper two levels (111 rows) are shared by every descriptor and are served from L2 / L1; levels 3 – 6 are the random gathers the rate above "
             "applies to (4 of the 6 groups, two thirds of the bytes).  See the note at the end for which bound the kernel sits against.\n")
    o.append("## Host path, one core of the same machine\n")
    o.append(f"`ssm_vocab_transform_host`: {host['host_transform_ms_per_frame']:.2f} ms per frame ({host['host_transform_ms_per_frame'] * FRAMES:.0f} ms for the {FRAMES} frames); "
             f"`ssm_bow_score_host`: {host['host_score_us_per_pair']:.2f} µs per pair through ctypes ({host['host_query_ms_500500_pairs']:.0f} ms for the 500 500 pairs).\n")
    ta, tq = min(add["add_ms_variant0"]), min(qry["query_ms"])
    o.append(f"Device against host: add {host['host_transform_ms_per_frame'] * FRAMES / ta:.0f} x, query {host['host_query_ms_500500_pairs'] / tq:.0f} x.\n")
    if a.parent:
        key = "value"
        o.append("## `python bench.py` (default line), parent commit and this tree alternated in one call\n")
        o.append("| tree | " + " | ".join(f"run {i + 1}" for i in range(a.bench_rounds)) + " | range |\n|---|" + "---|" * (a.bench_rounds + 1))
        for who in ("parent", "new"):
            vals = [b.get(key) for b in bench[who]]
            o.append(f"| {who} | " + " | ".join(f"{x:.1f}" for x in vals) + f" | {rng_of(vals)} |")
        o.append(f"\n(`{bench['new'][0].get('metric', 'value')}`, {bench['new'][0].get('unit', '')}; no existing kernel changed.)\n")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(o) + "\n")
    print("\n".join(o))


if __name__ == "__main__":
    main()
