"""Writes tests/golden/pgo.npz from tests/pgo_ref.py (the independent restatement of the pose-graph optimiser's contract): per scene of
pgo_ref.SCENES its start poses, edges and measurements, and per mode (g = global, l = local) the iteration count, the restatement's final poses, per-trial
accept masks and gains, the chi2 before / after every iteration and the measured ordering spread s: the largest pose-entry difference between two runs
of the restatement that differ only in the order of the unknowns (insertion order / reversed).  The tests allow 64 s between the product and the
restatement: the product's summation order differs on top of its solver order.
The iteration count of a (scene, mode) is the largest K <= 10 for which every trial of the first K iterations has |gain| >= 1e-3 -- below that the
accept decision is rounding noise and two correct implementations may disagree; the generator asserts it.  Arrays only.
Run from the repository root: python tests/golden/make_pgo_golden.py"""
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pgo_ref as R  # noqa: E402

MIN_GAIN = 1e-3


def main():
    out = {}
    for name, kw in R.SCENES.items():
        sc = R.make_scene(**kw)
        out[f"{name}_poses"] = sc["poses"]; out[f"{name}_edges"] = sc["edges"].astype(np.int32); out[f"{name}_Z"] = sc["Z"]
        for mode, local in (("g", False), ("l", True)):
            probe = R.scene_graph(sc, local).optimize(10)
            K = 0
            while K < probe["iterations"] and all(abs(x) >= MIN_GAIN for x in probe["gains"][K]):
                K += 1
            assert K >= 1, (name, mode, probe["gains"])
            g = R.scene_graph(sc, local); res = g.optimize(K)
            g2 = R.scene_graph(sc, local); res2 = g2.optimize(K, reverse=True)
            assert res["iterations"] == K and all(abs(x) >= MIN_GAIN for gl in res["gains"] for x in gl), (name, mode)
            assert res["accepted"] == res2["accepted"] and res["trials"] == res2["trials"], (name, mode)
            s = float(np.max(np.abs(g.X - g2.X)))
            assert s > 0
            gains = np.zeros((K, R.MAX_TRIALS))
            for i, gl in enumerate(res["gains"]):
                gains[i, :len(gl)] = gl
            p = f"{name}_{mode}_"
            out[p + "iterations"] = np.int32(K); out[p + "poses"] = g.X; out[p + "trials"] = np.array(res["trials"], np.int32)
            out[p + "accepted"] = np.array(res["accepted"], np.uint32); out[p + "gains"] = gains
            out[p + "chi2_before"] = np.array(res["chi2_before"]); out[p + "chi2_after"] = np.array(res["chi2_after"])
            out[p + "s"] = np.float64(s); out[p + "active"] = np.array([res["active_vertices"], res["active_edges"]], np.int32)
            rejected = sum(t - bin(a).count("1") for t, a in zip(res["trials"], res["accepted"]))
            print(f"{name:7s} {mode}: K = {K:2d}  s = {s:.3e}  bound = {64 * s:.3e}  rejected trials = {rejected}  chi2 {res['chi2_before'][0]:.4g} -> {res['chi2_after'][-1]:.4g}")
    path = os.path.join(HERE, "pgo.npz")
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
