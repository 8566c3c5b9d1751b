"""Writes tests/golden/uvd.npz from tests/uvd_ref.py (the independent restatement of UVDisparity::Process): two of the small scenes -- one
whose mask survives, one whose mask verifyByInliers removes -- with their inputs and every output: the three masks, the adjusted U-disparity image, the union
mask, the edited match flags and dis_c, the integer results (status, v_cols, Otsu threshold, line points, seeds, masks found / merged / kept, moving pixels)
and the float results (slope, V_C, measured and filtered pitch).  Arrays only.
Run from the repository root: python tests/golden/make_uvd_golden.py"""
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import uvd_ref as R  # noqa: E402


def main():
    out = {}
    for name in ("moving", "verified_away"):
        left, disp, m, fl, P = R.build_scene(name)
        r = R.process(R.Kalman(), R.Kalman(), left, disp, m, fl, P)
        out.update({name + "_left": left, name + "_disp": disp, name + "_moving": r["moving"], name + "_roi": r["roi"], name + "_ground": r["ground"],
                    name + "_u_adj": r["u_adj"], name + "_union": r["union"], name + "_flags": r["flags"], name + "_dis_c": r["matches"]["dis_c"],
                    name + "_ints": np.array([r["status"], r["v_cols"], r["otsu"], len(r["pts"]), len(r["areas"]), len(r["found"]), len(r["merged"]), len(r["kept"]),
                                              r["n_moving"]], np.int32),
                    name + "_floats": np.array([r["slope"], r["v_c"], r["pitch_measured"], r["pitch_filtered"]], np.float64)})
    np.savez_compressed(os.path.join(HERE, "uvd.npz"), **out)
    print(os.path.getsize(os.path.join(HERE, "uvd.npz")), "bytes")


if __name__ == "__main__":
    main()
