"""Generate g19_piv_convert.npz from the REFERENCE's own convert_PIV_result (source/optical_flow.py:2141-2230).

Runs only where the reference is checked out (see make_golden.py, whose stand-in import is used: none of the four replaced modules
is touched by convert_PIV_result, which is numpy and scipy.interpolate.griddata).  The input is a synthetic PIVlab-shaped result -
object arrays whose [k][0] is a 2-D array, as scipy.io.loadmat returns them - for a square 3-frame movie of 40 x 40 pixels: a 7 x 7
grid of step 6, three frames of vectors (one more than the movie has pairs: the reference unpacks it and does not upsample it), a
corner, a border and an interior vector missing in frame 0 and another border vector in frame 1, delta_t = 2.

Usage:  python tests/golden/make_piv_golden.py   (writes tests/golden/g19_piv_convert.npz)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))


def main():
    from make_golden import import_reference
    import piv_restatement as pr
    OF = import_reference()
    case = pr.grid_case((40, 40), 6, [[(0, 0), (3, 6), (2, 4)], [(6, 2)], []], 19)
    movie = np.random.default_rng(19).integers(0, 256, (3, 40, 40)).astype(np.uint8)
    delta_x, delta_t = 1.0, 2.0
    res = OF.convert_PIV_result(pr.pivlab_result(case["x"], case["y"], case["vx"], case["vy"]), movie, delta_x=delta_x, delta_t=delta_t)
    assert res["original_data"] is movie
    np.savez_compressed(os.path.join(HERE, "g19_piv_convert.npz"), movie=movie, x=case["x"], y=case["y"], u_original=case["vx"],
                        v_original=case["vy"], kw_delta_x=np.float64(delta_x), kw_delta_t=np.float64(delta_t),
                        **{"out_" + k: np.asarray(res[k]) for k in res if k != "original_data"})
    print({k: np.asarray(v).shape for k, v in res.items()})


if __name__ == "__main__":
    main()
