"""Generate the box-flow fixtures g11a_boxflow.npz ... g11f_boxflow.npz from the REFERENCE itself
(``conduct_optical_flow_jit`` / ``conduct_optical_flow``, OF.py:24-218), imported with the stand-ins of make_golden.py
(the numba decorators become the identity, so the decorated loop runs as plain numpy).  Numeric arrays only.

Every case holds the movie, ``v_x, v_y, speed`` of the run without and ``r_v_x, r_v_y, r_net_remodelling`` of the run with
remodelling (``speed`` of that run is asserted all zero here and not stored), ``box``, ``delta_x``, ``delta_t``.  Case f
holds two such sets from the wrapper: prefix ``s_`` (smoothing_sigma) and ``b_`` (background) plus their ``blurred_data``.
The conditioning number of every case (tests/boxflow_restatement.py) must stay below 1e5, so that the error bound of the GPU
tests means something.

Usage:  python tests/golden/make_boxflow_golden.py
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

KAPPA_CAP = 1e5


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
        return fn(*a, **k)


def check_kappa(name, movie, box, fields, remodelling):
    from boxflow_restatement import box_flow, kappa_max
    r = box_flow(movie, box, include_remodelling=remodelling)
    k = kappa_max(r["kappa"], *fields)
    print(f"  {name} remodelling={remodelling}: kappa_max {k:.3g}, non-finite {int((~np.isfinite(fields[0])).sum())}")
    assert k <= KAPPA_CAP, (name, k)


def jit_case(OF, name, movie, box, dx, dt):
    vx, vy, sp, _ = quiet(OF.conduct_optical_flow_jit, movie, box, dx, dt, False)
    rx, ry, rs, rg = quiet(OF.conduct_optical_flow_jit, movie, box, dx, dt, True)
    assert not rs.any()
    check_kappa(name, movie, box, (vx, vy, sp), False)
    check_kappa(name, movie, box, (rx, ry, rg), True)
    path = os.path.join(HERE, name)
    np.savez_compressed(path, movie=movie, box=np.int64(box), delta_x=np.float64(dx), delta_t=np.float64(dt), v_x=vx, v_y=vy,
                        speed=sp, r_v_x=rx, r_v_y=ry, r_net_remodelling=rg)
    print(f"{name}: {os.path.getsize(path)} bytes")


def main():
    from make_golden import import_reference
    from oracle import vof_oracle as orc
    OF = import_reference()
    tex = orc.make_texture_stack(64, 3, seed=0)
    jit_case(OF, "g11a_boxflow.npz", tex[:, :48, :64], 15, 0.25, 0.5)
    jit_case(OF, "g11b_boxflow.npz", tex[:, :64, :40], 7, 1.0, 1.0)
    jit_case(OF, "g11c_boxflow.npz", tex[:, :40, :56], 6, 1.0, 2.0)
    jit_case(OF, "g11d_boxflow.npz", np.round(orc.make_texture_stack(48, 2, seed=11) * 255.0).astype(np.uint8), 31, 0.0913, 10.0)
    gauss, dx = orc.make_gaussian_stack(40, 3)
    jit_case(OF, "g11e_boxflow.npz", gauss, 15, float(dx), 1.0)

    # f: the wrapper - blur, and background subtraction with both branches of the mask
    # (the first pair of a 40 x 52 crop of case a's texture: 18 planes have to fit the size of the largest older fixture)
    movie = np.ascontiguousarray(tex[:2, :40, :52])
    # background: the 20th percentile of the sigma-10-blurred movie.  At its median the zeroed regions are wider than the
    # window and whole windows become flat (conditioning 1e16); at the 20th percentile a fifth of the pixels is masked
    # and the conditioning stays below the cap
    background = float(np.percentile(quiet(OF.blur_movie, movie, smoothing_sigma=10), 20))
    out = dict(movie=movie, box=np.int64(15), delta_x=np.float64(0.25), delta_t=np.float64(0.5),
               smoothing_sigma=np.float64(1.5), background=np.float64(background))
    for prefix, kw in (("s_", dict(smoothing_sigma=1.5)), ("b_", dict(background=background))):
        res = quiet(OF.conduct_optical_flow, movie, 15, 0.25, 0.5, include_remodelling=False, **kw)
        rem = quiet(OF.conduct_optical_flow, movie, 15, 0.25, 0.5, include_remodelling=True, **kw)
        assert res["original_data"] is movie and not rem["speed"].any()
        assert sorted(res) == ["blurred_data", "delta_t", "delta_x", "original_data", "speed", "v_x", "v_y"]
        assert sorted(rem) == sorted(list(res) + ["net_remodelling"])
        if prefix == "b_":
            frac = float((res["blurred_data"] == 0.0).mean())
            assert 0.1 < frac < 0.8, frac        # both branches of the mask occur
        check_kappa("f " + prefix, res["blurred_data"], 15, (res["v_x"], res["v_y"], res["speed"]), False)
        check_kappa("f " + prefix, res["blurred_data"], 15, (rem["v_x"], rem["v_y"], rem["net_remodelling"]), True)
        out.update({prefix + "blurred_data": res["blurred_data"], prefix + "v_x": res["v_x"], prefix + "v_y": res["v_y"],
                    prefix + "speed": res["speed"], prefix + "r_v_x": rem["v_x"], prefix + "r_v_y": rem["v_y"],
                    prefix + "r_net_remodelling": rem["net_remodelling"]})
    path = os.path.join(HERE, "g11f_boxflow.npz")
    np.savez_compressed(path, **out)
    print(f"g11f_boxflow.npz: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
