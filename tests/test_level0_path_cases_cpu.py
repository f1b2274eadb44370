"""The tables of tests/level0_path_cases.py cannot thin out unnoticed: every option value and every shape is still there, every case
still runs the register-resident pass by the restated rule, the shapes still sit on the strip and band edges of s0_geometry as
it stands, and for every solve case the oracle's direct solve is accurate enough to be the reference."""
import collections
import os
import re

import pytest

import level0_path_cases as lc
from conftest import ROOT
from oracle import mg_prototype as mg

CSRC = os.path.join(ROOT, "opticalflow_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_restated_constants_are_the_library_s():
    dev, hip, s0r, ctx = source("vof_device.hpp"), source("vof.hip"), source("vof_sweep0r.hpp"), source("vof_host.hpp")
    assert int(re.search(r"constexpr int S0_W = (\d+)", dev).group(1)) == lc.S0_W
    assert int(re.search(r"constexpr int AUTO_F64_AFTER = (\d+)", hip).group(1)) == lc.AUTO_F64_AFTER
    assert int(re.search(r"long sweep0r_min_blocks = (\d+)", ctx).group(1)) == lc.DEFAULT_MIN_BLOCKS
    # the strip width, in the kernel's geometry (HALO = 4 NS + 2 EXT, OUT = S0_W - 2 HALO) and in the host's plan
    # (out = S0_W - 8 NSW - 4 with a trailing stage), and the band caps of pick_band_height: the numbers, whatever the layout
    m = re.search(r"HALO\s*=\s*(\d+)\s*\*\s*NS\s*\+\s*(\d+)\s*\*\s*EXT\s*,\s*OUT\s*=\s*S0_W\s*-\s*(\d+)\s*\*\s*HALO", s0r)
    assert m and [int(v) for v in m.groups()] == [4, 2, 2]
    m = re.search(r"out\s*=\s*S0_W\s*-\s*(\d+)\s*\*\s*NSW\s*-\s*\(\s*trail\s*\?\s*(\d+)\s*:\s*(\d+)\s*\)", hip)
    assert m and [int(v) for v in m.groups()] == [8, 4, 0]
    m = re.search(r"blocks128\s*<\s*(\d+)\s*\?\s*(\d+)\s*:\s*\(\s*blocks128\s*<\s*(\d+)\s*\?\s*(\d+)\s*:\s*(\d+)\s*\)", hip)
    assert m and [int(v) for v in m.groups()] == [768, 32, 1536, 64, 128]
    assert mg.COARSEST_MAX == lc.COARSEST_MAX
    assert [lc.strip_width(ns, trail) for ns, trail in ((2, False), (2, True), (1, False), (1, True))] == [112, 108, 120, 116]


def test_shapes_sit_on_the_strip_and_band_edges():
    assert len(lc.SHAPES) == len(set(lc.SHAPES)) >= 14
    widths = {s[1] - 2 for s in lc.SHAPES}
    heights = {s[0] - 2 for s in lc.SHAPES}
    assert {108, 110, 112, 114, 116, 118, 120, 122, 216, 224, 226, 34} <= widths
    assert {6, 31, 32, 33, 34, 64} <= heights
    for ns, trail in ((2, False), (2, True), (1, False), (1, True)):
        out = lc.strip_width(ns, trail)
        assert out in widths and out + 2 in widths                       # a strip exactly full, and full plus two columns
        assert lc.strip_count(out, ns, trail) == 1 and lc.strip_count(out + 2, ns, trail) == 2
    assert lc.strip_count(216, 2, True) == 2 and lc.strip_count(224, 2, False) == 2 and lc.strip_count(226, 2, False) == 3
    assert lc.strip_count(34, 2, True) == 1
    # small launches cap a band at 32 rows; the reverse pass covers one row more
    assert [lc.band_height(rows, 1) for rows in (6, 7, 31, 32, 33, 34, 35, 64, 65)] == [6, 8, 32, 32, 18, 18, 18, 32, 22]
    for shape in lc.SHAPES:
        assert len(mg.Hierarchy.level_shapes(shape[0] - 2, shape[1] - 2)) > 1
        assert lc.takes_register_pass(shape, True, "float64", min_blocks=0)
        assert not lc.takes_register_pass(shape, True, "float64")                     # why the switch is needed: far below 512 blocks
        assert not lc.takes_register_pass(shape, False, "float64", min_blocks=0)
        assert not lc.takes_register_pass((shape[0], shape[1] + 1), True, "float64", min_blocks=0)
    assert lc.takes_register_pass((1024, 1024), units=8)                              # the product's own sizes reach it unforced
    assert not lc.takes_register_pass((128, 128), units=8)


def test_cycle_table():
    assert len(lc.CYCLES) == len(set(lc.CYCLES)) >= 8
    for row in [(2, 2, 1, 1, 1, 3), (2, 2, 1, 1, -1, 0), (2, 2, 1, 1, 0, 3), (1, 1, 1, 1, 1, 3), (3, 2, 1, 1, 1, 3), (2, 3, 1, 1, -1, 0),
                (1, 2, 2, 2, 0, 2), (3, 3, 2, 1, 1, 2)]:
        assert row in lc.CYCLES
    # every (nu_pre, nu_post) that occurs: one sweep per pass, two, a double and a single pass before / after / both, mixed
    assert {c[:2] for c in lc.CYCLES} == {(2, 2), (1, 1), (3, 2), (2, 3), (1, 2), (3, 3)}
    assert {c[4] for c in lc.CYCLES} == {-1, 0, 1}


def test_solve_table_covers_every_option_and_shape():
    assert len(lc.SOLVE_CASES) == 36 and len({c["seed"] for c in lc.SOLVE_CASES}) == 36
    # only a case whose every cycle runs on the pass counts as coverage - and that is every case
    cases = [c for c in lc.SOLVE_CASES if lc.reaches_register_pass_from_the_first_cycle(c)]
    assert len(cases) == 36
    for key, values in (("krylov_method", lc.KRYLOV_METHODS), ("coarse_precision", lc.COARSE_PRECISIONS), ("vcycle_precision", lc.VCYCLE_PRECISIONS),
                        ("w_cycle_level", lc.W_CYCLE_LEVELS), ("multigrid_sweeps", lc.MULTIGRID_SWEEPS), ("max_pairs_in_flight", lc.MAX_PAIRS),
                        ("scale", lc.SCALES), ("frames", lc.FRAMES), ("shape", tuple(lc.SHAPES))):
        count = collections.Counter(c[key] for c in cases)
        assert set(count) == set(values), key
        assert min(count.values()) >= 2, (key, count)
    count = collections.Counter((c["entry"], c["lanes"]) for c in cases)
    assert set(count) == set(lc.ENTRIES) and min(count.values()) >= 2, count
    for i, c in enumerate(cases):
        assert c == lc.draw_solve_case(i, c["seed"]), i                                # the table is what the generator draws
        assert c["entry"] == "numpy" or c["frames"] - 1 >= c["lanes"]
        assert 10 ** -0.5 <= c["speed_alpha"] / c["scale"] ** 2 <= 100 and 1 <= c["remodelling_alpha"] <= 1e4
        # "auto" reaches the pass from the first cycle under GMRES only; BiCGStab would get there in its ninth iteration
        assert c["vcycle_precision"] != "auto" or c["krylov_method"] == "gmres"
        for method in ("bicgstab", "auto"):
            assert lc.takes_register_pass(c["shape"], True, c["vcycle_precision"], 0, 0, krylov_method=method) == (c["vcycle_precision"] != "auto")
            assert lc.takes_register_pass(c["shape"], True, c["vcycle_precision"], lc.AUTO_F64_AFTER, 0, krylov_method=method)
            assert not lc.takes_register_pass(c["shape"], True, "float32", 1000, 0, krylov_method=method)
        assert lc.takes_register_pass(c["shape"], True, "float32", 0, 0, krylov_method="gmres")
    # the solves that witness the switch (float32 hand-off, on k_sweep0r only)
    assert sum(lc.stores_float32_handoff(c) for c in cases) >= 2


@pytest.mark.parametrize("index", range(len(lc.SOLVE_CASES)))
def test_oracle_alone_is_accurate_enough_to_be_the_reference(index):
    """The fields are compared to 1e-6 with the oracle's direct solve: its own residual (pair 0, units 1, by the matrix-free interior
    operator) must be far below the 1e-10 the library solves to."""
    assert lc.oracle_pair0_residual(lc.SOLVE_CASES[index]) <= lc.ORACLE_RESIDUAL_BAR
