"""The case tables of the two sun-blur shape tests (tests/test_gpu_flux_blur_shapes.py, tests/test_gpu_radial_blur_shapes.py)
without a GPU: ``flux_blur_ref.tiling`` and ``radial_blur_ref.tiling`` restate the launch decisions of
artist_amd/csrc/flux_blur_kernels.hip and radial_blur_kernels.hip, and the tables in the two reference modules must reach every
branch those restatements name - a case that stopped reaching its branch (an edited constant, a shape dropped) fails here, not
silently on the GPU.  Also: the references stay self-adjoint at shapes of several tiles, and no expected output is NaN."""
import numpy as np
import pytest

import flux_blur_ref as gauss
import radial_blur_ref as radial


# ---- the Gaussian window -----------------------------------------------------------------------------------------------------
def test_gaussian_cases_reach_every_branch():
    reached = {}
    for shape in gauss.SHAPES:
        for index, covariance in enumerate(gauss.COVARIANCES):
            plan = gauss.tiling(covariance, *shape)
            assert plan is not None, (index, shape)
            for name in plan["branches"]:
                reached.setdefault(name, (index, shape))
    print("first case per branch", reached)
    assert set(reached) == set(gauss.BRANCHES), set(gauss.BRANCHES) - set(reached)
    assert {name for _, name in gauss.CASES} == set(gauss.INPUTS) and {shape for shape, _ in gauss.CASES} == set(gauss.SHAPES)


@pytest.mark.parametrize("index,shape,names", gauss.CLAIMS, ids=[f"cov{i}-{s[0]}x{s[1]}" for i, s, _ in gauss.CLAIMS])
def test_gaussian_case_reaches_what_its_comment_claims(index, shape, names):
    plan = gauss.tiling(gauss.COVARIANCES[index], *shape)
    assert names <= plan["branches"], (names - plan["branches"], plan)


def test_gaussian_plan_in_numbers():
    """The figures the table's comments state."""
    limit = gauss.tiling(gauss.COVARIANCES[1], 300, 130)
    assert (limit["Kr"], limit["Ka"], limit["TR"], limit["grid"]) == (64, 64, 256, (2, 3))
    for index, s in ((2, 0.78125), (3, -0.78125)):
        plan = gauss.tiling(gauss.COVARIANCES[index], 257, 66)
        assert (plan["Kr"], plan["Ka"], plan["s"]) == (64, 40, s)
    last16, first10 = gauss.tiling(gauss.COVARIANCES[5], 300, 130), gauss.tiling(gauss.COVARIANCES[6], 300, 130)
    assert (last16["s"], last16["shear_bits"], last16["grid"][1]) == (64.0, 16, 258)
    assert (first10["s"], first10["shear_bits"]) == (64.25, 10)
    assert len(last16["skipped"]) > last16["groups"]                    # most tiles are corners, every workgroup walks several
    assert (first10["lean"], gauss.tiling(gauss.COVARIANCES[7], 257, 66)["lean"]) == (64.25, 90.0)     # s rounded to 10 bits
    assert abs(gauss.tiling(gauss.COVARIANCES[7], 257, 66)["s"] - 90.0) < 1e-6
    assert abs(gauss.tiling(gauss.COVARIANCES[8], 513, 40)["s"] + 70.0) < 1e-6
    # Hh = 129: a full block of 128 rows, then one row in a wave of 8; Hh = 257: the second tile row holds one row
    assert gauss.tiling(gauss.COVARIANCES[1], 129, 70)["runs"][(0, 0)] == (0, 129)
    assert gauss.tiling(gauss.COVARIANCES[1], 257, 66)["runs"][(1, 0)] == (0, 1)
    for bad in ((4.0, 5.0, 4.0), (300.0, 0.0, 9.0), (float("nan"), 0.0, 1.0)):
        assert gauss.tiling(bad, 48, 40) is None


def test_gaussian_inputs():
    for shape, name in gauss.CASES:
        x = gauss.case_input(shape, name)
        assert x.shape == shape and x.dtype == np.float32 and np.isfinite(x).all() and np.any(x != 0), (shape, name)
        assert np.array_equal(x, gauss.case_input(shape, name))
    assert (gauss.case_input((300, 130), "dense") < 0).any()
    seams = gauss.case_input((300, 130), "seams")
    assert all(seams[r, c] != 0 for r in (0, 127, 128, 255, 256, 299) for c in (0, 63, 64, 129)) and np.count_nonzero(seams) == 24
    assert np.unique(np.abs(seams[seams != 0])).size == 24
    bands = gauss.case_input((300, 130), "bands")
    assert set(np.nonzero(bands.any(axis=1))[0]) == {100, 101, 102, 299} and not bands[299, :65].any()


@pytest.mark.parametrize("index", range(len(gauss.COVARIANCES)))
def test_gaussian_reference_is_self_adjoint_and_finite_over_several_tiles(index):
    rng = np.random.default_rng(5)
    x, y = rng.standard_normal((2, 257, 66))
    fx, fy = gauss.blur_one(x, gauss.COVARIANCES[index]), gauss.blur_one(y, gauss.COVARIANCES[index])
    assert np.isfinite(fx).all() and np.isfinite(fy).all()              # no row of the table is a NaN bitmap
    assert abs((fx * y).sum() - (x * fy).sum()) <= 1e-12 * np.linalg.norm(x) * np.linalg.norm(y)


def test_gaussian_yardsticks_make_the_bound_meaningful():
    """fp32 against fp64 on the largest dense case: between 1e-8 and 4e-6 of the peak for every covariance."""
    x = np.repeat(gauss.case_input((300, 130), "dense")[None], len(gauss.COVARIANCES), axis=0)
    want, yard = gauss.yardstick(x, gauss.COVARIANCES)
    ratio = yard / np.abs(want).reshape(len(yard), -1).max(axis=1)
    print("yardstick / peak", ratio)
    assert not np.isnan(want).any() and (ratio <= 4e-6).all()


# ---- the radial window -------------------------------------------------------------------------------------------------------
def test_radial_cases_reach_every_branch():
    reached = {}
    tables = radial.tables()
    for table_name, shape, _ in radial.CASES:
        table, metrics, _ = tables[table_name]
        for index, metric in enumerate(metrics):
            plan = radial.tiling(metric, table, *shape, len(metrics))
            assert plan is not None, (table_name, index, shape)
            for name in plan["branches"]:
                reached.setdefault(name, (table_name, index, shape, len(metrics)))
    for table_name, shape, batches in radial.BATCH_CASES:
        table, metrics, _ = tables[table_name]
        for B in batches:
            for name in radial.tiling(metrics[0], table, *shape, B)["branches"]:
                reached.setdefault(name, (table_name, 0, shape, B))
    print("first case per branch", reached)
    assert set(reached) == set(radial.BRANCHES), set(radial.BRANCHES) - set(reached)
    assert {t for t, _, _ in radial.CASES} == set(tables)


def test_radial_case_reaches_what_its_comment_claims():
    for table_name, (table, metrics, claims) in radial.tables().items():
        assert len(claims) == len(metrics)
        for index, (metric, names) in enumerate(zip(metrics, claims)):
            plan = radial.tiling(metric, table, *radial.CLAIM_SHAPE, len(metrics))
            assert names <= plan["branches"], (table_name, index, names - plan["branches"], plan)
            assert {"ragged_rows", "ragged_cols"} <= plan["branches"]          # (130, 70) is ragged under every shape
    tables = radial.tables()
    # every shape but the first also runs with ragged last tiles in both directions, and stencil row 64 holds taps where claimed
    plan = radial.tiling(tables["pillbox"][1][3], tables["pillbox"][0], 130, 70, 6)
    assert (plan["Rr"], plan["Rc"], plan["row64_taps"], plan["shape"]) == (64, 64, 11, (1, 2, 64))
    plan = radial.tiling(tables["pillbox"][1][4], tables["pillbox"][0], 130, 70, 6)
    assert (plan["Rr"], plan["Rc"]) == (64, 20) and plan["row64_taps"] > 0
    plan = radial.tiling(tables["pillbox"][1][5], tables["pillbox"][0], 130, 70, 6)
    assert (plan["Rr"], plan["Rc"]) == (20, 64)
    plan = radial.tiling(tables["uniform4096"][1][0], tables["uniform4096"][0], 130, 70, 1)
    assert (plan["kstar"], plan["table_chunks"], plan["shape"], plan["row64_taps"] > 0) == (2621, 5, (1, 1, 32), True)


def test_radial_batches_change_the_launch():
    tables = radial.tables()
    table, metrics, _ = tables["uniform4096"]
    small = [radial.tiling(metrics[0], table, 40, 20, B) for B in (1, 1025, 2049)]
    assert [p["share"] for p in small] == [2048, 2, 1] and [p["groups"] for p in small] == [1, 1, 1]
    assert all(p["grid"] == (2, 3) and "tiles>groups" in p["branches"] for p in small)      # one workgroup, one stencil, six tiles
    large = [radial.tiling(metrics[0], table, 130, 70, B) for B in (1, 1025, 2049)]
    assert [p["groups"] for p in large] == [4, 2, 1]                    # here B sets the grid
    assert ["share<tiles" in p["branches"] for p in large] == [False, True, True]


def test_radial_spot_cases_have_zero_tiles_and_a_late_stencil():
    table, metrics, _ = radial.tables()["pillbox"]
    x = radial.case_input(radial.SPOT_SHAPE, "spot")
    assert np.count_nonzero(x) == 6 and x[190:193, 140:142].all()
    plans = [radial.tiling(metric, table, *radial.SPOT_SHAPE, 2, x) for metric in metrics[:2]]
    print([(p["shape"], p["grid"], p["groups"], p["zero_tiles"], p["late_stencil"]) for p in plans])
    for plan in plans:
        assert plan["zero_ragged_tiles"] and len(plan["zero_tiles"]) < plan["grid"][0] * plan["grid"][1]
    # under the 5 px disc every workgroup has one tile; under the 50 px one some workgroup meets a zero tile, then the spot's
    assert [plan["late_stencil"] for plan in plans] == [False, True]
    assert radial.tiling(metrics[0], table, *radial.SPOT_SHAPE, 2, np.zeros(radial.SPOT_SHAPE))["late_stencil"] is False


def test_radial_inputs():
    for shape in radial.SHAPES:
        for name in radial.INPUTS:
            x = radial.case_input(shape, name)
            assert x.shape == shape and x.dtype == np.float32 and np.isfinite(x).all() and np.any(x != 0), (shape, name)
    seams = radial.case_input((130, 70), "seams")
    assert all(seams[r, c] != 0 for r in (0, 129) for c in (0, 69))
    assert all(seams[r, c] != 0 for r in radial.SEAM_ROWS for c in radial.SEAM_COLS) and np.count_nonzero(seams) == 28
    assert (radial.case_input((130, 70), "dense") < 0).any()


@pytest.mark.parametrize("table_name,index", [("pillbox", 3), ("pillbox", 4), ("pillbox", 5), ("uniform4096", 0), ("buie", 0)])
def test_radial_reference_is_self_adjoint_and_finite_over_several_tiles(table_name, index):
    table, metrics, _ = radial.tables()[table_name]
    rng = np.random.default_rng(5)
    x, y = rng.standard_normal((2, 130, 70))
    w = radial.stencil(metrics[index], table)
    fx, fy = radial.convolve(x, w, np.float64), radial.convolve(y, w, np.float64)
    assert np.isfinite(fx).all() and np.isfinite(fy).all()
    assert abs((fx * y).sum() - (x * fy).sum()) <= 1e-12 * np.linalg.norm(x) * np.linalg.norm(y)


def test_no_radial_case_is_a_nan_bitmap():
    for table_name, (table, metrics, _) in radial.tables().items():
        for metric in metrics:
            assert radial.k_star(metric, table) is not None, (table_name, metric)
