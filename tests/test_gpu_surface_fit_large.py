"""NURBS surface fitting beyond what one CU's LDS holds: the chunked path of ``art_surface_fit_loss_grad / _run`` and the tiled
``art_surface_fit_prepare`` (include/artist_hip_surface_fit.h), up to 2^20 rows per facet.  The yardsticks are
those of tests/test_gpu_surface_fit.py: the numpy restatement's own fp32-vs-fp64 distance (tests/surface_fit_ref.py) times
K_GRAD / MARGIN, and - between the chunked and the resident path - equality of bits."""
import functools
import os

import numpy as np
import pytest
import torch

import surface_fit_ref as sfr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
PLATEAU = dict(factor=0.2, patience=5, threshold=1e-7, threshold_mode="abs")
MARGIN = 3.0                                # tests/test_gpu_surface_fit.py
K_GRAD, FLOOR_GRAD = 3.0, 2e-4              # tests/test_gpu_surface_fit.py::test_loss_and_gradient_against_the_helper
ADAM = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, maximize=False)
LARGE = [(npts, net, deg) for npts in (6000, 20011) for net, deg in ((10, 3), (5, 2))]
METHODS = [sfr.POINTS, sfr.NORMALS]
FIXTURES = [(npts, net, deg, method) for npts in (37, 800) for net, deg in ((5, 2), (10, 3)) for method in METHODS]
KNOB = "ARTIST_HIP_FIT_CHUNK"


def case_name(npts, net, deg, method):
    return f"surface_fit_{npts}_{net}x{net}_d{deg}_{method}"


def t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def n(x):
    return x.detach().cpu().numpy()


def record(line):
    """Measured distances: printed, and appended to the file named by SURFACE_FIT_PARITY_OUT (tests/test_gpu_surface_fit.py)."""
    print(line)
    out = os.environ.get("SURFACE_FIT_PARITY_OUT")
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def generator(net, deg):
    from artist_amd import SurfaceGenerator
    return SurfaceGenerator(torch.tensor([net, net]), torch.tensor([deg, deg]))


def plateau_state(prep):
    from artist_amd.surface_generator import _FitState, plateau_hyperparameters
    sched = plateau_hyperparameters(None)
    sched.update(use=True, factor=PLATEAU["factor"], patience=PLATEAU["patience"], threshold=PLATEAU["threshold"], threshold_abs=True)
    return _FitState(prep.initial_control_points.clone(), 1e-3, sched), sched


def same_bits(a, b):
    """``torch.equal`` on the bit patterns: a facet without valid rows has a NaN loss, which must be the same NaN."""
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    elif a.dtype == torch.float64:
        a, b = a.view(torch.int64), b.view(torch.int64)
    return a.shape == b.shape and torch.equal(a, b)


@functools.lru_cache(maxsize=None)
def facet(npts, seed):
    return sfr.synthetic_facet(npts, seed)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape", LARGE, ids=lambda s: f"{s[0]}_{s[1]}x{s[1]}_d{s[2]}")
def test_loss_and_gradient_beyond_the_resident_limit(shape, method):
    """More points than a CU's LDS holds (6000) and than the old cap of 16384 admitted (20 011: odd, no multiple of 64):
    loss and gradient against the helper at the initial net and 20 epochs on, points and normals bit-equal to NURBSSurfaces."""
    from artist_amd import NURBSSurfaces
    from artist_amd.surface_generator import run_epochs
    npts, net, deg = shape
    pts_np, nrm_np = facet(npts, 4000 + npts % 97)
    m = 0 if method == sfr.POINTS else 1
    targets_np = pts_np if m == 0 else nrm_np
    degrees = np.array([deg, deg])
    prep = generator(net, deg).prepare(t(pts_np)[None])
    targets = t(targets_np)[None]
    uv = n(prep.eval_uv)[0]
    state, sched = plateau_state(prep)
    for epoch in (0, 20):
        if epoch:
            run_epochs(prep, state, targets, m, epoch, 1e-10, 400, ADAM, sched)
            assert int(state.epochs_run[0]) == epoch
        cp = n(state.control_points)[0].copy()
        loss, grad, pts, nrm = prep.loss_grad(t(cp)[None], targets, m, with_points=True)
        loss32, grad32, _, _ = sfr.loss_and_grad(cp, uv, targets_np, degrees, method)
        loss64, grad64, _, _ = sfr.loss_and_grad(cp.astype(np.float64), uv.astype(np.float64), targets_np.astype(np.float64), degrees, method)
        yard = sfr.rel_l2(grad32, grad64)
        err = sfr.rel_l2(n(grad)[0], grad32)
        loss_yard = abs(float(loss32) - float(loss64)) / float(loss64)
        loss_err = abs(float(loss) - float(loss32)) / float(loss64)
        record(f"large loss_grad {case_name(npts, net, deg, method)} epoch {epoch}: grad rel-L2 vs helper {err:.3e}, yardstick (helper fp32 vs "
               f"fp64) {yard:.3e}; loss {float(loss):.9e} helper {float(loss32):.9e} fp64 {float(loss64):.9e}")
        assert err < max(K_GRAD * yard, FLOOR_GRAD), (epoch, err, yard)
        assert loss_err < max(K_GRAD * loss_yard, FLOOR_GRAD), (epoch, float(loss), float(loss32), loss_yard)
        surf = NURBSSurfaces(torch.tensor([deg, deg]), t(cp)[None, None], device=DEV)
        want_pts, want_nrm = surf.calculate_surface_points_and_normals(prep.eval_uv[None], None, None)
        assert torch.equal(pts[0], want_pts[0, 0]) and torch.equal(nrm[0], want_nrm[0, 0])


@pytest.mark.parametrize("shape", LARGE, ids=lambda s: f"{s[0]}_{s[1]}x{s[1]}_d{s[2]}")
def test_prepare_at_large_n(shape):
    npts, net, deg = shape
    pts_np, _ = facet(npts, 4000 + npts % 97)
    prep = generator(net, deg).prepare(t(pts_np)[None])
    uv = sfr.normalize_points(pts_np[:, :2])
    assert np.array_equal(n(prep.eval_uv)[0], uv)
    assert np.array_equal(n(prep.initial_control_points)[0], sfr.initial_net(pts_np, net, net))
    perm, starts = n(prep.perm)[0], n(prep.cell_start)[0]
    assert np.array_equal(np.sort(perm), np.arange(npts)) and starts[0] == 0 and starts[-1] == npts and np.all(np.diff(starts) >= 0)
    ncv = net - deg
    span = np.floor(uv * np.float32(ncv)).astype(np.int64)
    cell = span[:, 0] * ncv + span[:, 1]
    assert np.all(np.diff(cell[perm]) >= 0)                               # cells ascending along the sorted order
    for c in range(ncv * ncv):
        members = perm[starts[c]:starts[c + 1]]
        assert np.all(cell[members] == c) and np.all(np.diff(members) > 0)


def fixture_batch(d, npts):
    """Three copies of a fixture padded to its own N: all rows valid, the first two thirds valid (filler 7.0 beyond them), none."""
    pts, nrm = np.repeat(d["points"][None], 3, 0).copy(), np.repeat(d["normals"][None], 3, 0).copy()
    n_valid = np.array([npts, (2 * npts) // 3, 0], np.int32)
    pts[1, n_valid[1]:] = 7.0
    nrm[1, n_valid[1]:] = 7.0
    return pts, nrm, n_valid


def all_outputs(case, d):
    """Everything prepare, loss_grad and 40 plateau-scheduled epochs of run write for the three-facet batch of a fixture."""
    from artist_amd.surface_generator import run_epochs
    npts, net, deg, method = case
    m = 0 if method == sfr.POINTS else 1
    pts, nrm, n_valid = fixture_batch(d, npts)
    prep = generator(net, deg).prepare(t(pts), t(n_valid, torch.int32))
    targets = t(pts if m == 0 else nrm)
    out = dict(eval_uv=prep.eval_uv, cp0=prep.initial_control_points.clone(), perm=prep.perm, cell_start=prep.cell_start, table=prep.table)
    out["loss"], out["grad"], out["points"], out["normals"] = prep.loss_grad(prep.initial_control_points, targets, m, with_points=True)
    state, sched = plateau_state(prep)
    run_epochs(prep, state, targets, m, 40, 1e-10, 400, ADAM, sched)
    out.update(cp=state.control_points, exp_avg=state.exp_avg, exp_avg_sq=state.exp_avg_sq, f64=state.f64, i32=state.i32,
               last_loss=state.last_loss)
    return out


_UNFORCED = {}


@pytest.mark.parametrize("chunk", [64, 192, 4096])
@pytest.mark.parametrize("case", FIXTURES, ids=lambda c: case_name(*c))
def test_chunked_path_gives_the_bits_of_the_resident_path(golden, case, chunk, monkeypatch):
    """ARTIST_HIP_FIT_CHUNK forces the chunked run / loss_grad and the tiled prepare at the fixtures' N: chunks of 64 (cells of
    ~89 points straddle boundaries on the 5 x 5 net), 192 (a partial last chunk) and 4096 (one chunk, longer than n)."""
    d = golden(case_name(*case))
    if case not in _UNFORCED:
        monkeypatch.delenv(KNOB, raising=False)
        _UNFORCED[case] = all_outputs(case, d)
    want = _UNFORCED[case]
    monkeypatch.setenv(KNOB, str(chunk))
    got = all_outputs(case, d)
    for key in want:
        assert same_bits(want[key], got[key]), key
    # the facet without valid rows, as the header describes it; its neighbours did run
    assert got["i32"][:, 3].tolist() == [40, 40, 1] and got["i32"][:, 4].tolist() == [0, 0, 1]
    assert bool(torch.isnan(got["loss"][2])) and bool(torch.isnan(got["last_loss"][2]))
    assert float(got["grad"][2].abs().max()) == 0.0 and float(got["cp"][2].abs().max()) == 0.0
    assert float(got["f64"][:2, 0].max()) <= 1e-3 and torch.isfinite(got["cp"]).all()


@pytest.mark.parametrize("method", METHODS)
def test_large_facet_is_independent_of_batch_padding_and_launches(golden, method):
    """B = 3 facets padded to N = 6000 with n_valid = (6000, 37, 800): every row has the bits of that facet fitted alone at its
    own N (37 and 800 alone take the resident path), 40 epochs in one launch are 4 x 10, and a second run repeats the first."""
    from artist_amd.surface_generator import run_epochs
    gen = generator(10, 3)
    m = 0 if method == sfr.POINTS else 1
    rows = [facet(6000, 4083), (golden(case_name(37, 10, 3, method))["points"], golden(case_name(37, 10, 3, method))["normals"]),
            (golden(case_name(800, 10, 3, method))["points"], golden(case_name(800, 10, 3, method))["normals"])]
    pts, nrm = np.full((3, 6000, 4), 7.0, np.float32), np.full((3, 6000, 4), 7.0, np.float32)
    n_valid = np.array([r[0].shape[0] for r in rows], np.int32)
    for b, (p, q) in enumerate(rows):
        pts[b, :p.shape[0]], nrm[b, :p.shape[0]] = p, q
    opt = torch.optim.Adam([torch.zeros(1, requires_grad=True)], lr=1e-3)
    sch = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, **PLATEAU)
    kw = dict(optimizer=opt, scheduler=sch, fit_method=method, max_epoch=39)

    def state_equal(x, y, i, j):
        return all(same_bits(getattr(x.fit_state, k)[i], getattr(y.fit_state, k)[j])
                   for k in ("control_points", "exp_avg", "exp_avg_sq", "f64", "i32", "last_loss"))

    a, ea, la = gen.fit_nurbs_batch(t(pts), t(nrm), t(n_valid, torch.int32), **kw)
    b, eb, lb = gen.fit_nurbs_batch(t(pts), t(nrm), t(n_valid, torch.int32), **kw)
    assert all(state_equal(a, b, i, i) for i in range(3)) and ea.tolist() == [40, 40, 40] and torch.isfinite(a.control_points).all()
    c, _, _ = gen.fit_nurbs_batch(t(pts), t(nrm), t(n_valid, torch.int32), epochs_per_launch=10, **kw)
    assert all(state_equal(a, c, i, i) for i in range(3))
    for row in range(3):
        k = int(n_valid[row])
        one, _, _ = gen.fit_nurbs_batch(t(pts[row:row + 1, :k]), t(nrm[row:row + 1, :k]), None, **kw)
        assert state_equal(one, a, 0, row), row
    # the loss an epoch reports is loss_grad's at the net it started from
    prep = gen.prepare(t(pts), t(n_valid, torch.int32))
    targets = t(pts if m == 0 else nrm)
    state, sched = plateau_state(prep)
    before = prep.loss_grad(state.control_points, targets, m)[0].clone()
    run_epochs(prep, state, targets, m, 1, 1e-10, 400, ADAM, sched)
    assert torch.equal(before, state.last_loss)


def test_unsupported_names_what_does_not_fit():
    """What is left of ART_EUNSUPPORTED: a net whose own LDS block exceeds 160 KiB.  prepare still runs (it keeps offsets and
    knots only); loss_grad and run say what does not fit, and that the points are not it."""
    from artist_amd import ArtistHipError
    from artist_amd.surface_generator import run_epochs
    pts_np, nrm_np = facet(6000, 4083)
    prep = generator(64, 3).prepare(t(pts_np)[None])
    perm = n(prep.perm)[0]
    assert np.array_equal(np.sort(perm), np.arange(6000))
    with pytest.raises(ArtistHipError, match=r"art_surface_fit_loss_grad: the LDS block of a 64 x 64 net .* does not fit in 160 KiB.*"
                                             r"cell partial sums 697\.7 KiB.*the number of points per facet does not enter"):
        prep.loss_grad(prep.initial_control_points, t(nrm_np)[None], 1)
    state, sched = plateau_state(prep)
    with pytest.raises(ArtistHipError, match=r"art_surface_fit_run: .*does not fit in 160 KiB.*fewer epochs per launch"):
        run_epochs(prep, state, t(nrm_np)[None], 1, 10, 1e-10, 400, ADAM, sched)


def four_large_facets():
    return [facet(20011, 3000 + k) for k in range(4)]


@functools.lru_cache(maxsize=None)
def helper_fits():
    """The helper's 21-epoch fits of the four facets in fp32 and fp64, side by side (numpy releases the interpreter lock)."""
    import concurrent.futures
    jobs = [(k, dtype) for k in range(4) for dtype in (np.float32, np.float64)]

    def one(job):
        p, q = four_large_facets()[job[0]]
        return sfr.fit(p, q, 10, 10, np.array([3, 3]), sfr.NORMALS, dtype=job[1], max_epoch=20)["cp"]

    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as pool:
        return dict(zip(jobs, pool.map(one, jobs)))


def helper_fit(k, dtype):
    return helper_fits()[(k, dtype)]


def test_fit_of_20011_points_follows_the_helper():
    """fit_nurbs_batch on four facets of 20 011 points, 21 epochs, against the helper's fp32 fit; yardstick: the helper's own
    fp32-vs-fp64 drift (so early no Adam sign flip has occurred in either precision: 1.2e-7 to 1.9e-7)."""
    gen = generator(10, 3)
    facets = four_large_facets()
    pts, nrm = t(np.stack([f[0] for f in facets])), t(np.stack([f[1] for f in facets]))
    surf, epochs_run, loss = gen.fit_nurbs_batch(pts, nrm, fit_method=sfr.NORMALS, max_epoch=20)
    assert epochs_run.tolist() == [21] * 4 and torch.isfinite(loss).all()
    for k in range(4):
        want, want64 = helper_fit(k, np.float32), helper_fit(k, np.float64)
        drift = np.abs(want.astype(np.float64) - want64).max()
        err = np.abs(n(surf.control_points)[k, 0].astype(np.float64) - want).max()
        record(f"large fit, facet {k} (20011 points, 21 epochs): max |cp - helper fp32| {err:.3e}, helper fp32-vs-fp64 drift {drift:.3e}")
        assert err <= MARGIN * drift, (k, err, drift)


def test_surface_config_from_every_measured_point():
    """generate_fitted_surface_config with deflectometry_step_size=1 on four facets of 20 011 points: four finite nets whose
    loss over ALL points is lower than that of the nets fitted to every 25th point."""
    gen = generator(10, 3)
    facets = four_large_facets()
    pts3, nrm3 = [t(f[0][:, :3]) for f in facets], [t(f[1][:, :3]) for f in facets]
    zero_tr, cant = torch.zeros(4, 4, device=DEV), torch.zeros(4, 2, 4, device=DEV)
    opt = torch.optim.Adam([torch.zeros(1, requires_grad=True)], lr=1e-3)
    prep = gen.prepare(t(np.stack([f[0] for f in facets])))
    targets = t(np.stack([f[1] for f in facets]))
    losses = {}
    for step in (1, 25):
        fitted = gen.generate_fitted_surface_config("synthetic", zero_tr, cant, pts3, nrm3, opt, None, deflectometry_step_size=step,
                                                    fit_method=sfr.NORMALS, max_epoch=39)
        nets = torch.stack([f.control_points for f in fitted])
        assert len(fitted) == 4 and nets.shape == (4, 10, 10, 3) and torch.isfinite(nets).all()
        losses[step] = n(prep.loss_grad(nets, targets, 1)[0])
    record(f"surface config, loss over all 20011 points: step 1 {losses[1].tolist()}, step 25 {losses[25].tolist()}")
    assert np.all(np.isfinite(losses[1])) and np.all(losses[1] < losses[25]), (losses[1], losses[25])
