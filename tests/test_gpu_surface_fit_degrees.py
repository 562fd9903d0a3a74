"""NURBS surface fitting at degrees other than 2 x 2 and 3 x 3: the runtime-degree instantiations (``DEG = 0``) of
``art_surface_fit_prepare / _loss_grad / _run`` (include/artist_hip_surface_fit.h), which no fixture of
tests/test_gpu_surface_fit.py or tests/test_gpu_surface_fit_large.py reaches.  The yardsticks are theirs: the numpy restatement's
own fp32-vs-fp64 distance (tests/surface_fit_ref.py) times K_GRAD, and - between the chunked and the resident path - equality of
bits."""
import functools

import numpy as np
import pytest
import torch

import surface_fit_ref as sfr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
PLATEAU = dict(factor=0.2, patience=5, threshold=1e-7, threshold_mode="abs")
K_GRAD, FLOOR_GRAD = 3.0, 2e-4              # tests/test_gpu_surface_fit.py::test_loss_and_gradient_against_the_helper
ADAM = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, maximize=False)
SHAPES = [((6, 5), (3, 2)), ((7, 7), (4, 4))]        # (net, degrees): 3 x 3 = 9 span cells each
METHODS = [sfr.POINTS, sfr.NORMALS]
NPTS, N_VALID, EPOCHS = 200, [200, 137], 12
KNOB = "ARTIST_HIP_FIT_CHUNK"


def t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def n(x):
    return x.detach().cpu().numpy()


def same_bits(a, b):
    """``torch.equal`` on the bit patterns (tests/test_gpu_surface_fit_large.py)."""
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    elif a.dtype == torch.float64:
        a, b = a.view(torch.int64), b.view(torch.int64)
    return a.shape == b.shape and torch.equal(a, b)


@functools.lru_cache(maxsize=None)
def batch():
    """Two facets of 200 rows; the second counts its first 137 only (filler 7.0 beyond them)."""
    facets = [sfr.synthetic_facet(NPTS, 5200 + k) for k in range(2)]
    pts, nrm = np.stack([f[0] for f in facets]), np.stack([f[1] for f in facets])
    pts[1, N_VALID[1]:] = 7.0
    nrm[1, N_VALID[1]:] = 7.0
    return pts, nrm


def all_outputs(net, deg, method):
    """Everything prepare, loss_grad and 12 plateau-scheduled epochs of run write for the batch."""
    from artist_amd import SurfaceGenerator
    from artist_amd.surface_generator import _FitState, plateau_hyperparameters, run_epochs
    m = 0 if method == sfr.POINTS else 1
    pts, nrm = batch()
    prep = SurfaceGenerator(torch.tensor(net), torch.tensor(deg)).prepare(t(pts), t(np.array(N_VALID), torch.int32))
    targets = t(pts if m == 0 else nrm)
    out = dict(eval_uv=prep.eval_uv, cp0=prep.initial_control_points.clone(), perm=prep.perm, cell_start=prep.cell_start, table=prep.table)
    out["loss"], out["grad"], out["points"], out["normals"] = prep.loss_grad(prep.initial_control_points, targets, m, with_points=True)
    sched = plateau_hyperparameters(None)
    sched.update(use=True, factor=PLATEAU["factor"], patience=PLATEAU["patience"], threshold=PLATEAU["threshold"], threshold_abs=True)
    state = _FitState(prep.initial_control_points.clone(), 1e-3, sched)
    run_epochs(prep, state, targets, m, EPOCHS, 1e-10, 400, ADAM, sched)
    out.update(cp=state.control_points, exp_avg=state.exp_avg, exp_avg_sq=state.exp_avg_sq, f64=state.f64, i32=state.i32,
               last_loss=state.last_loss)
    out["loss_end"], out["grad_end"] = prep.loss_grad(state.control_points, targets, m)[:2]
    return out


_UNFORCED = {}


def unforced(net, deg, method, monkeypatch):
    """The outputs of the call the host chooses by itself (resident), computed once per case and left unchanged."""
    key = (net, deg, method)
    if key not in _UNFORCED:
        monkeypatch.delenv(KNOB, raising=False)
        _UNFORCED[key] = all_outputs(net, deg, method)
    return _UNFORCED[key]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}_d{s[1][0]}{s[1][1]}")
def test_loss_and_gradient_against_the_helper_at_other_degrees(shape, method, monkeypatch):
    """(a) loss and gradient of both facets against the helper, at the initial net and 12 epochs on."""
    net, deg = shape
    out = unforced(net, deg, method, monkeypatch)
    pts_np, nrm_np = batch()
    targets_np = pts_np if method == sfr.POINTS else nrm_np
    degrees = np.array(deg)
    assert out["i32"][:, 3].tolist() == [EPOCHS, EPOCHS] and torch.isfinite(out["cp"]).all()
    for b, k in enumerate(N_VALID):
        uv = n(out["eval_uv"])[b, :k]
        assert np.array_equal(uv, sfr.normalize_points(pts_np[b, :k, :2]))
        assert np.array_equal(n(out["cp0"])[b], sfr.initial_net(pts_np[b, :k], net[0], net[1]))
        for tag, cp_key, loss_key, grad_key in (("initial", "cp0", "loss", "grad"), ("epoch 12", "cp", "loss_end", "grad_end")):
            cp = n(out[cp_key])[b].copy()
            loss, grad = float(out[loss_key][b]), n(out[grad_key])[b]
            loss32, grad32, _, _ = sfr.loss_and_grad(cp, uv, targets_np[b, :k], degrees, method)
            loss64, grad64, _, _ = sfr.loss_and_grad(cp.astype(np.float64), uv.astype(np.float64), targets_np[b, :k].astype(np.float64),
                                                     degrees, method)
            yard = sfr.rel_l2(grad32, grad64)
            err = sfr.rel_l2(grad, grad32)
            loss_yard = abs(float(loss32) - float(loss64)) / float(loss64)
            loss_err = abs(loss - float(loss32)) / float(loss64)
            print(f"degrees {deg} net {net} {method} facet {b} {tag}: grad rel-L2 vs helper {err:.3e}, yardstick (helper fp32 vs fp64) "
                  f"{yard:.3e}; loss {loss:.9e} helper {float(loss32):.9e} fp64 {float(loss64):.9e}")
            assert err < max(K_GRAD * yard, FLOOR_GRAD), (b, tag, err, yard)
            assert loss_err < max(K_GRAD * loss_yard, FLOOR_GRAD), (b, tag, loss, float(loss32), loss_yard)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}_d{s[1][0]}{s[1][1]}")
def test_forced_chunking_gives_the_same_bits_at_other_degrees(shape, method, monkeypatch):
    """(b) ARTIST_HIP_FIT_CHUNK=64 forces the chunked run / loss_grad and the tiled prepare: 200 rows over 9 cells are four
    chunks with a partial last one (137 rows: three), and cells that straddle chunks.  Every output has the bits of the unforced
    call."""
    net, deg = shape
    want = unforced(net, deg, method, monkeypatch)
    monkeypatch.setenv(KNOB, "64")
    got = all_outputs(net, deg, method)
    for key in want:
        assert same_bits(want[key], got[key]), key
    starts = n(got["cell_start"])
    assert starts[:, -1].tolist() == N_VALID and int((np.diff(starts[0]) > 0).sum()) > 4       # more occupied cells than chunks
