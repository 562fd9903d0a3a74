"""TEST INFRASTRUCTURE - ``SurfaceGenerator.fit_nurbs`` (artist/scenario/surface_generator.py:71-223) restated in numpy on top of
``oracle.nurbs_fwd`` / ``oracle.nurbs_bwd`` (scattered points, float32 or float64), with a numpy Adam
(torch/optim/adam.py, ``_single_tensor_adam``) and ``ReduceLROnPlateau``.  tests/test_surface_fit_host.py pins it to the
reference's own runs (tests/golden/surface_fit_*.npz); the GPU tests use it as the yardstick that travels with the repository.
"""
from __future__ import annotations

import math

import numpy as np

import oracle

POINTS, NORMALS = "point_cloud", "deflectometry"


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def synthetic_facet(n_points, seed, width=1.6, height=1.3):
    """A canted, slightly paraboloidal facet with a few sinusoidal dents of ~1e-4 m, sampled at random (non-grid) positions:
    ``(points [N,4], normals [N,4])`` in float32, analytic unit normals."""
    rng = np.random.default_rng(seed)
    x = (rng.random(n_points) - 0.5) * width
    y = (rng.random(n_points) - 0.5) * height
    cant = rng.normal(0.0, 8e-3, 2)
    focal = 40.0 + 20.0 * rng.random()
    z = cant[0] * x + cant[1] * y + (x * x + y * y) / (4.0 * focal)
    zx = cant[0] + x / (2.0 * focal)
    zy = cant[1] + y / (2.0 * focal)
    for _ in range(3):
        amp, kx, ky = 1e-4 * (0.5 + rng.random()), 2.0 + 6.0 * rng.random(), 2.0 + 6.0 * rng.random()
        px, py = 2 * math.pi * rng.random(2)
        z += amp * np.sin(kx * x + px) * np.sin(ky * y + py)
        zx += amp * kx * np.cos(kx * x + px) * np.sin(ky * y + py)
        zy += amp * ky * np.sin(kx * x + px) * np.cos(ky * y + py)
    nrm = np.stack([-zx, -zy, np.ones_like(zx)], axis=1)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    points = np.concatenate([np.stack([x, y, z], axis=1), np.ones((n_points, 1))], axis=1).astype(np.float32)
    normals = np.concatenate([nrm, np.zeros((n_points, 1))], axis=1).astype(np.float32)
    return points, normals


def normalize_points(xy):
    """coordinates.normalize_points in the array's dtype."""
    dt = xy.dtype.type
    rng = xy - xy.min(axis=0)
    return (rng + dt(1e-5)) / (rng + dt(2e-5)).max(axis=0)


def linspace(start, end, steps, dtype):
    """torch.linspace on the CPU: symmetric about the middle, every value one fused multiply-add (for float32: the product in
    double is exact, the sum is rounded once more to double - a double rounding that can differ from a true fma only when the
    double sum is itself a tie, which 24-bit operands of this size do not produce)."""
    dt = np.dtype(dtype).type
    start, end = dt(start), dt(end)
    step = dt((end - start) / dt(steps - 1))
    out = np.empty(steps, dtype=dtype)
    for i in range(steps):
        # (float64: the plain formula - a last-bit difference there is far below what the fp64 runs are used for)
        out[i] = float(start) + float(step) * i if i < steps // 2 else float(end) - float(step) * (steps - i - 1)
    return out


def initial_net(points, nu, nv):
    """surface_generator.py:148-174 in the points' dtype."""
    dt = points.dtype
    two = dt.type(2)
    w = points[:, 0].max() - points[:, 0].min()
    h = points[:, 1].max() - points[:, 1].min()
    cp = np.zeros((nu, nv, 3), dtype=dt)
    cp[..., 0] = linspace(-w / two, w / two, nu, dt)[:, None]
    cp[..., 1] = linspace(-h / two, h / two, nv, dt)[None, :]
    return cp


def loss_and_grad(cp, uv, targets, degrees, method):
    """MSELoss (mean over N*4 components) of the surface points / normals at ``uv [N,2]`` against ``targets [N,4]`` and its
    gradient w.r.t. ``cp [nu,nv,3]``, in cp's dtype.  Returns ``(loss, grad, points, normals)``."""
    dt = cp.dtype
    pts, nrm = oracle.nurbs_fwd(cp[None, None], np.ascontiguousarray(uv, dtype=dt)[None, None], degrees)
    value = pts if method == POINTS else nrm
    res = value[0, 0] - targets.astype(dt)
    numel = res.size
    loss = dt.type(np.sum(res.astype(np.float64) ** 2) / numel) if dt == np.float32 else np.sum(res * res) / numel
    g = (dt.type(2.0 / numel) * res)[None, None]
    zero = np.zeros_like(g)
    grad = oracle.nurbs_bwd(cp[None, None], np.ascontiguousarray(uv, dtype=dt)[None, None], degrees,
                            g if method == POINTS else zero, zero if method == POINTS else g)
    return loss, grad[0, 0], pts[0, 0], nrm[0, 0]


class Plateau:
    """torch.optim.lr_scheduler.ReduceLROnPlateau.step in Python floats."""

    def __init__(self, lr, mode="min", factor=0.1, patience=10, threshold=1e-4, threshold_mode="rel", cooldown=0, min_lr=0.0, eps=1e-8):
        self.lr, self.mode, self.factor, self.patience, self.threshold = float(lr), mode, factor, patience, threshold
        self.threshold_mode, self.cooldown, self.min_lr, self.eps = threshold_mode, cooldown, min_lr, eps
        self.best = math.inf if mode == "min" else -math.inf
        self.num_bad_epochs = self.cooldown_counter = 0

    def step(self, metric):
        cur = float(metric)
        if self.mode == "min":
            better = cur < self.best * (1.0 - self.threshold) if self.threshold_mode == "rel" else cur < self.best - self.threshold
        else:
            better = cur > self.best * (self.threshold + 1.0) if self.threshold_mode == "rel" else cur > self.best + self.threshold
        if better:
            self.best, self.num_bad_epochs = cur, 0
        else:
            self.num_bad_epochs += 1
        if self.cooldown_counter > 0:
            self.cooldown_counter -= 1
            self.num_bad_epochs = 0
        if self.num_bad_epochs > self.patience:
            new_lr = max(self.lr * self.factor, self.min_lr)
            if self.lr - new_lr > self.eps:
                self.lr = new_lr
            self.cooldown_counter, self.num_bad_epochs = self.cooldown, 0


def adam_step(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """_single_tensor_adam in the arrays' dtype (in place)."""
    dt = p.dtype.type
    m += (g - m) * dt(1.0 - beta1)
    v *= dt(beta2)
    v += (dt(1.0 - beta2) * g) * g
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    denom = np.sqrt(v) / dt(math.sqrt(bc2)) + dt(eps)
    p -= dt(lr / bc1) * (m / denom)


def fit(points, normals, nu, nv, degrees, method, dtype=np.float32, lr=1e-3, plateau=None, tolerance=1e-10, max_epoch=400,
        record=()):
    """The reference's loop.  Returns a dict: ``uv``, ``cp0``, ``cp`` (final), ``epochs_run``, ``loss [E]``, ``lr [E]`` (the
    rate each epoch stepped with) and, for the epochs in ``record``, ``cp_at`` / ``grad_at`` (before that epoch's update)."""
    pts = points.astype(dtype)
    uv = normalize_points(pts[:, :2])
    cp = initial_net(pts, nu, nv)
    out = dict(uv=uv, cp0=cp.copy(), loss=[], lr=[], cp_at={}, grad_at={})
    targets = (points if method == POINTS else normals).astype(dtype)
    m, v = np.zeros_like(cp), np.zeros_like(cp)
    sched = Plateau(lr, **plateau) if plateau is not None else None
    loss, epoch = math.inf, 0
    tol = np.float32(tolerance) if dtype == np.float32 else tolerance
    while loss > tol and epoch <= max_epoch:
        loss, grad, _, _ = loss_and_grad(cp, uv, targets, degrees, method)
        rate = sched.lr if sched is not None else lr
        if epoch in record:
            out["cp_at"][epoch], out["grad_at"][epoch] = cp.copy(), grad.copy()
        out["loss"].append(float(loss))
        out["lr"].append(rate)
        adam_step(cp, grad, m, v, epoch + 1, rate)
        if sched is not None:
            sched.step(abs(float(loss)))
        epoch += 1
    out.update(cp=cp, epochs_run=epoch, loss=np.asarray(out["loss"]), lr=np.asarray(out["lr"]))
    return out
