"""Host tests (no device) of tests/epoch_ops_ref.py - the references that tests/test_gpu_epoch_ops.py holds ``art_align_fwd`` /
``art_align_bwd``, ``art_reflect``, ``art_per_target_sum`` and ``art_adam_step`` to - and of those entry points' argument checks.

Three things are shown here.  The references are right: each fp64 reference equals torch's fp64 evaluation of the operation it
restates (``@`` and autograd, ``index_add_``, the reflect formula, ``torch.optim.Adam``).  The bounds are honest: on every case
that the GPU file runs, the fp32 op-for-op restatement (for the orientation gradient: a simulation of the kernel's summation
tree) stays within the stated bound of the fp64 reference - a bound that an exact fp32 evaluation could miss would say nothing
about a kernel.  And the entry points refuse what they must before they look at a pointer or launch anything.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import epoch_ops_ref as ref

F64_SLACK = 64 * 2.0 ** -53         # an fp64 reference against torch's fp64: a few dozen roundings of either, relative to the sum of magnitudes


def worst(err, bound):
    """Largest error / bound over the entries (0 / 0 counts as 0; an error where the bound is 0 as infinite)."""
    err, bound = np.abs(np.asarray(err, np.float64)), np.asarray(bound, np.float64)
    ratio = np.divide(err, bound, out=np.where(err > 0, np.inf, 0.0), where=bound > 0)
    return float(ratio.max()) if ratio.size else 0.0


# ------------------------------------------------------------------------------------------------ the references are right
@pytest.mark.parametrize("H,P", [(1, 1), (3, 65), (2, 1025)])
def test_align_reference_equals_torch_fp64(H, P):
    points, normals, M, g_p, g_n = ref.align_inputs(H, P)
    x, y, m = (torch.from_numpy(a.astype(np.float64)).requires_grad_(True) for a in (points, normals, M))
    out_p, out_n = x @ m.transpose(1, 2), y @ m.transpose(1, 2)
    (out_p * torch.from_numpy(g_p.astype(np.float64)) + out_n * torch.from_numpy(g_n.astype(np.float64))).sum().backward()
    for got, want in ((ref.align_fwd64(points, M), out_p), (ref.align_fwd64(normals, M), out_n),
                      (ref.align_bwd64(g_p, M), x.grad), (ref.align_bwd64(g_n, M), y.grad),
                      (ref.align_gm64(points, normals, g_p, g_n), m.grad)):
        value, bound = got
        assert value.shape == tuple(want.shape)
        assert worst(value - want.detach().numpy(), bound / ref.U * F64_SLACK) <= 1.0       # (bound / u = the sum of magnitudes x count)


def test_reflect_reference_equals_the_torch_formula():
    for H, P in ref.REFLECT_SHAPES:
        incident, normals = ref.reflect_inputs(H, P)
        i, n = torch.from_numpy(incident.astype(np.float64))[:, None, :], torch.from_numpy(normals.astype(np.float64))
        want = i - 2 * torch.sum(i * n, dim=-1).unsqueeze(-1) * n                  # geometry.reflect
        value, bound = ref.reflect64(incident, normals)
        assert worst(value - want.numpy(), bound / ref.U * F64_SLACK) <= 1.0


def test_per_target_sum_reference_equals_index_add():
    for npix, H, T in ref.PER_TARGET_SMALL:
        bitmaps, idx = ref.per_target_inputs(npix, H, T)
        ok = (idx >= 0) & (idx < T)
        want = torch.zeros(T, npix, dtype=torch.float64).index_add_(0, torch.from_numpy(idx[ok]), torch.from_numpy(bitmaps[ok].astype(np.float64)))
        mags = ref.per_target_sum64(np.abs(bitmaps), idx, T)
        assert worst(ref.per_target_sum64(bitmaps, idx, T) - want.numpy(), mags * H * 2.0 ** -53) <= 1.0
        if T > 1:
            assert not (idx == T - 1).any() and not ref.per_target_sum32(bitmaps, idx, T)[T - 1].any()
        if H >= 3:
            assert (idx == -1).any() and (idx == T).any()
        unaimed = ref.per_target_unaimed(H, T)
        assert not ((unaimed >= 0) & (unaimed < T)).any() and not ref.per_target_sum32(bitmaps, unaimed, T).any()


ADAM_TORCH_SETTINGS = [dict(lr=1e-3), dict(lr=1e-2, weight_decay=0.1), dict(lr=1e-2, maximize=True),
                       dict(lr=5e-3, weight_decay=0.05, maximize=True, betas=(0.8, 0.9), eps=1e-6), dict(lr=1e-3, betas=(0.0, 0.0))]


@pytest.mark.parametrize("steps", [1, 12])
@pytest.mark.parametrize("kw", ADAM_TORCH_SETTINGS, ids=lambda kw: "-".join(k for k in kw if k != "lr") or "default")
def test_adam_reference_equals_torch_adam_fp64(kw, steps):
    """``adam_step64`` with the UNROUNDED scalars follows ``torch.optim.Adam`` in fp64 (single-tensor path) - the two differ in a
    handful of fp64 roundings per step (torch divides by sqrt(bc2) where the entry point multiplies by its reciprocal, its lerp
    has two forms): 16 roundings a step, relative to the magnitudes that enter each sum, with a margin of 8 -, and at every
    step of that trajectory the variant with the scalars rounded to fp32 as ``art_adam_step`` rounds them stays within the Adam
    bound of the unrounded one: each scalar's rounding is one more relative error of u on a term that the bound counts."""
    n = 257
    p0, _, _, _ = ref.adam_inputs(n, seed=1)
    rng = np.random.default_rng(5)
    tp = torch.from_numpy(p0.astype(np.float64)).requires_grad_(True)
    opt = torch.optim.Adam([tp], foreach=False, **kw)
    p, m, v = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    sched = dict(lr=kw["lr"], betas=kw.get("betas", (0.9, 0.999)), eps=kw.get("eps", 1e-8), weight_decay=kw.get("weight_decay", 0.0),
                 maximize=kw.get("maximize", False))
    tol = 8 * 16 * 2.0 ** -53
    for k in range(1, steps + 1):
        g = ref.spread(rng, n, -6, 2).astype(np.float64)
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        exact = ref.adam_scalars(step=k, rounded=False, **sched)
        rounded = ref.adam_scalars(step=k, rounded=True, **sched)
        p_r, m_r, v_r = ref.adam_step64(p, g, m, v, rounded)
        b_p, b_m, b_v, _ = ref.adam_bounds(p, g, m, v, rounded)
        p1, m1, v1 = ref.adam_step64(p, g, m, v, exact)
        assert worst(p_r - p1, b_p) <= 1.0 and worst(m_r - m1, b_m) <= 1.0 and worst(v_r - v1, b_v) <= 1.0, k
        # ... and the bounds are not vacuous: they stay at rounding level of the quantities they bound
        assert (b_m <= 16 * ref.U * (np.abs(m) + np.abs(g) + np.abs(p)) + 1e-300).all()
        p, m, v = p1, m1, v1
        state = opt.state[tp]
        gr_mag = np.abs(g) + kw.get("weight_decay", 0.0) * np.abs(p)
        assert np.abs(m - state["exp_avg"].numpy()).max() <= k * tol * (np.abs(m) + gr_mag).max()
        assert np.abs(v - state["exp_avg_sq"].numpy()).max() <= k * tol * (v + gr_mag ** 2).max()
        # the update is step_size m'/denom with |m'/denom| of order 1 / sqrt(1 - beta2) at most: errors relative to max|p| + that
        assert np.abs(p - tp.detach().numpy()).max() <= k * tol * (np.abs(p).max() + 40.0 * kw["lr"] / (1 - sched["betas"][0] ** k))
    assert int(opt.state[tp]["step"]) == steps


@pytest.mark.parametrize("nets,nu,nv", ref.ADAM_LOCK_SHAPES)
def test_lock_rule_equals_zeroing_the_edge_gradient(nets, nu, nv):
    """``adam_locked`` against the recipe of tests/test_gpu_optim.py (surface_reconstructor.py:1155-1224): u and v of the first /
    last row and column of every net."""
    g = np.ones((nets, nu, nv, 3))
    for edge in (g[:, 0], g[:, -1], g[:, :, 0], g[:, :, -1]):
        edge[..., :2] = 0
    locked = ref.adam_locked(g.size, nu, nv)
    assert np.array_equal(locked, g.reshape(-1) == 0)
    assert not ref.adam_locked(g.size, 0, 0).any()
    p, grad, m, v = ref.adam_inputs(g.size, seed=2)
    s = ref.adam_scalars(lr=1e-2, weight_decay=0.1, step=3)
    for a, b in zip(ref.adam_step64(p, grad, m, v, s, locked), ref.adam_step64(p, grad * g.reshape(-1), m, v, s)):
        assert np.array_equal(a, b)


def test_plans_restate_the_entry_points():
    assert ref.plan_per_target_sum(1 << 20, 0x1000, 0x2000) == 4
    assert ref.plan_per_target_sum((1 << 20) + 4, 0x1000, 0x2000) == 4
    assert ref.plan_per_target_sum((1 << 20) + 2, 0x1000, 0x2000) == 1
    assert ref.plan_per_target_sum((1 << 20) - 4, 0x1000, 0x2000) == 1
    assert ref.plan_per_target_sum(1 << 20, 0x1004, 0x2000) == 1 and ref.plan_per_target_sum(1 << 20, 0x1000, 0x2008) == 1
    assert ref.plan_adam(1024, 0, 16, 32, 48) == (256, 0)
    assert ref.plan_adam(1027, 0, 16, 32, 48) == (256, 1)
    assert ref.plan_adam(3, 0, 16, 32, 48) == (0, 1)
    assert ref.plan_adam(1024, 4, 16, 32, 48) == (0, 256) and ref.plan_adam(1027, 0, 16, 32, 52) == (0, 257)


# -------------------------------------------------------------------------------------------------- the bounds are honest
@pytest.mark.parametrize("H,P", ref.ALIGN_SHAPES)
def test_align_bounds_hold_for_the_fp32_restatement(H, P):
    points, normals, M, g_p, g_n = ref.align_inputs(H, P)
    assert all((a != 0).all() and (np.abs(a[a != 0]) > 1e-30).all() for a in (points, normals, M, g_p, g_n))     # full matrices, no denormals
    ratios = []
    for x in (points, normals):
        value, bound = ref.align_fwd64(x, M)
        ratios.append(worst(ref.align_fwd32(x, M) - value, bound))
    for g in (g_p, g_n):
        value, bound = ref.align_bwd64(g, M)
        ratios.append(worst(ref.align_bwd32(g, M) - value, bound))
    value, bound = ref.align_gm64(points, normals, g_p, g_n)
    ratios.append(worst(ref.align_gm_tree32(points, normals, g_p, g_n) - value, bound))
    print(f"align ({H},{P}): error / bound  apply {max(ratios[:4]):.3f}  orientation gradient {ratios[4]:.3f} (depth {ref.align_gm_depth(P)})")
    assert max(ratios) <= 1.0


def test_align_gm_depth_follows_the_tree():
    assert [ref.align_gm_depth(P) for P in (0, 1, 1024, 1025, 2049, 3073)] == [25, 25, 25, 28, 31, 34]


@pytest.mark.parametrize("p", ref.ALIGN_SENTINEL_POINTS)
def test_align_sentinel_is_what_the_tree_gives(p):
    """One non-zero upstream gradient: the simulated tree returns the single rounded products exactly, whatever lane and wave the
    point falls into (0 and 63: first wave; 64; 1023: last wave; 1024, 2048: second and third iteration of thread 0)."""
    H, P = ref.ALIGN_SENTINEL_SHAPE
    points, normals, _, g_p, g_n = ref.align_inputs(H, P)
    only_p, only_n = np.zeros_like(g_p), np.zeros_like(g_n)
    only_p[H - 1, p], only_n[H - 1, p] = g_p[H - 1, p], g_n[H - 1, p]
    got = ref.align_gm_tree32(points, normals, only_p, only_n)
    assert np.array_equal(got[H - 1], ref.align_gm_single32(points, normals, g_p, g_n, H - 1, p)) and got[H - 1].all()
    assert not got[:H - 1].any()


def test_reflect_bound_holds_for_the_fp32_restatement():
    for H, P in ref.REFLECT_SHAPES:
        incident, normals = ref.reflect_inputs(H, P)
        assert (incident != 0).all() and (normals != 0).all()
        assert H == 1 or not np.array_equal(incident[0], incident[1])
        value, bound = ref.reflect64(incident, normals)
        ratio = worst(ref.reflect32(incident, normals) - value, bound)
        print(f"reflect ({H},{P}): error / bound {ratio:.3f}")
        assert ratio <= 1.0


@pytest.mark.parametrize("npix,H,T", ref.PER_TARGET_SMALL + ref.PER_TARGET_LARGE)
def test_per_target_sum_restatement_is_within_the_summation_bound(npix, H, T):
    """The index-order fp32 sum against the fp64 sum: (n - 1) u sum|x| over the n <= H bitmaps of a target (any order)."""
    bitmaps, idx = ref.per_target_inputs(npix, H, T)
    bound = (H - 1) * ref.U * ref.per_target_sum64(np.abs(bitmaps), idx, T)
    ratio = worst(ref.per_target_sum32(bitmaps, idx, T) - ref.per_target_sum64(bitmaps, idx, T), bound)
    print(f"per-target sum ({npix},{H},{T}): error / bound {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("name", list(ref.ADAM_SETTINGS))
def test_adam_bounds_hold_for_the_fp32_restatement(name):
    kw = ref.ADAM_SETTINGS[name]
    worst_p = worst_m = worst_v = worst_local = 0.0
    for n in ref.ADAM_SIZES:
        for before in ref.ADAM_STEPS_BEFORE:
            p, g, m, v = ref.adam_inputs(n, seed=before)
            s = ref.adam_scalars(step=before + 1, **kw)
            p32, m32, v32 = ref.adam_step32(p, g, m, v, s)
            p64, m64, v64 = ref.adam_step64(p, g, m, v, s)
            b_p, b_m, b_v, b_local = ref.adam_bounds(p, g, m, v, s)
            worst_p, worst_m, worst_v = max(worst_p, worst(p32 - p64, b_p)), max(worst_m, worst(m32 - m64, b_m)), max(worst_v, worst(v32 - v64, b_v))
            worst_local = max(worst_local, worst(p32 - ref.adam_p_from_moments64(p, m32, v32, s), b_local))
            if n >= 5 and kw.get("weight_decay", 0.0) == 0.0:
                zero = (g == 0) & (m == 0) & (v == 0)
                assert zero.any() and np.array_equal(p32[zero], p[zero]) and not m32[zero].any() and not v32[zero].any()
    print(f"adam {name}: error / bound  p {worst_p:.3f}  m {worst_m:.3f}  v {worst_v:.3f}  p from its own moments {worst_local:.3f}")
    assert max(worst_p, worst_m, worst_v, worst_local) <= 1.0


@pytest.mark.parametrize("nets,nu,nv", ref.ADAM_LOCK_SHAPES)
def test_adam_bounds_hold_with_the_lock(nets, nu, nv):
    n = nets * nu * nv * 3
    locked = ref.adam_locked(n, nu, nv)
    for wd in (0.0, 0.1):
        p, g, m, v = ref.adam_inputs(n, seed=3)
        s = ref.adam_scalars(lr=1e-2, weight_decay=wd, step=2)
        got, want, bounds = ref.adam_step32(p, g, m, v, s, locked), ref.adam_step64(p, g, m, v, s, locked), ref.adam_bounds(p, g, m, v, s, locked)
        assert max(worst(a - b, c) for a, b, c in zip(got, want, bounds)) <= 1.0


# ------------------------------------------------------------------------------------ argument checks need no device
INT_MAX = 2 ** 31 - 1


def test_epoch_ops_argument_checks_need_no_device():
    from artist_amd import _lib
    lib = _lib.lib()
    OK, EINVAL = _lib.ART_OK, _lib.ART_EINVAL
    p = ctypes.c_void_p(16)                              # (never dereferenced: every call below returns first)
    odd = ctypes.c_void_p(20)                            # a contiguous view at a storage offset of one float
    # zero sizes launch nothing and look at no pointer
    assert lib.art_align_fwd(None, None, None, 0, 5, None, None, None) == OK
    assert lib.art_align_fwd(None, None, None, 4, 0, None, None, None) == OK
    assert lib.art_align_bwd(None, None, None, None, None, 0, 5, None, None, None, None) == OK
    assert lib.art_align_bwd(None, None, None, None, None, 4, 0, None, None, None, None) == OK     # (no grad_orientation to zero)
    assert lib.art_reflect(None, None, 0, 3, None, None) == OK
    assert lib.art_reflect(None, None, 3, 0, None, None) == OK
    assert lib.art_per_target_sum(None, None, 5, 0, 16, None, None) == OK
    assert lib.art_per_target_sum(None, None, 5, 2, 0, None, None) == OK
    assert lib.art_adam_step(None, None, None, None, 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0, 0, 0, None) == OK
    # negative sizes, whatever the pointers
    for H, P in ((-1, 4), (4, -1), (-1, 0), (0, -1)):
        assert lib.art_align_fwd(p, p, p, H, P, p, p, None) == EINVAL, (H, P)
        assert lib.art_align_bwd(p, p, p, p, p, H, P, p, p, p, None) == EINVAL, (H, P)
        assert lib.art_reflect(p, p, H, P, p, None) == EINVAL, (H, P)
    for H, T, npix in ((-1, 2, 16), (4, -1, 16), (4, 2, -1)):
        assert lib.art_per_target_sum(p, p, H, T, npix, p, None) == EINVAL, (H, T, npix)
    assert lib.art_adam_step(p, p, p, p, -1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0, 0, 0, None) == EINVAL
    assert lib.art_adam_step(p, p, p, p, 27, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0, -3, 3, None) == EINVAL
    assert lib.art_adam_step(p, p, p, p, 27, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0, 3, -3, None) == EINVAL
    # null pointers with work to do
    for k in (0, 1, 2, 5, 6):
        args = [p, p, p, 4, 4, p, p, None]
        args[k] = None
        assert lib.art_align_fwd(*args) == EINVAL, k
    for k in (2, 3, 4, 7, 8):
        args = [p, p, p, p, p, 4, 4, p, p, p, None]
        args[k] = None
        assert lib.art_align_bwd(*args) == EINVAL, k
    assert lib.art_align_bwd(None, p, p, p, p, 4, 4, p, p, p, None) == EINVAL            # the orientation gradient needs the inputs
    assert lib.art_align_bwd(p, None, p, p, p, 4, 4, p, p, p, None) == EINVAL
    for k in (0, 1, 4):
        args = [p, p, 4, 4, p, None]
        args[k] = None
        assert lib.art_reflect(*args) == EINVAL, k
    assert lib.art_per_target_sum(None, p, 4, 2, 16, p, None) == EINVAL
    assert lib.art_per_target_sum(p, None, 4, 2, 16, p, None) == EINVAL
    assert lib.art_per_target_sum(p, p, 4, 2, 16, None, None) == EINVAL
    assert lib.art_per_target_sum(None, None, 0, 2, 16, None, None) == EINVAL            # (H = 0 still zero-fills out)
    for k in range(4):
        args = [p, p, p, p, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0, 0, 0, None]
        args[k] = None
        assert lib.art_adam_step(*args) == EINVAL, k
    # sizes that the launch geometry or an int in a kernel cannot hold
    assert lib.art_per_target_sum(p, p, 4, 65536, 16, p, None) == EINVAL
    assert lib.art_per_target_sum(p, p, INT_MAX + 1, 2, 16, p, None) == EINVAL             # H is an int in the kernels
    assert lib.art_per_target_sum(p, p, 1 << 40, 2, 16, p, None) == EINVAL                 # (2^40 narrows to 0: refused, not narrowed)
    assert lib.art_per_target_sum(p, p, 4, 2, 256 * (INT_MAX + 1), p, None) == EINVAL      # blocks > INT_MAX
    assert lib.art_align_fwd(p, p, p, 4, INT_MAX + 1, p, p, None) == EINVAL                # P is an int in the kernels
    assert lib.art_align_bwd(p, p, p, p, p, 4, INT_MAX + 1, p, p, p, None) == EINVAL
    assert lib.art_align_fwd(p, p, p, (1 << 30) + 1, 257, p, p, None) == EINVAL            # H * tiles = 2^31 + 2 > INT_MAX
    assert lib.art_align_bwd(p, p, p, p, p, (1 << 30) + 1, 257, p, p, p, None) == EINVAL
    assert lib.art_reflect(p, p, 1 << 31, 256, p, None) == EINVAL                          # blocks > INT_MAX
    assert lib.art_adam_step(p, p, p, p, 1024 * (INT_MAX + 1), 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0, 0, 0, None) == EINVAL
    # Adam's own rules
    good = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, step=1, lock=(0, 0), n=108)

    def adam_code(**kw):
        a = dict(good, **kw)
        return lib.art_adam_step(p, p, p, p, a["n"], a["lr"], a["beta1"], a["beta2"], a["eps"], a["wd"], a["step"], 0, a["lock"][0], a["lock"][1], None)
    for bad in (dict(step=0), dict(step=-1), dict(beta1=1.0), dict(beta1=-0.1), dict(beta1=float("nan")), dict(beta2=1.0),
                dict(beta2=-1e-9), dict(beta2=float("nan")), dict(beta2=1.5), dict(eps=-1e-8), dict(eps=float("nan")),
                dict(lock=(3, 0)), dict(lock=(0, 3)), dict(lock=(5, 3)), dict(lock=(3, 3), n=28), dict(lock=(4097, 1), n=4097 * 3),
                dict(lock=(1, 4097), n=4097 * 3), dict(lock=(1, 1), n=3 * (1 << 30))):
        assert adam_code(**bad) == EINVAL, bad
    # alignment (section "Alignment" of art_align_* / art_reflect in include/artist_hip.h): every [.,.,4] tensor, before any launch
    for k in (0, 1, 5, 6):
        args = [p, p, p, 4, 4, p, p, None]
        args[k] = odd
        assert lib.art_align_fwd(*args) == EINVAL, k
    for k in (0, 1, 3, 4, 7, 8):
        args = [p, p, p, p, p, 4, 4, p, p, p, None]
        args[k] = odd
        assert lib.art_align_bwd(*args) == EINVAL, k
    for k in (0, 1, 4):
        args = [p, p, 4, 4, p, None]
        args[k] = odd
        assert lib.art_reflect(*args) == EINVAL, k
    for k in (3, 4, 7, 8):                                 # without grad_orientation, points and normals are not read: any pointer will do
        args = [odd, odd, p, p, p, 4, 4, p, p, None, None]
        args[k] = odd
        assert lib.art_align_bwd(*args) == EINVAL, k
    # ... and an empty batch asks nothing of a pointer's alignment
    assert lib.art_align_fwd(odd, odd, odd, 4, 0, odd, odd, None) == OK
    assert lib.art_reflect(odd, odd, 3, 0, odd, None) == OK
