"""GPU tests (``-m gpu``) of the four small entry points that every epoch of every optimiser runs - ``art_align_fwd`` /
``art_align_bwd`` (``ops.align_surfaces``), ``art_reflect`` (``ops.reflect_directions``), ``art_per_target_sum``
(``ops.per_target_sum``) and ``art_adam_step`` (``optim.Adam``) - at every branch that the shape, the alignment or the layout of a
call selects, against tests/epoch_ops_ref.py.

Rule (the module docstring of epoch_ops_ref.py has the derivations, tests/test_epoch_ops_host.py shows that each bound holds for
an exact fp32 evaluation of every case below): where the order of the fp32 operations is the contract - the align apply forward
and backward, reflect, the per-target sum - the kernel gives the BITS of the op-for-op fp32 restatement; elsewhere - the
orientation gradient's summation tree, Adam with its ``sqrtf`` and ``/`` - it stays within a rounding bound derived from the
operations it performs, against fp64 from the same fp32 inputs.  Nothing here was tuned to an output of the kernels.  Paths that
must agree (4-pixel and 1-pixel per-target kernels, 16-byte and element-wise Adam) are compared bit for bit on the same data, the
path being chosen by the alignment of a view; ``epoch_ops_ref.plan_*`` restate the entry points' conditions so that a test can
say which path its call is meant to take.  A misaligned view never reaches a float4 kernel: the align and reflect wrappers copy
it (their entry points refuse it, tests/test_epoch_ops_host.py).

Every test prints its largest error / bound.

Measured on an MI355X (114 tests, 5 s), largest error / bound per operation: align apply 0.846 (1 x 3073; bit-equal everywhere, so
this is the fp32 restatement's own distance from fp64, the figure of the host test); orientation gradient 0.059 (3 x 65, depth 25;
every shape lands on the figure of the host test's simulated tree); reflect 0.906 (7 x 37, bit-equal); per-target sum bit-equal on
all 18 cases and both kernels (at most 0.12 of the any-order summation bound against fp64, which is not asserted: it could not
tell one order from another); Adam p 0.496, m 0.394, v 0.306, p against fp64 from the kernel's own moments 0.496 - over 11 sizes x
3 step numbers x 5 settings.

Seeded mistakes, one build each (an edited copy of one source file through the Makefile's ``SRC_<file>=copy.hip`` variant, loaded
with ``ARTIST_HIP_LIB``; all memory-safe, none kept):
1. ``align_bwd_kernel`` applies ``M^T``: all 12 cases of ``test_align_apply_gives_the_bits_of_the_fp32_restatement`` fail - no bit
   equality, 6.1e6 bounds at 1 x 1 and 1.8e9 at 3 x 2049.
2. ``align_gm_kernel`` leaves out the last wave's partial sum: ``test_align_orientation_gradient_is_within_the_tree_bound`` fails
   at every shape that reaches the last wave (P = 1023: 45 027 bounds, 1024: 30 681, 1025: 45 327, 2049: 104 823, 3073: 17 775) and
   ``test_align_orientation_gradient_of_a_single_point[1023]`` gets zeros.
3. ``per_target_sum_kernel<4>`` adds its eight in-flight values in reverse order: the four 4-pixel cases of
   ``test_per_target_sum_large_bitmaps`` fail with 452 244 to 520 659 of the 1 048 576 words of the aimed-at target different (the
   error stays inside every rounding bound: only bit equality sees it); the scalar kernel's cases pass.
4. The element-wise Adam path ignores the lock: ``test_adam_edge_lock_on_both_paths`` fails on all 14 element-wise cases and on
   the vector cases whose size is no multiple of 4 (1 x 3 x 3, 5 x 3 x 3: the tail thread) - 1 to 74 words differ from the
   zeroed-gradient recipe, the locked components are 1.6e6 bounds (p) away from the fp64 restatement.
5. ``adam_locked`` tests ``col == nv`` for ``nv - 1``: the same test fails on both paths for every shape whose last column
   holds a row that is no edge row (nu > 2 and nv > 1: 16 cases; 7.1e5 bounds in p).
"""
import functools

import numpy as np
import pytest
import torch

import epoch_ops_ref as ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def n(x):
    return x.detach().cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def worst(err, bound):
    err, bound = np.abs(np.asarray(err, np.float64)), np.asarray(bound, np.float64)
    ratio = np.divide(err, bound, out=np.where(err > 0, np.inf, 0.0), where=bound > 0)
    return float(ratio.max()) if ratio.size else 0.0


def offset_view(x, like=None):
    """``x`` (numpy or tensor) as a contiguous device view whose first element lies one float past a 16-byte boundary."""
    x = t(x) if isinstance(x, np.ndarray) else x
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=DEV)
    view = buf[1:].view(x.shape)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return view


def poison_allocator(shape):
    """Leave NaNs in the block that the next ``torch.empty`` of this size will be given: an output that is not fully written shows."""
    junk = torch.full(shape, float("nan"), device=DEV)
    del junk


# ---------------------------------------------------------------------------------------------------------------- align
def align_call(points, normals, M, g_p, g_n, orientation_grad=True):
    """(out_points, out_normals, grad_points, grad_normals, grad_orientation or None) of ``ops.align_surfaces`` on tensors."""
    from artist_amd import align_surfaces
    x, y = points.detach().requires_grad_(True), normals.detach().requires_grad_(True)
    m = M.detach().requires_grad_(orientation_grad)
    out_p, out_n = align_surfaces(x, y, m)
    torch.autograd.backward([out_p, out_n], [g_p, g_n])
    return out_p.detach(), out_n.detach(), x.grad, y.grad, m.grad


@functools.lru_cache(maxsize=None)
def align_case(H, P):
    inputs = ref.align_inputs(H, P)
    return inputs, tuple(n(a) for a in align_call(*(t(a) for a in inputs)))


@pytest.mark.parametrize("H,P", ref.ALIGN_SHAPES)
def test_align_apply_gives_the_bits_of_the_fp32_restatement(H, P):
    (points, normals, M, g_p, g_n), (out_p, out_n, gx, gy, _) = align_case(H, P)
    ratios, equal = [], []
    for got, x, restated, reference in ((out_p, points, ref.align_fwd32, ref.align_fwd64), (out_n, normals, ref.align_fwd32, ref.align_fwd64),
                                        (gx, g_p, ref.align_bwd32, ref.align_bwd64), (gy, g_n, ref.align_bwd32, ref.align_bwd64)):
        value, bound = reference(x, M)
        ratios.append(worst(got - value, bound))
        equal.append(same_bits(got, restated(x, M)))
    print(f"align apply ({H},{P}): largest error / bound {max(ratios):.3f}, bit-equal {equal}")
    assert all(equal) and max(ratios) <= 1.0


@pytest.mark.parametrize("H,P", ref.ALIGN_SHAPES)
def test_align_orientation_gradient_is_within_the_tree_bound(H, P):
    inputs, (_, _, _, _, gm) = align_case(H, P)
    points, normals, M, g_p, g_n = inputs
    value, bound = ref.align_gm64(points, normals, g_p, g_n)
    ratio = worst(gm - value, bound)
    print(f"align orientation gradient ({H},{P}): error / bound {ratio:.4f} (depth {ref.align_gm_depth(P)})")
    assert gm.shape == (H, 4, 4) and ratio <= 1.0
    again = n(align_call(*(t(a) for a in inputs))[4])
    assert same_bits(gm, again)                                             # a fixed summation order: bit-reproducible


@pytest.mark.parametrize("p", ref.ALIGN_SENTINEL_POINTS)
def test_align_orientation_gradient_of_a_single_point(p):
    """The upstream gradient is non-zero at ONE point of the last heliostat: its orientation gradient is the single rounded
    products of that point - a term that the tree drops, or takes from another point or heliostat, has nothing to hide behind -
    and the other heliostats' gradients are exact zeros."""
    H, P = ref.ALIGN_SENTINEL_SHAPE
    points, normals, M, g_p, g_n = ref.align_inputs(H, P)
    only_p, only_n = np.zeros_like(g_p), np.zeros_like(g_n)
    only_p[H - 1, p], only_n[H - 1, p] = g_p[H - 1, p], g_n[H - 1, p]
    gm = n(align_call(t(points), t(normals), t(M), t(only_p), t(only_n))[4])
    want = ref.align_gm_single32(points, normals, g_p, g_n, H - 1, p)
    assert want.all() and np.array_equal(gm[H - 1], want)
    assert not gm[:H - 1].any()


@pytest.mark.parametrize("H,P", [(3, 65), (2, 1025)])
def test_align_without_orientation_gradient_keeps_the_other_bits(H, P):
    inputs, (out_p, out_n, gx, gy, _) = align_case(H, P)
    got = align_call(*(t(a) for a in inputs), orientation_grad=False)
    assert got[4] is None
    for a, b in zip(got[:4], (out_p, out_n, gx, gy)):
        assert same_bits(n(a), b)


def test_align_layouts_and_dtypes_give_the_bits_of_aligned_fp32_copies():
    H, P = 2, 255
    inputs, base = align_case(H, P)
    points, normals, M, g_p, g_n = (t(a) for a in inputs)
    # fp64 inputs: the values are the fp32 ones, every gradient comes back in its input's dtype
    got = align_call(points.double(), normals.double(), M.double(), g_p, g_n)
    assert [a.dtype for a in got] == [torch.float32, torch.float32, torch.float64, torch.float64, torch.float64]
    for a, b in zip(got, base):
        assert a.shape == b.shape and same_bits(n(a.float()), b)
    # points as a transposed, non-contiguous view; the gradient of the underlying [P,H,4] leaf has that shape
    from artist_amd import align_surfaces
    leaf = points.transpose(0, 1).contiguous().requires_grad_(True)
    out_p, out_n = align_surfaces(leaf.transpose(0, 1), normals, M)
    assert not leaf.transpose(0, 1).is_contiguous()
    torch.autograd.backward([out_p, out_n], [g_p, g_n])
    assert same_bits(n(out_p), base[0]) and leaf.grad.shape == (P, H, 4) and same_bits(n(leaf.grad.transpose(0, 1).contiguous()), base[2])
    # contiguous views at a storage offset of one float, inputs and upstream gradients alike: the wrapper hands the kernels aligned copies
    got = align_call(offset_view(points), offset_view(normals), offset_view(M), offset_view(g_p), offset_view(g_n))
    for a, b in zip(got, base):
        assert a.dtype == torch.float32 and same_bits(n(a), b)
    # one orientation expanded over the heliostats: the leaf's gradient is the sum of the two heliostats' (a + b: one rounding)
    single = M[:1].clone()
    tiled = tuple(n(a) for a in align_call(points, normals, single.expand(H, 4, 4).contiguous(), g_p, g_n))
    single.requires_grad_(True)
    out_p, out_n = align_surfaces(points, normals, single.expand(H, 4, 4))
    torch.autograd.backward([out_p, out_n], [g_p, g_n])
    assert same_bits(n(out_p), tiled[0]) and same_bits(n(out_n), tiled[1])
    assert single.grad.shape == (1, 4, 4) and same_bits(n(single.grad)[0], tiled[4][0] + tiled[4][1])


@pytest.mark.parametrize("H,P", [(0, 5), (4, 0)])
def test_align_of_an_empty_batch(H, P):
    """Like the batched matmul it replaces: empty outputs and gradients, and the orientation gradient of heliostats without points
    is the sum over nothing - zeros, fully written."""
    rng = np.random.default_rng(3)
    M = t(rng.standard_normal((H, 4, 4)).astype(np.float32))
    empty = torch.empty((H, P, 4), device=DEV)
    poison_allocator((H, 4, 4))
    out_p, out_n, gx, gy, gm = align_call(empty, empty.clone(), M, empty.clone(), empty.clone())
    assert out_p.shape == out_n.shape == gx.shape == gy.shape == (H, P, 4)
    assert gm.shape == (H, 4, 4) and not n(gm).any() and not np.isnan(n(gm)).any()


# -------------------------------------------------------------------------------------------------------------- reflect
@pytest.mark.parametrize("H,P", ref.REFLECT_SHAPES)
def test_reflect_gives_the_bits_of_the_fp32_restatement(H, P):
    from artist_amd.ops import reflect_directions
    incident, normals = ref.reflect_inputs(H, P)
    got = n(reflect_directions(t(incident), t(normals)))
    value, bound = ref.reflect64(incident, normals)
    ratio = worst(got - value, bound)
    print(f"reflect ({H},{P}): error / bound {ratio:.3f}")
    assert same_bits(got, ref.reflect32(incident, normals)) and ratio <= 1.0
    assert same_bits(n(reflect_directions(offset_view(incident), offset_view(normals))), got)
    assert same_bits(n(reflect_directions(t(incident).double(), t(normals).double())), got)


@pytest.mark.parametrize("H,P", ref.REFLECT_EMPTY_SHAPES)
def test_reflect_of_an_empty_batch(H, P):
    from artist_amd.ops import reflect_directions
    out = reflect_directions(torch.ones((H, 4), device=DEV), torch.ones((H, P, 4), device=DEV))
    assert out.shape == (H, P, 4) and out.dtype == torch.float32


# ------------------------------------------------------------------------------------------------------- per-target sum
def per_target_checked(bitmaps, idx, T, want, vec=None):
    """``ops.per_target_sum`` for int64 and int32 indices into an output block that held NaNs; both equal ``want`` bit for bit."""
    from artist_amd import per_target_sum
    for index in (t(idx), t(idx.astype(np.int32))):
        poison_allocator((T,) + tuple(bitmaps.shape[1:]))
        out = per_target_sum(bitmaps, index, T)
        if vec is not None:
            assert ref.plan_per_target_sum(int(np.prod(bitmaps.shape[1:])), bitmaps.data_ptr(), out.data_ptr()) == vec
        got = n(out)
        assert got.shape == want.shape and same_bits(got, want), int((bits(got) != bits(want)).sum())
    return got


@pytest.mark.parametrize("npix,H,T", ref.PER_TARGET_SMALL)
def test_per_target_sum_small_bitmaps(npix, H, T):
    bitmaps, idx = ref.per_target_inputs(npix, H, T)
    got = per_target_checked(t(bitmaps), idx, T, ref.per_target_sum32(bitmaps, idx, T), vec=1)
    if T > 1:
        assert not bits(got[T - 1]).any()                                   # nobody aims at it: +0.0f, written
    unaimed = ref.per_target_unaimed(H, T)
    assert not bits(per_target_checked(t(bitmaps), unaimed, T, np.zeros((T, npix), np.float32))).any()
    bound = (H - 1) * ref.U * ref.per_target_sum64(np.abs(bitmaps), idx, T)
    print(f"per-target sum ({npix},{H},{T}): bit-equal; error / summation bound against fp64 {worst(got - ref.per_target_sum64(bitmaps, idx, T), bound):.3f}")


@functools.lru_cache(maxsize=2)
def large_case(npix, H, T):
    bitmaps, idx = ref.per_target_inputs(npix, H, T)
    return bitmaps, idx, ref.per_target_sum32(bitmaps, idx, T)


@pytest.mark.parametrize("npix,H,T", ref.PER_TARGET_LARGE)
def test_per_target_sum_large_bitmaps(npix, H, T):
    """From 2^20 pixels on the entry point picks four pixels per thread (eight heliostats in flight, H = 9: a chunk with a tail;
    2^20 + 4: a ragged last block) unless npix % 4 != 0 (2^20 + 2) or a pointer is misaligned - the same bits on every path."""
    bitmaps, idx, want = large_case(npix, H, T)
    shape = (1024, 1024) if npix == 1 << 20 else (npix,)
    vec = 4 if npix % 4 == 0 else 1
    dev = t(bitmaps).view((H,) + shape)
    got = per_target_checked(dev, idx, T, want.reshape((T,) + shape), vec=vec)
    assert not bits(got[T - 1]).any() and (idx == -1).any() and (idx == T).any()
    if npix == 1 << 20:
        moved = offset_view(dev)                                            # the scalar kernel at a large size, on the same data
        per_target_checked(moved, idx, T, want.reshape((T,) + shape), vec=1)
    print(f"per-target sum ({npix},{H},{T}): VEC {vec}, bit-equal")


@pytest.mark.parametrize("layout", ["contiguous", "transposed", "fp64"])
def test_per_target_sum_backward_is_an_exact_gather(layout):
    from artist_amd import per_target_sum
    npix, H, T = 257, 65, 3
    bitmaps, idx = ref.per_target_inputs(npix, H, T)
    leaf = {"contiguous": lambda: t(bitmaps), "transposed": lambda: t(bitmaps.T.copy()), "fp64": lambda: t(bitmaps).double()}[layout]()
    leaf.requires_grad_(True)
    out = per_target_sum(leaf.t() if layout == "transposed" else leaf, t(idx), T)
    assert same_bits(n(out), ref.per_target_sum32(bitmaps, idx, T))
    g_out = ref.spread(np.random.default_rng(23), (T, npix), -3, 3)
    out.backward(t(g_out))
    grad = n(leaf.grad.t() if layout == "transposed" else leaf.grad)
    assert leaf.grad.shape == leaf.shape and leaf.grad.dtype == leaf.dtype
    ok = (idx >= 0) & (idx < T)
    want = np.where(ok[:, None], g_out[np.clip(idx, 0, T - 1)], np.float32(0))
    assert (~ok).sum() == 2 and np.array_equal(grad.astype(np.float64), want.astype(np.float64)) and not grad[~ok].any()


# ----------------------------------------------------------------------------------------------------------------- Adam
def adam_run(p, g, m, v, before, kw, shape=None, misaligned="", lock=False):
    """One ``optim.Adam`` step from the prepared state (``step = before``): new (p, m, v) as numpy and the plan of the call.
    ``misaligned``: which of p, g, m (both moments) are contiguous views one float past a 16-byte boundary."""
    from artist_amd.optim import Adam
    shape = shape or p.shape
    place = lambda a, key: (offset_view(a.reshape(shape)) if key in misaligned else t(a.reshape(shape)).clone())     # noqa: E731
    param = place(p, "p").detach().requires_grad_(True)
    param.grad = place(g, "g")
    opt = Adam([param], lock_outer_edges=lock, **kw)
    state = dict(step=before, exp_avg=place(m, "m"), exp_avg_sq=place(v, "m"))
    opt.state[param] = state
    plan = ref.plan_adam(param.numel(), param.data_ptr(), param.grad.data_ptr(), state["exp_avg"].data_ptr(), state["exp_avg_sq"].data_ptr())
    opt.step()
    assert opt.state[param]["step"] == before + 1
    return (n(param).reshape(-1), n(state["exp_avg"]).reshape(-1), n(state["exp_avg_sq"]).reshape(-1)), plan


def scalars_of(kw, step):
    return ref.adam_scalars(step=step, **kw)


@pytest.mark.parametrize("before", ref.ADAM_STEPS_BEFORE)
@pytest.mark.parametrize("name", list(ref.ADAM_SETTINGS))
def test_adam_step_is_within_the_derived_bounds(name, before):
    kw = ref.ADAM_SETTINGS[name]
    ratios = np.zeros(4)
    for size in ref.ADAM_SIZES:
        p, g, m, v = ref.adam_inputs(size, seed=before)
        (p1, m1, v1), plan = adam_run(p, g, m, v, before, kw)
        assert plan == (size // 4, 1 if size % 4 else 0)
        s = scalars_of(kw, before + 1)
        want_p, want_m, want_v = ref.adam_step64(p, g, m, v, s)
        b_p, b_m, b_v, b_local = ref.adam_bounds(p, g, m, v, s)
        ratios = np.maximum(ratios, [worst(p1 - want_p, b_p), worst(m1 - want_m, b_m), worst(v1 - want_v, b_v),
                                     worst(p1 - ref.adam_p_from_moments64(p, m1, v1, s), b_local)])
        if size >= 5 and kw.get("weight_decay", 0.0) == 0.0:
            zero = (g == 0) & (m == 0) & (v == 0)
            assert zero.any() and same_bits(p1[zero], p[zero]) and not bits(m1[zero]).any() and not bits(v1[zero]).any()
    print(f"adam {name}, step {before + 1}: error / bound  p {ratios[0]:.3f}  m {ratios[1]:.3f}  v {ratios[2]:.3f}  p from its own moments {ratios[3]:.3f}")
    assert ratios.max() <= 1.0


@pytest.mark.parametrize("name", ["default", "maximize_weight_decay"])
@pytest.mark.parametrize("misaligned", ["p", "g", "m", "pgm"])
def test_adam_element_wise_path_gives_the_bits_of_the_vector_path(misaligned, name):
    """The same data with the parameter (a leaf view at a storage offset of one float), only the gradient, or only the moments
    (views handed in through the state) misaligned: the kernel goes element by element - and ends on the same bits, the
    ``n % 4`` tail included."""
    kw = ref.ADAM_SETTINGS[name]
    for size in ref.ADAM_SIZES:
        p, g, m, v = ref.adam_inputs(size, seed=7)
        base, plan = adam_run(p, g, m, v, 1, kw)
        moved, plan_moved = adam_run(p, g, m, v, 1, kw, misaligned=misaligned)
        assert plan == (size // 4, 1 if size % 4 else 0) and plan_moved == (0, (size + 3) // 4)
        for a, b in zip(moved, base):
            assert same_bits(a, b), (size, misaligned)


def zero_edge_uv(g, shape):
    locked = g.reshape(shape).copy()
    for edge in (locked[:, 0], locked[:, -1], locked[:, :, 0], locked[:, :, -1]):
        edge[..., :2] = 0                                                   # u and v of the edge control points; z stays free
    return locked.reshape(-1)


@pytest.mark.parametrize("weight_decay", [0.0, 0.1])
@pytest.mark.parametrize("misaligned", ["", "pgm"], ids=["vector", "element-wise"])
@pytest.mark.parametrize("nets,nu,nv", ref.ADAM_LOCK_SHAPES)
def test_adam_edge_lock_on_both_paths(nets, nu, nv, misaligned, weight_decay):
    """The lock against this Adam WITHOUT it, stepping on the gradient whose edge u, v are zeroed (the recipe of
    tests/test_gpu_optim.py): the same bits, from a prepared state and from a fresh one.  From a fresh state the locked components
    move by the weight-decay term and nothing else - not at all without weight decay -, z of the edge points and every
    interior point move."""
    shape = (nets, nu, nv, 3)
    size = int(np.prod(shape))
    kw = dict(lr=1e-2, weight_decay=weight_decay)
    p, g, m, v = ref.adam_inputs(size, seed=9, zeros=False)
    locked = ref.adam_locked(size, nu, nv)
    assert np.array_equal(zero_edge_uv(g, shape) == 0, locked)
    for fresh in (False, True):
        m0, v0, before = (np.zeros_like(m), np.zeros_like(v), 0) if fresh else (m, v, 3)
        got, plan = adam_run(p, g, m0, v0, before, kw, shape=shape, misaligned=misaligned, lock=True)
        want, _ = adam_run(p, zero_edge_uv(g, shape), m0, v0, before, kw, shape=shape)
        assert plan == ((0, (size + 3) // 4) if misaligned else (size // 4, 1 if size % 4 else 0))
        for a, b in zip(got, want):
            assert same_bits(a, b), (fresh, int((bits(a) != bits(b)).sum()))
        if fresh:
            s = scalars_of(kw, 1)
            if weight_decay == 0.0:
                assert same_bits(got[0][locked], p[locked]) and not bits(got[1][locked]).any() and not bits(got[2][locked]).any()
            else:
                alone = ref.adam_step64(p, np.zeros_like(g), m0, v0, s)           # the weight-decay term alone
                bounds = ref.adam_bounds(p, np.zeros_like(g), m0, v0, s)
                assert max(worst((a - b)[locked], c[locked]) for a, b, c in zip(got, alone, bounds)) <= 1.0
            assert (got[0][~locked] != p[~locked]).all() and (~locked).sum() >= size // 3         # z everywhere, and the interior
        ratios = [worst(a - b, c) for a, b, c in zip(got, ref.adam_step64(p, g, m0, v0, scalars_of(kw, before + 1), locked),
                                                     ref.adam_bounds(p, g, m0, v0, scalars_of(kw, before + 1), locked))]
        assert max(ratios) <= 1.0
