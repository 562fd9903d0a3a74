"""Plain-numpy references of the four small entry points that every epoch of every optimiser runs - ``art_align_fwd`` /
``art_align_bwd``, ``art_reflect``, ``art_per_target_sum``, ``art_adam_step`` - with the inputs and the case lists that
tests/test_epoch_ops_host.py (no device) and tests/test_gpu_epoch_ops.py (the kernels) share.

Rule of the comparisons.  The library is compiled with ``-ffp-contract=off`` and three of these kernels use nothing but IEEE fp32
``+`` and ``*``: where the ORDER of those operations is the contract (align forward / backward apply, reflect, per-target sum)
there is an fp32 restatement here, op for op with every step rounded to ``np.float32``, and the kernel must give its bits.
Where the order is the kernel's own business (the orientation gradient's summation tree) or the kernel uses ``sqrtf`` and ``/``
(Adam), the kernel is held to a rounding bound DERIVED below from the operations it performs, against an fp64 evaluation of the
same formula from the same fp32 inputs.  No bound here was measured; ``u = 2^-24`` is the unit roundoff of fp32 throughout.

Two facts are used repeatedly (Jeannerod & Rump, "Improved error bounds for inner products in floating-point arithmetic", SIAM J.
Matrix Anal. Appl. 34, 2013): a sum of n floating-point numbers evaluated in ANY order has an error of at most ``(n-1) u sum|x_i|``
and an n-term dot product one of at most ``n u sum|x_i y_i|`` - without second-order terms, barring underflow (the inputs below
hold no denormals and produce none).

The kernels cannot be asked which path they ran; ``plan_per_target_sum`` and ``plan_adam`` RESTATE the condition of the entry
point / kernel (they are not observations), so that the tests can say which path a case is meant to take; both paths of either
operation must give the same bits, which is what the tests check.
"""
import math

import numpy as np

F32 = np.float32
U = 2.0 ** -24


def _rng(*seed):
    return np.random.default_rng(list(seed))


def spread(rng, shape, lo, hi):
    """Normal variates times 10^uniform(lo, hi): magnitudes over several decades (a wrong order or a wrong index changes bits),
    never zero, never denormal (|x| >= 1e-6 * 10^lo)."""
    x = rng.standard_normal(shape)
    x = np.where(np.abs(x) < 1e-6, 1e-6, x)
    return (x * 10.0 ** rng.uniform(lo, hi, shape)).astype(F32)


# ---------------------------------------------------------------------------------------------------------------- align
#: (H, P): one point, below / at / above a wave, around the 256-thread tile of the apply kernels, around the 1024-thread block
#: of the orientation gradient (one, two, three and four strided iterations), several heliostats with several tiles each.
ALIGN_SHAPES = ((1, 1), (1, 63), (2, 64), (3, 65), (2, 255), (1, 256), (3, 257), (2, 1023), (1, 1024), (2, 1025), (3, 2049),
                (1, 3073))
ALIGN_SENTINEL_SHAPE = (3, 2049)
ALIGN_SENTINEL_POINTS = (0, 63, 64, 1023, 1024, 2048)
GM_BLOCK = 1024


def align_inputs(H, P, seed=0):
    """points, normals [H,P,4], orientation [H,4,4], upstream gradients [H,P,4] x 2 (fp32): a different full matrix per
    heliostat with all sixteen entries non-zero, points of order 100 with a random w, random-w normals."""
    rng = _rng(11, H, P, seed)
    M = spread(rng, (H, 4, 4), -2, 1)
    points = (rng.standard_normal((H, P, 4)) * 100.0).astype(F32)
    points[..., 3] = spread(rng, (H, P), -1, 1)
    points = np.where(points == 0, F32(1.0), points)
    normals = spread(rng, (H, P, 4), -2, 0)
    g_points, g_normals = spread(rng, (H, P, 4), -3, 2), spread(rng, (H, P, 4), -3, 2)
    return points, normals, M, g_points, g_normals


def align_fwd32(x, M):
    """out[h,p,j] = ((x0 M[j][0] + x1 M[j][1]) + x2 M[j][2]) + x3 M[j][3], every step rounded to fp32 (``apply_mt``)."""
    x, M = np.asarray(x, F32), np.asarray(M, F32)
    m = M[:, None, :, :]                                                     # [H,1,j,k]
    x0, x1, x2, x3 = (x[..., k, None] for k in range(4))                    # [H,P,1]
    return ((x0 * m[..., 0] + x1 * m[..., 1]) + x2 * m[..., 2]) + x3 * m[..., 3]


def align_bwd32(g, M):
    """grad_x[h,p,k] = ((g0 M[0][k] + g1 M[1][k]) + g2 M[2][k]) + g3 M[3][k] (``apply_m``): the forward with M transposed."""
    return align_fwd32(g, np.swapaxes(np.asarray(M, F32), 1, 2))


def align_fwd64(x, M):
    """(x @ M^T in fp64 from the fp32 inputs, bound [H,P,4]): ``4 u sum_k |x_k M_jk|`` - the 4-term dot-product bound, which
    holds for any summation order."""
    x, M = np.asarray(x, np.float64), np.asarray(M, np.float64)
    return np.einsum("hpk,hjk->hpj", x, M), 4.0 * U * np.einsum("hpk,hjk->hpj", np.abs(x), np.abs(M))


def align_bwd64(g, M):
    return align_fwd64(g, np.swapaxes(np.asarray(M), 1, 2))


def align_gm_depth(P):
    """Roundings on the longest path from a product to the stored sum in ``align_gm_kernel``: per thread and iteration two
    products with one add (2: each product passes its own rounding and the add) and one accumulate (1) - 3 per iteration,
    ``ceil(P / 1024)`` iterations -, then the six levels of the wave's shuffle tree, then the sixteen wave sums added in
    order.  If a later change reshapes the tree this formula follows the tree: count the roundings between a product and the
    stored value on the longest path, per iteration x iterations + levels of each tree + length of each in-order chain."""
    return 3 * max(1, math.ceil(P / GM_BLOCK)) + 6 + 16


def align_gm64(points, normals, g_points, g_normals):
    """(G, bound): G[h,j,k] = sum_p (gP_j xP_k + gN_j xN_k) in fp64 from the fp32 inputs and ``depth u S_jk 1.01`` with
    S_jk = sum_p (|gP_j xP_k| + |gN_j xN_k|): every term passes at most ``depth`` roundings, each relative to a partial sum whose
    magnitude is at most S; 1.01 covers the second-order terms ((1+u)^depth - 1 <= depth u 1.01 for depth u < 0.01).  A bound on
    the kernel's summation tree, not a measurement.  A dropped term stays far outside it: at P = 2049 one of 4098 terms averages
    S / 4098 = 4096 u S against 31 u S."""
    xp, xn, gp, gn = (np.asarray(a, np.float64) for a in (points, normals, g_points, g_normals))
    G = np.einsum("hpj,hpk->hjk", gp, xp) + np.einsum("hpj,hpk->hjk", gn, xn)
    S = np.einsum("hpj,hpk->hjk", np.abs(gp), np.abs(xp)) + np.einsum("hpj,hpk->hjk", np.abs(gn), np.abs(xn))
    return G, align_gm_depth(xp.shape[1]) * U * S * 1.01


def align_gm_tree32(points, normals, g_points, g_normals):
    """The kernel's order simulated in fp32: 1024 threads stride over the points (``gm += g_j x_k + h_j y_k``), each wave of 64
    adds its lanes in the shuffle tree (offsets 32, 16, ... 1: lane i takes lane i + off), thread k < 16 adds the sixteen wave
    sums in index order starting from +0.  Used by the host test to show that the bound above is honest for this tree; the
    kernel is held to the bound, not to these bits."""
    xp, xn, gp, gn = (np.asarray(a, F32) for a in (points, normals, g_points, g_normals))
    H, P = xp.shape[:2]
    n_it = max(1, math.ceil(P / GM_BLOCK))
    pad = lambda a: np.concatenate([a, np.zeros((H, n_it * GM_BLOCK - P, 4), F32)], axis=1)      # noqa: E731  (x + 0 = x)
    xp, xn, gp, gn = pad(xp), pad(xn), pad(gp), pad(gn)
    acc = np.zeros((H, GM_BLOCK, 4, 4), F32)
    for it in range(n_it):
        s = slice(it * GM_BLOCK, (it + 1) * GM_BLOCK)
        acc = acc + (gp[:, s, :, None] * xp[:, s, None, :] + gn[:, s, :, None] * xn[:, s, None, :])
    w = acc.reshape(H, GM_BLOCK // 64, 64, 4, 4)
    off = 32
    while off > 0:
        w = w[:, :, :off] + w[:, :, off:2 * off]
        off >>= 1
    out = np.zeros((H, 4, 4), F32)
    for k in range(GM_BLOCK // 64):
        out = out + w[:, k, 0]
    return out


def align_gm_single32(points, normals, g_points, g_normals, h, p):
    """The orientation gradient of heliostat ``h`` when the upstream gradient is non-zero at point ``p`` only: the single rounded
    products ``fl(fl(gP_j xP_k) + fl(gN_j xN_k))`` - every other term is an exact zero, so no order can change it."""
    xp, xn, gp, gn = (np.asarray(a, F32)[h, p] for a in (points, normals, g_points, g_normals))
    return gp[:, None] * xp[None, :] + gn[:, None] * xn[None, :]


# -------------------------------------------------------------------------------------------------------------- reflect
REFLECT_SHAPES = ((1, 1), (3, 85), (1, 256), (7, 37), (2, 1025))
REFLECT_EMPTY_SHAPES = ((0, 3), (3, 0))


def reflect_inputs(H, P, seed=0):
    """incident [H,4] (a different row per heliostat), normals [H,P,4]: four non-zero components in both."""
    rng = _rng(13, H, P, seed)
    return spread(rng, (H, 4), -1, 1), spread(rng, (H, P, 4), -2, 1)


def reflect32(incident, normals):
    """s = ((i0 n0 + i1 n1) + i2 n2) + i3 n3, s2 = 2 s, out_c = i_c - s2 n_c, every step rounded to fp32."""
    i, n = np.asarray(incident, F32)[:, None, :], np.asarray(normals, F32)
    s = ((i[..., 0] * n[..., 0] + i[..., 1] * n[..., 1]) + i[..., 2] * n[..., 2]) + i[..., 3] * n[..., 3]
    s2 = F32(2.0) * s
    return i - s2[..., None] * n


def reflect64(incident, normals):
    """(out in fp64, bound).  Derivation: the computed dot product is s^ = s + e with |e| <= 4 u A, A = sum_k |i_k n_k| (4-term dot
    product); doubling is exact; t = fl(2 s^ n_c) = 2 s^ n_c (1 + d1); out^ = (i_c - t)(1 + d2), |d| <= u.  So
    out^ - out = -2 e n_c - 2 s^ n_c d1 + (i_c - t) d2, and with |2 s^| <= 2 A (1 + 4u), |t| <= 2 A |n_c| (1 + 4u)(1 + u):
    |out^ - out| <= u (8 A |n_c| + 2 A |n_c| + |i_c| + 2 A |n_c|) (1 + O(u)) = u (|i_c| + 12 A |n_c|) (1 + O(u)); the factor
    1.01 covers the O(u) terms."""
    i, n = np.asarray(incident, np.float64)[:, None, :], np.asarray(normals, np.float64)
    s = (i * n).sum(-1, keepdims=True)
    A = (np.abs(i) * np.abs(n)).sum(-1, keepdims=True)
    return i - 2.0 * s * n, U * (np.abs(i) + 12.0 * A * np.abs(n)) * 1.01


# ------------------------------------------------------------------------------------------------------- per-target sum
#: (npix, H, T) of the 64-loads-in-flight scalar kernel: one pixel, below / at / above a 256-thread block, several blocks with a
#: ragged last one; below / at / above one 64-heliostat chunk and two chunks with a tail; one target and three.
PER_TARGET_SMALL = ((1, 1, 1), (1, 65, 3), (255, 63, 3), (255, 1, 1), (256, 64, 1), (256, 130, 3), (257, 65, 1), (257, 63, 3),
                    (4097, 1, 3), (4097, 64, 3), (4097, 130, 1), (1, 130, 1), (256, 65, 3))
#: (npix, H, T) at and above 2^20 pixels, where the entry point picks the 4-pixel kernel for npix % 4 == 0 and aligned pointers:
#: one full 8-heliostat chunk and one with a tail (H = 9); 2^20 + 4 leaves the last block ragged; 2^20 + 2 takes the scalar kernel.
PER_TARGET_LARGE = ((1 << 20, 8, 2), (1 << 20, 9, 2), ((1 << 20) + 4, 8, 2), ((1 << 20) + 4, 9, 2), ((1 << 20) + 2, 9, 2))
VEC4_MIN_NPIX = 1 << 20


def per_target_inputs(npix, H, T, seed=0):
    """bitmaps [H,npix] fp32 and target indices [H] (int64) in [-1, T]: the indices -1 and T are among the heliostats when there
    is room for them (they contribute nothing), and target ``T - 1`` is never aimed at when T > 1 (its row must be exactly
    zero).  With T == 1 the only target is aimed at by every in-range heliostat; ``per_target_unaimed`` gives the indices of
    the second call of such a case, in which nobody aims at it."""
    rng = _rng(17, npix % 65521, H, T, seed)
    bitmaps = spread(rng, (H, npix), -3, 3)
    idx = rng.integers(0, max(T - 1, 1), H)
    if H >= 3:
        idx[rng.integers(0, H)] = -1
        idx[(int(np.argmax(idx == -1)) + 1) % H] = T
    return bitmaps, idx.astype(np.int64)


def per_target_unaimed(H, T):
    """Indices [H] that are all outside [0, T): -1 and T in turn."""
    return np.where(np.arange(H) % 2 == 0, -1, T).astype(np.int64)


def per_target_sum32(bitmaps, idx, T):
    """out[t] starts at +0.0f and takes ``bitmaps[h]`` for h = 0..H-1 with idx[h] == t, in index order, each sum rounded to fp32;
    indices outside [0, T) contribute nothing.  (The kernels also add +0.0f for foreign heliostats and past the end of the
    last chunk: x + 0 = x, and an accumulator that starts at +0 never becomes -0.)"""
    bitmaps = np.asarray(bitmaps, F32)
    out = np.zeros((T,) + bitmaps.shape[1:], F32)
    for h, t in enumerate(np.asarray(idx).tolist()):
        if 0 <= t < T:
            out[t] = out[t] + bitmaps[h]
    return out


def per_target_sum64(bitmaps, idx, T):
    bitmaps = np.asarray(bitmaps, np.float64)
    out = np.zeros((T,) + bitmaps.shape[1:], np.float64)
    for h, t in enumerate(np.asarray(idx).tolist()):
        if 0 <= t < T:
            out[t] += bitmaps[h]
    return out


def plan_per_target_sum(npix, bitmaps_ptr, out_ptr):
    """VEC of the kernel that ``art_per_target_sum`` launches - 4 or 1 - restated from the entry point's condition: 4-pixel
    threads for ``npix >= 2^20`` with ``npix % 4 == 0`` and both pointers 16-byte aligned, else one pixel per thread."""
    return 4 if npix >= VEC4_MIN_NPIX and npix % 4 == 0 and bitmaps_ptr % 16 == 0 and out_ptr % 16 == 0 else 1


# ----------------------------------------------------------------------------------------------------------------- Adam
ADAM_SIZES = (1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025, 1027)
ADAM_STEPS_BEFORE = (0, 1, 999)
ADAM_SETTINGS = {
    "default": dict(lr=1e-3),
    "weight_decay": dict(lr=1e-2, weight_decay=0.1),
    "maximize": dict(lr=1e-2, maximize=True),
    "maximize_weight_decay": dict(lr=5e-3, weight_decay=0.05, maximize=True, betas=(0.8, 0.9), eps=1e-6),
    "betas_zero": dict(lr=1e-3, betas=(0.0, 0.0)),
}
#: (nets, nu, nv) of the edge lock: one net and several (27 elements per net straddle the 4-element groups), a single row, a
#: single column, nets that are all edge, nets with an interior, a net count that is no multiple of 4.
ADAM_LOCK_SHAPES = ((1, 3, 3), (5, 3, 3), (2, 1, 4), (3, 4, 1), (2, 2, 2), (3, 5, 4), (7, 4, 6))


def adam_inputs(n, seed=0, zeros=True):
    """p, g, m, v (fp32, [n]): a random exp_avg, a non-negative exp_avg_sq spread over many decades, and - from five elements on,
    unless ``zeros`` is off - every fifth element with g = m = v = 0."""
    rng = _rng(19, n, seed)
    p, g, m = spread(rng, n, -1, 1), spread(rng, n, -6, 2), spread(rng, n, -6, 2)
    v = np.abs(spread(rng, n, -12, 2))
    if n >= 5 and zeros:
        g[4::5] = 0; m[4::5] = 0; v[4::5] = 0
    return p, g, m, v


def adam_scalars(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, maximize=False, step=1, rounded=True):
    """The scalars of one step as ``art_adam_step`` forms them: the bias corrections in double from the step number, then
    ``(float)beta1``, ``(float)beta2``, ``(float)(1 - beta1)``, ``(float)(1 - beta2)``, ``(float)eps``, ``(float)(lr / bc1)``,
    ``(float)(1 / sqrt(bc2))``, ``(float)weight_decay`` - as doubles holding the fp32 values (``rounded=False``: the doubles
    themselves, which is what torch.optim.Adam computes with in fp64)."""
    beta1, beta2 = float(betas[0]), float(betas[1])
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    s = dict(beta2=beta2, one_minus_beta1=1.0 - beta1, one_minus_beta2=1.0 - beta2, eps=float(eps), step_size=lr / bc1,
             inv_bc2_sqrt=1.0 / math.sqrt(bc2), weight_decay=float(weight_decay))
    if rounded:
        s = {k: float(F32(x)) for k, x in s.items()}
    s["grad_sign"] = -1.0 if maximize else 1.0
    return s


def adam_locked(n, nu, nv):
    """[n] bool: is element i a u or v component (0, 1) of a control point in the first / last row or column of its [nu,nv,3]
    net?  (``lock_nu, lock_nv`` of the entry point; nu == 0: nothing is locked.)"""
    if nu <= 0:
        return np.zeros(n, bool)
    i = np.arange(n)
    cell, comp = i // 3, i % 3
    line, col = cell // nv, cell % nv
    row = line % nu
    return (comp < 2) & ((row == 0) | (row == nu - 1) | (col == 0) | (col == nv - 1))


def _adam(p, g, m, v, s, locked, dtype):
    c = lambda x: dtype(x)                                                   # noqa: E731
    p, g, m, v = (np.asarray(a, dtype) for a in (p, g, m, v))
    gr = np.where(locked, dtype(0.0), c(s["grad_sign"]) * g)
    if s["weight_decay"] != 0.0:
        gr = gr + c(s["weight_decay"]) * p
    m1 = m + (gr - m) * c(s["one_minus_beta1"])
    v1 = v * c(s["beta2"]) + (c(s["one_minus_beta2"]) * gr) * gr
    denom = np.sqrt(v1) * c(s["inv_bc2_sqrt"]) + c(s["eps"])
    return p - c(s["step_size"]) * (m1 / denom), m1, v1, gr, denom


def adam_step64(p, g, m, v, scalars, locked=False):
    """``adam_element`` in fp64 from the fp32 state: (p', m', v')."""
    return _adam(p, g, m, v, scalars, locked, np.float64)[:3]


def adam_step32(p, g, m, v, scalars, locked=False):
    """``adam_element`` op for op in fp32 (numpy's fp32 sqrt and division are correctly rounded).  For the host test of the
    bounds; the kernel is held to the bounds, not to these bits."""
    return _adam(p, g, m, v, scalars, locked, F32)[:3]


ADAM_MARGIN = 2.0


def adam_bounds(p, g, m, v, scalars, locked=False):
    """(bound_p, bound_m, bound_v) of an fp32 evaluation of ``adam_element`` against ``adam_step64``, and ``bound_p_local`` (below).
    Every d is a rounding, |d| <= u; first order in u, and the margin factor of 2 covers the second-order terms.

    gr: ``sign g`` is exact.  With weight decay gr^ = (sign g + wd p (1 + d1))(1 + d2): |gr^ - gr| <= E_gr = 2 u (|g| + |wd p|);
        E_gr = 0 without it.
    m': m^ = (m + (gr^ - m)(1 + d1) c (1 + d2))(1 + d3), c = 1 - beta1: three roundings, the first two on |gr - m| c and the third
        on |m'| <= |m| + |gr - m| c, plus what gr brought:  E_m = 3 u (|m| + |gr - m| c) + c E_gr.
    v': v^ = (v b2 (1 + d1) + c2 gr^ (1 + d2) gr^ (1 + d3))(1 + d4), c2 = 1 - beta2: both terms are non-negative, no term passes
        more than three of the four roundings, plus what gr brought:  E_v = 4 u (v b2 + c2 gr^2) + 2 c2 |gr| E_gr.
    p': denom^ = (sqrt(v^)(1 + d1) r (1 + d2) + eps)(1 + d3) is a sum of non-negatives, so nothing cancels: its relative error is
        at most 3 u + E_v / (2 v') (the square root halves the relative error of v^; 0 where v' = 0).  w^ = ss (m^ / denom^)(1 + d4)
        (1 + d5) and p^ = (p - w^)(1 + d6):
        E_p = u |p'| + |w| (5 u + E_v / (2 v')) + ss E_m / denom,   w = ss m' / denom.
        The first two terms with E_v = 0 are the roundings of the last two lines alone - ``bound_p_local``: what an fp32
        evaluation may differ by from the fp64 evaluation of those two lines on ITS OWN m^ and v^ (u |p'|, plus the five
        relative roundings of sqrt, *, +, /, * applied to ss |m'/denom|)."""
    s = scalars
    p1, m1, v1, gr, denom = _adam(p, g, m, v, s, locked, np.float64)
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    c, c2 = s["one_minus_beta1"], s["one_minus_beta2"]
    e_gr = 2.0 * U * (np.abs(gr - s["weight_decay"] * p) + np.abs(s["weight_decay"] * p)) if s["weight_decay"] != 0.0 else 0.0 * p
    e_m = 3.0 * U * (np.abs(m) + np.abs(gr - m) * c) + c * e_gr
    e_v = 4.0 * U * (v * s["beta2"] + c2 * gr * gr) + 2.0 * c2 * np.abs(gr) * e_gr
    w = np.abs(s["step_size"] * (m1 / denom))
    rel_v = np.divide(e_v, 2.0 * v1, out=np.zeros_like(v1), where=v1 > 0)
    local = U * np.abs(p1) + w * 5.0 * U
    e_p = local + w * rel_v + s["step_size"] * e_m / denom
    return ADAM_MARGIN * e_p, ADAM_MARGIN * e_m, ADAM_MARGIN * e_v, ADAM_MARGIN * local


def adam_p_from_moments64(p, m1, v1, scalars):
    """The last two lines of ``adam_element`` in fp64 from given (fp32) new moments: what ``bound_p_local`` is a bound against."""
    p, m1, v1 = (np.asarray(a, np.float64) for a in (p, m1, v1))
    return p - scalars["step_size"] * (m1 / (np.sqrt(v1) * scalars["inv_bc2_sqrt"] + scalars["eps"]))


def plan_adam(n, *pointers):
    """How ``adam_step_kernel`` covers ``n`` elements - (threads on the 16-byte path, threads on the element-wise path) - restated
    from the kernel's condition: a thread owns elements [4k, 4k + 4) and takes the vector path when its group is whole and all
    four pointers (param, grad, exp_avg, exp_avg_sq) are 16-byte aligned."""
    threads = (n + 3) // 4
    if any(ptr % 16 for ptr in pointers):
        return 0, threads
    return n // 4, threads - n // 4
