"""The project's own restatement (numpy, fp64 by default) of the facet canting: the basis of
artist/geometry/transforms.py:320-340, the rotation with or without the facet translation (transforms.py:341-347,
artist/nurbs/surfaces.py:674-687), and the gradients autograd derives for them, written out by hand.

TEST INFRASTRUCTURE - not part of the product.  Checked against the reference's fp64 outputs on the host
(tests/test_canting_host.py); the yardstick of the GPU tests where no fixture reaches (tests/test_gpu_canting.py).

Shapes: canting [..., 2, 4], data [..., M, 4], translations [..., 4], with the same leading dimensions."""
import numpy as np

EPS_E, EPS_U, EPS_N = 1e-12, 1e-8, 1e-8

CASES = ["a", "b", "c", "d", "e"]                 # tests/golden/canting.npz (generate_canting_golden.py)


def fixture_case(d, name):
    """Case ``name`` of tests/golden/canting.npz as a dict without the prefix."""
    return {k[len(name) + 1:]: v for k, v in d.items() if k.startswith(name + "_")}


def activate(x, mask):
    """Rows of ``x`` repeated as ``HeliostatGroup.activate_heliostats`` repeats them."""
    return np.repeat(np.asarray(x), np.asarray(mask), axis=0)


def to_base(g_active, mask):
    """The adjoint of :func:`activate`: the gradients of a heliostat's replicas added up in its row."""
    owner = np.repeat(np.arange(len(mask)), np.asarray(mask))
    out = np.zeros((len(mask),) + g_active.shape[1:], dtype=g_active.dtype)
    np.add.at(out, owner, g_active)
    return out


def _norm(v):
    return np.sqrt((v * v).sum(-1, keepdims=True))


def _unit(v, eps):
    return v / np.maximum(_norm(v), v.dtype.type(eps))


def _unit_adjoint(v, eps, g):
    """g_v for out = v / max(|v|, eps): a clamped norm is a constant (clamp_min passes no gradient below its bound)."""
    n = _norm(v)
    live = n >= eps
    safe = np.where(live, n, v.dtype.type(1.0))
    o = v / safe
    return np.where(live, (g - o * (o * g).sum(-1, keepdims=True)) / safe, g / v.dtype.type(eps))


def basis(canting, dtype=np.float64):
    """B [..., 3, 3]: rows e^, n_ortho, u (the columns of the reference's rotation matrix)."""
    c = np.asarray(canting, dtype=dtype)
    e = _unit(c[..., 0, :3], EPS_E)
    u = _unit(np.cross(e, c[..., 1, :3]), EPS_U)
    o = _unit(np.cross(u, e), EPS_N)
    return np.stack([e, o, u], axis=-2)


def rotate(canting, data, inverse=False, translations=None, dtype=np.float64):
    """perform_canting (+ the translation): data @ R^T, or data @ R for the inverse; w passes through."""
    B = basis(canting, dtype)
    d = np.asarray(data, dtype=dtype)
    out = d.copy()
    out[..., :3] = np.einsum("...mk,...kj->...mj" if not inverse else "...mj,...kj->...mk", d[..., :3], B)
    if translations is not None:
        out = out + np.asarray(translations, dtype=dtype)[..., None, :]
    return out


def gradients(canting, pairs, inverse=False, with_translations=False, dtype=np.float64):
    """``pairs`` = [(data, grad_out, translated)] - the arrays canted with one ``canting`` (points and normals, say) and the
    gradients w.r.t. their canted versions.  Returns (grad_canting [..., 2, 4], grad_translations [..., 4] or None,
    [grad_data per pair])."""
    c = np.asarray(canting, dtype=dtype)
    e0, n = c[..., 0, :3], c[..., 1, :3]
    e = _unit(e0, EPS_E)
    u0 = np.cross(e, n)
    u = _unit(u0, EPS_U)
    o0 = np.cross(u, e)
    B = np.stack([e, _unit(o0, EPS_N), u], axis=-2)
    gB = np.zeros_like(B)
    g_tr = np.zeros(c.shape[:-2] + (4,), dtype=dtype) if with_translations else None
    g_data = []
    for data, g_out, translated in pairs:
        d, g = np.asarray(data, dtype=dtype), np.asarray(g_out, dtype=dtype)
        gd = g.copy()
        if inverse:      # out_k = sum_j d_j B[k][j]
            gd[..., :3] = np.einsum("...mk,...kj->...mj", g[..., :3], B)
            gB += np.einsum("...mk,...mj->...kj", g[..., :3], d[..., :3])
        else:            # out_j = sum_k d_k B[k][j]
            gd[..., :3] = np.einsum("...mj,...kj->...mk", g[..., :3], B)
            gB += np.einsum("...mk,...mj->...kj", d[..., :3], g[..., :3])
        g_data.append(gd)
        if translated and with_translations:
            g_tr += g.sum(-2)
    # the adjoint of the basis (c = a x b: g_a = b x g_c, g_b = g_c x a)
    g_o0 = _unit_adjoint(o0, EPS_N, gB[..., 1, :])
    g_u = gB[..., 2, :] + np.cross(e, g_o0)
    g_e = gB[..., 0, :] + np.cross(g_o0, u)
    g_u0 = _unit_adjoint(u0, EPS_U, g_u)
    g_e = g_e + np.cross(n, g_u0)
    g_n = np.cross(g_u0, e)
    g_e0 = _unit_adjoint(e0, EPS_E, g_e)
    g_c = np.zeros_like(c)
    g_c[..., 0, :3], g_c[..., 1, :3] = g_e0, g_n
    return g_c, g_tr, g_data
