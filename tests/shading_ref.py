"""NumPy restatement of heliostat shading (include/artist_hip_shading.h), evaluated in the dtype it is
given (float64: the yardstick; float32: the arithmetic of the kernels, operation order not guaranteed):

  * the cull rule of ``art_shading_cull`` (stated at the top of artist_amd/csrc/shading_kernels.hip) with, for every pair,
    its relative distance from the decision threshold;
  * the shear tables of ``art_shading_prims_fwd``, in NumPy and - for the adjoint - in torch;
  * the soft mask of ``soft_ray_blocking_mask`` (artist/raytracing/blocking.py:288-352) for arbitrary rays;
  * a DIRECT shading transmittance per surface point: the sunward ray against the real rectangles, no shear anywhere.
"""
import numpy as np

TILT = 0.02            # kShadeTilt
OFF_PLANE = 0.05       # kShadeOffPlane
MIN_COS = 1e-3         # kShadeMinCos
SOFTNESS, ALPHA, OFFSET, EPS = 1000.0, 100.0, 0.05, 1e-12      # blocking.py:217-220


def _dot(a, b):
    return (a * b).sum(-1)


def _normalize(v):
    length = np.maximum(np.sqrt(_dot(v, v)), v.dtype.type(1e-12))
    return v / length[..., None]


def rectangles(corners, dtype=np.float64):
    """corner 0, span_u, span_v, centre, unit normal, half of the longer diagonal of ``corners [N,4,>=3]``."""
    c = np.asarray(corners, dtype=dtype)[..., :3]
    c0, su, sv = c[:, 0], c[:, 1] - c[:, 0], c[:, 3] - c[:, 0]
    half = dtype(0.5)
    centre = c0 + half * (su + sv)
    dp, dm = su + sv, su - sv
    half_diag = half * np.sqrt(np.maximum(_dot(dp, dp), _dot(dm, dm)))
    return c0, su, sv, centre, _normalize(np.cross(su, sv)), half_diag


def spans_and_normals(corners):
    """The tables ``create_blocking_primitives_rectangles_by_index`` forms from ``corners [N,4,4]``."""
    corners = np.asarray(corners)
    spans = np.stack((corners[:, 1] - corners[:, 0], corners[:, 3] - corners[:, 0]), axis=1)
    normals = np.zeros((corners.shape[0], 4), corners.dtype)
    normals[:, :3] = _normalize(np.cross(spans[:, 0, :3], spans[:, 1, :3]))
    return spans, normals


def cull(corners, owner, incident, max_scatter, dtype=np.float64):
    """``(listed [H,N] bool, margin [H,N])``: the rule, and how far (relative) each pair is from flipping: the smallest
    relative slack of the inequalities that decide it (inf where none does: the owner itself, a grazing sun)."""
    dt = dtype
    _, _, _, centre, normal, half_diag = rectangles(corners, dt)
    owner = np.asarray(owner).astype(np.int64)
    H, N = owner.shape[0], centre.shape[0]
    listed, margin = np.zeros((H, N), bool), np.full((H, N), np.inf)
    for h in range(H):
        o = owner[h]
        s = -np.asarray(incident, dtype=dt)[h, :3]
        n = normal[o]
        sn = _dot(s, n)
        if abs(sn) < dt(MIN_COS):
            continue
        sp = s - sn * n
        T = np.sqrt(_dot(sp, sp)) / abs(sn)
        g = dt(1.0) + dt(2.0) * T
        kappa = g * (dt(1.4143) * dt(max_scatter) + dt(TILT))
        r_own = dt(1.02) * half_diag[o] + dt(OFF_PLANE) * g
        reach = r_own + (dt(1.06) * half_diag + dt(2e-3))
        w = centre - centre[o]
        a = _dot(w, s)
        perp = np.sqrt(np.maximum(_dot(w, w) - a * a, dt(0.0)))
        ok = np.ones(N, bool)
        m = np.full(N, np.inf)
        if kappa < dt(0.5):
            limit = reach + (a + reach) * (kappa / (dt(1.0) - kappa))
            ok &= (a >= -reach) & (perp <= limit)
            m = np.minimum(m, np.abs(a + reach) / reach)
            m = np.minimum(m, np.abs(limit - perp) / np.maximum(np.abs(limit), reach))
        if kappa < abs(sn):
            front = np.sign(sn) * _dot(w, n)
            ok &= front >= -reach
            m = np.minimum(m, np.abs(front + reach) / reach)
        ok[o], m[o] = False, np.inf
        listed[h], margin[h] = ok, m
    return listed, margin


def cull_lists(listed, slots):
    """``(shader_idx [H,S] int32, shade_count [H] int32)`` as ``art_shading_cull`` writes them."""
    H = listed.shape[0]
    idx = np.full((H, slots), -1, np.int32)
    count = np.zeros(H, np.int32)
    for h in range(H):
        found = np.nonzero(listed[h])[0]
        count[h] = len(found)
        idx[h, :min(slots, len(found))] = found[:slots]
    return idx, count


def own_planes(corners, owner, incident, dtype=np.float64):
    """centre ``c``, normal ``n``, sun vector ``s``, ``s.n`` and ``s_par`` per traced heliostat."""
    _, _, _, centre, normal, _ = rectangles(corners, dtype)
    owner = np.asarray(owner).astype(np.int64)
    s = -np.asarray(incident, dtype=dtype)[:, :3]
    c, n = centre[owner], normal[owner]
    sn = _dot(s, n)
    return c, n, s, sn, s - sn[:, None] * n


def shear(x, c, n, sn, sp):
    """``A_h(x) = x - 2 ((x - c).n)/(s.n) s_par`` for points ``x [...,3]`` of ONE heliostat."""
    a = _dot(x - c, n) / sn
    return x - (x.dtype.type(2.0) * a)[..., None] * sp


def shear_tables(corners, owner, incident, shader_idx, dtype=np.float64):
    """The three tables of ``art_shading_prims_fwd``: ``[H*S,4,4]``, ``[H*S,2,4]``, ``[H*S,4]``; zeros in empty slots."""
    dt = dtype
    corners = np.asarray(corners, dtype=dt)
    c, n, s, sn, sp = own_planes(corners, owner, incident, dt)
    H, S = shader_idx.shape
    vc, vs, vn = np.zeros((H * S, 4, 4), dt), np.zeros((H * S, 2, 4), dt), np.zeros((H * S, 4), dt)
    for h in range(H):
        for k in range(S):
            j = int(shader_idx[h, k])
            if j < 0 or abs(sn[h]) < dt(MIN_COS):
                continue
            i = h * S + k
            vc[i, :, :3] = shear(corners[j, :, :3], c[h], n[h], sn[h], sp[h])
            vc[i, :, 3] = corners[j, :, 3]
    filled = np.repeat((np.asarray(shader_idx).reshape(-1) >= 0)[:, None], 4, 1)
    spans, normals = spans_and_normals(vc)
    vs[:] = spans
    vn[:] = np.where(filled, normals, dt(0.0))
    return vc, vs, vn


def shear_tables_torch(corners, owner, incident, shader_idx):
    """``shear_tables`` in torch (any dtype, CPU), differentiable w.r.t. ``corners [N,4,4]``: the yardstick of the adjoint."""
    import torch
    owner, idx = torch.as_tensor(owner).long(), torch.as_tensor(shader_idx).long()
    H, S = idx.shape
    x = corners[..., :3]
    su, sv = x[:, 1] - x[:, 0], x[:, 3] - x[:, 0]
    centre = x[:, 0] + 0.5 * (su + sv)
    normal = torch.nn.functional.normalize(torch.linalg.cross(su, sv), dim=-1)
    s = -torch.as_tensor(incident, dtype=corners.dtype)[:, :3]
    c, n = centre[owner], normal[owner]
    sn = (s * n).sum(-1)
    sp = s - sn[:, None] * n
    filled = (idx >= 0)
    q = x[idx.clamp(min=0)]                                                        # [H,S,4,3]
    a = ((q - c[:, None, None]) * n[:, None, None]).sum(-1) / sn[:, None, None]
    y = q - 2.0 * a[..., None] * sp[:, None, None]
    y = y * filled[..., None, None]
    U, V = y[:, :, 1] - y[:, :, 0], y[:, :, 3] - y[:, :, 0]
    nv = torch.nn.functional.normalize(torch.linalg.cross(U, V), dim=-1) * filled[..., None]
    return y.reshape(H * S, 4, 3), torch.stack((U, V), dim=2).reshape(H * S, 2, 3), nv.reshape(H * S, 3)


def sigmoid(x):
    out = np.empty_like(x)
    pos = x >= 0
    out[pos] = 1.0 / (1.0 + np.exp(-x[pos]))
    e = np.exp(x[~pos])
    out[~pos] = e / (1.0 + e)
    return out.astype(x.dtype)


def soft_sigma(origins, dirs, corners, spans, normals):
    """sigma ``[M,K]`` of rays ``origins/dirs [M,3]`` against ``K`` parallelograms, and ``(t, u, v) [M,K]``
    (blocking.py:288-348: plane hit, Gram system with the span_u.span_v term, five sigmoids, clamp)."""
    dt = origins.dtype.type
    c0 = np.asarray(corners, origins.dtype)[None, :, 0, :3]
    su = np.asarray(spans, origins.dtype)[None, :, 0, :3]
    sv = np.asarray(spans, origins.dtype)[None, :, 1, :3]
    nn = np.asarray(normals, origins.dtype)[None, :, :3]
    o, d = origins[:, None, :], dirs[:, None, :]
    den = _dot(d, nn)
    den = np.where(np.abs(den) < dt(EPS), np.where(den >= 0, dt(EPS), dt(-EPS)), den)
    t = _dot(c0 - o, nn) / den
    off = (o + t[..., None] * d) - c0
    suu, svv, suv = _dot(su, su), _dot(sv, sv), _dot(su, sv)
    pu, pv = _dot(off, su), _dot(off, sv)
    det = suu * svv - suv * suv
    det = np.where(np.abs(det) < dt(EPS), np.sign(det) * dt(EPS), det)
    u = (pu * svv - pv * suv) / det
    v = (pv * suu - pu * suv) / det
    k = dt(SOFTNESS)
    sigma = (sigmoid(k * u) * sigmoid(k * (dt(1.0) - u))) * (sigmoid(k * v) * sigmoid(k * (dt(1.0) - v))) * sigmoid(k * (t - dt(OFFSET)))
    return np.clip(sigma, dt(0.0), dt(1.0)), (t, u, v)


def transmittance(origins, dirs, corners, spans, normals):
    """``exp(-alpha sum sigma) [M]`` (blocking.py:350-351); 1 where there is no parallelogram."""
    if len(corners) == 0:
        return np.ones(origins.shape[0], origins.dtype)
    sigma, _ = soft_sigma(origins, dirs, corners, spans, normals)
    return np.exp(-origins.dtype.type(ALPHA) * sigma.sum(-1)).astype(origins.dtype)


def direct_transmittance(points, owner, incident, corners, dtype=np.float64):
    """Shading from first principles, ``[H,P]``: the ray from every surface point TOWARDS THE SUN against the real rectangles
    of all other heliostats."""
    dt = dtype
    corners = np.asarray(corners, dtype=dt)
    spans, normals = spans_and_normals(corners)
    points = np.asarray(points, dtype=dt)[..., :3]
    owner = np.asarray(owner).astype(np.int64)
    out = np.ones(points.shape[:2], dt)
    for h in range(points.shape[0]):
        others = np.array([j for j in range(corners.shape[0]) if j != owner[h]], np.int64)
        s = -np.asarray(incident, dtype=dt)[h, :3]
        out[h] = transmittance(points[h], np.broadcast_to(s, points[h].shape).copy(), corners[others], spans[others], normals[others])
    return out


def reflect(incident3, normals3):
    """``i - 2 (i.n) n``."""
    return incident3 - incident3.dtype.type(2.0) * _dot(incident3, normals3)[..., None] * normals3


def shear_transmittance(points, point_normals, owner, incident, corners, shader_idx, dtype=np.float64):
    """The method of the kernels, ``[H,P]``: the REFLECTED ray of every surface point (its own normal) against the sheared
    tables of its heliostat."""
    dt = dtype
    vc, vs, vn = shear_tables(corners, owner, incident, shader_idx, dt)
    points = np.asarray(points, dtype=dt)[..., :3]
    point_normals = np.asarray(point_normals, dtype=dt)[..., :3]
    H, S = shader_idx.shape
    out = np.ones(points.shape[:2], dt)
    for h in range(H):
        rows = np.array([h * S + k for k in range(S) if shader_idx[h, k] >= 0], np.int64)
        inc = np.broadcast_to(np.asarray(incident, dtype=dt)[h, :3], points[h].shape)
        out[h] = transmittance(points[h], reflect(inc, point_normals[h]), vc[rows], vs[rows], vn[rows])
    return out


# ---- a small field of flat (or canted) heliostats, built without the library -------------------------------------------
def flat_heliostat(centre, normal, width=3.21, height=2.55, side=8, cant=0.0, lift=0.0, dtype=np.float64):
    """``(points [4*side*side,4], normals [4*side*side,4])`` of a heliostat of four facets in the layout the rectangle rule
    reads (facet order upper left, upper right, lower left, lower right; inside a facet the north index runs fastest), its
    centre at ``centre``, its plane normal ``normal``; ``cant`` tilts every facet's normal by that angle towards the axis
    (the points stay in the plane); ``lift`` moves the facets off the plane along the normal, the two of one diagonal up and
    the two of the other down."""
    n = np.asarray(normal, dtype) / np.linalg.norm(normal)
    east = np.cross(np.array([0.0, 0.0, 1.0], dtype), n)
    east /= np.linalg.norm(east)
    up = np.cross(n, east)
    pts, nrm = [], []
    e_loc = np.linspace(-width / 4 + 0.01, width / 4 - 0.01, side).astype(dtype)        # (a 2 cm gap between the facets)
    n_loc = np.linspace(-height / 4 + 0.01, height / 4 - 0.01, side).astype(dtype)
    for te, tn in ((-1, 1), (1, 1), (-1, -1), (1, -1)):
        ee, nn = np.meshgrid(te * width / 4 + e_loc, tn * height / 4 + n_loc, indexing="ij")
        pts.append(np.asarray(centre, dtype)[None] + ee.reshape(-1, 1) * east[None] + nn.reshape(-1, 1) * up[None] + (te * tn * lift) * n[None])
        tilted = n - np.tan(cant) * (te * east * 0.7071 + tn * up * 0.7071)
        nrm.append(np.broadcast_to(tilted / np.linalg.norm(tilted), pts[-1].shape))
    p, q = np.concatenate(pts), np.concatenate(nrm)
    return (np.concatenate([p, np.ones((len(p), 1), dtype)], 1).astype(dtype),
            np.concatenate([q, np.zeros((len(q), 1), dtype)], 1).astype(dtype))


def corner_points(points):
    """``corners [H,4,4]`` of surfaces ``[H,P,4]`` by the index rule of create_blocking_primitives_rectangles_by_index."""
    P = points.shape[1]
    side = int(round(np.sqrt(P / 4)))
    return points[:, [P // 2, side - 1, P // 2 - 1, P - side]]


def field(positions, incident, aim, cant=0.0, side=8, lift=0.0, dtype=np.float64):
    """Flat heliostats at ``positions [H,3]``, each turned so that its plane normal bisects the sun and ``aim``:
    ``(points [H,P,4], normals [H,P,4])``."""
    s = -np.asarray(incident, np.float64)[:3]
    out = []
    for pos in np.asarray(positions, np.float64):
        to_aim = np.asarray(aim, np.float64) - pos
        n = s / np.linalg.norm(s) + to_aim / np.linalg.norm(to_aim)
        out.append(flat_heliostat(pos, n, side=side, cant=cant, lift=lift, dtype=np.float64))
    return (np.stack([o[0] for o in out]).astype(dtype), np.stack([o[1] for o in out]).astype(dtype))


def shadow_edge_distance(points, owner, incident, corners):
    """``[H,P]`` metres: how far the sunward ray of every surface point passes from the boundary of the nearest rectangle of
    another heliostat that lies towards the sun (measured in that rectangle's plane, fp64; inf where there is none)."""
    corners = np.asarray(corners, np.float64)
    c0, su, sv, _, normal, _ = rectangles(corners)
    points = np.asarray(points, np.float64)[..., :3]
    out = np.full(points.shape[:2], np.inf)
    for h in range(points.shape[0]):
        s = -np.asarray(incident, np.float64)[h, :3]
        for j in range(corners.shape[0]):
            if j == int(owner[h]):
                continue
            den = s @ normal[j]
            if abs(den) < 1e-9:
                continue
            t = ((c0[j] - points[h]) @ normal[j]) / den
            off = points[h] + t[:, None] * s - c0[j]
            lu, lv = np.linalg.norm(su[j]), np.linalg.norm(sv[j])
            x, y = off @ su[j] / lu, off @ sv[j] / lv              # (rectangles: the spans are orthogonal)
            dx, dy = np.maximum(np.maximum(-x, x - lu), 0.0), np.maximum(np.maximum(-y, y - lv), 0.0)
            inside = np.minimum(np.minimum(x, lu - x), np.minimum(y, lv - y))
            dist = np.where((dx == 0) & (dy == 0), inside, np.sqrt(dx * dx + dy * dy))
            out[h] = np.where(t > 0, np.minimum(out[h], dist), out[h])
    return out


def shadow_edge_length(corners, h, j, incident3):
    """Metres of the outline of rectangle ``j``'s shadow (cast along the sun's rays onto the plane of rectangle ``h``) that lie
    inside rectangle ``h``: the four projected edges clipped to ``h``'s rectangle (Liang-Barsky), fp64."""
    corners = np.asarray(corners, np.float64)[..., :3]
    c0, su, sv, _, normal, _ = rectangles(corners)
    s = -np.asarray(incident3, np.float64)[:3]
    lu, lv = np.linalg.norm(su[h]), np.linalg.norm(sv[h])
    t = ((c0[h] - corners[j]) @ normal[h]) / (s @ normal[h])
    cast = corners[j] + t[:, None] * s - c0[h]
    xy = np.stack((cast @ su[h] / lu, cast @ sv[h] / lv), axis=1)
    total = 0.0
    for a, b in zip(xy, np.roll(xy, -1, axis=0)):
        d, lo, hi = b - a, 0.0, 1.0
        for p, q in ((-d[0], a[0]), (d[0], lu - a[0]), (-d[1], a[1]), (d[1], lv - a[1])):
            if p == 0.0:
                if q < 0.0:
                    lo, hi = 1.0, 0.0
            elif p < 0.0:
                lo = max(lo, q / p)
            else:
                hi = min(hi, q / p)
        total += max(hi - lo, 0.0) * np.linalg.norm(d)
    return total
