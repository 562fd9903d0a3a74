"""Heliostat shading, the part that needs no GPU: the shear identity behind it, the argument checks, and the size of the
approximation on a canted heliostat."""
import ctypes

import numpy as np

import shading_ref as ref


def _random_case(rng):
    """A flat mirror (random plane, sun with s.n >= 0.2), parallelograms 5-40 m sunward of it, points of the mirror plane."""
    n = rng.normal(size=3)
    n /= np.linalg.norm(n)
    while True:
        s = rng.normal(size=3)
        s /= np.linalg.norm(s)
        if s @ n >= 0.2:
            break
    c = rng.uniform(-50, 50, size=3)
    e1 = np.cross(n, rng.normal(size=3))
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(n, e1)
    own = np.stack([c - 1.6 * e1 - 1.3 * e2, c - 1.6 * e1 + 1.3 * e2, c + 1.6 * e1 + 1.3 * e2, c + 1.6 * e1 - 1.3 * e2])
    prims = [own]
    for _ in range(4):
        centre = c + rng.uniform(5, 40) * s + rng.uniform(-2.5, 2.5) * e1 + rng.uniform(-2.5, 2.5) * e2
        a, b = rng.normal(size=3), rng.normal(size=3)
        a, b = a / np.linalg.norm(a) * rng.uniform(1, 4), b / np.linalg.norm(b) * rng.uniform(1, 4)
        c0 = centre - 0.5 * (a + b)
        prims.append(np.stack([c0, c0 + a, c0 + a + b, c0 + b]))
    corners = np.concatenate([np.stack(prims), np.ones((5, 4, 1))], axis=2)
    uv = rng.uniform(-1, 1, size=(400, 2))
    points = c + 1.6 * uv[:, :1] * e1 + 1.3 * uv[:, 1:] * e2
    return corners, -np.append(s, 0.0)[None], points, n, s


def test_shear_identity_in_fp64():
    """On flat mirrors the mask over the sheared tables along the reflected direction equals the mask over the real rectangles
    along the direction to the sun: to 1e-9 in fp64, and the hit parameters (t, u, v) agree."""
    rng = np.random.default_rng(11)
    worst = worst_t = worst_uv = 0.0
    hit = 0
    for _ in range(50):
        corners, incident, points, n, s = _random_case(rng)
        owner = np.array([0])
        idx = np.array([[1, 2, 3, 4]], np.int32)
        vc, vs, vn = ref.shear_tables(corners, owner, incident, idx)
        spans, normals = ref.spans_and_normals(corners)
        d = 2.0 * (s @ n) * n - s
        to_sun = np.broadcast_to(s, points.shape).copy()
        along_d = np.broadcast_to(d, points.shape).copy()
        sig_s, (t_s, u_s, v_s) = ref.soft_sigma(points, to_sun, corners[1:], spans[1:], normals[1:])
        sig_d, (t_d, u_d, v_d) = ref.soft_sigma(points, along_d, vc, vs, vn)
        direct = 1.0 - np.exp(-ref.ALPHA * sig_s.sum(-1))
        sheared = 1.0 - np.exp(-ref.ALPHA * sig_d.sum(-1))
        worst = max(worst, float(np.abs(direct - sheared).max()))
        worst_t = max(worst_t, float(np.abs(t_s / t_d - 1.0).max()))
        worst_uv = max(worst_uv, float(np.abs(u_s - u_d).max()), float(np.abs(v_s - v_d).max()))
        hit += int((direct > 0.5).sum())
    print(f"mask {worst:.2e}, t relative {worst_t:.2e}, (u, v) absolute {worst_uv:.2e}, {hit} shaded rays")
    assert hit > 500                                    # the cases do shade
    assert worst_t < 1e-8 and worst_uv < 1e-9, (worst_t, worst_uv)       # (measured 2.0e-10 and 2.2e-11)
    assert worst < 1e-9, worst


def test_shading_argument_checks_need_no_device():
    from artist_amd import _lib
    lib = _lib.lib()
    p = ctypes.c_void_p(16)                              # (never dereferenced: every call below returns first)
    # empty sizes launch nothing and look at no pointer
    assert lib.art_shading_cull(None, None, None, 0, 5, 0.0, 8, None, None, None) == 0
    assert lib.art_shading_prims_fwd(None, None, None, None, 0, 5, 8, None, None, None, None) == 0
    assert lib.art_shading_prims_bwd(None, None, None, None, None, None, None, 3, 0, 8, None, None, None) == 0
    assert lib.art_shading_append(None, None, 0, 5, 8, 16, None, None, None) == 0
    # bad sizes, whatever the pointers
    for H, N, S in ((-1, 4, 8), (4, -1, 8), (4, 4, 0), (4, 4, 4097), (1 << 23, 4, 8), (4, 1 << 23, 8), (1 << 20, 4, 8)):
        assert lib.art_shading_cull(p, p, p, H, N, 0.0, S, p, p, None) == _lib.ART_EINVAL, (H, N, S)
        assert lib.art_shading_prims_fwd(p, p, p, p, H, N, S, p, p, p, None) == _lib.ART_EINVAL, (H, N, S)
        assert lib.art_shading_prims_bwd(p, p, p, p, p, p, p, H, N, S, p, p, None) == _lib.ART_EINVAL, (H, N, S)
        assert lib.art_shading_append(p, p, H, N, S, 16, p, p, None) == _lib.ART_EINVAL, (H, N, S)
    assert lib.art_shading_cull(p, p, p, 4, 4, -1.0, 8, p, p, None) == _lib.ART_EINVAL          # the scatter bound is the caller's
    assert lib.art_shading_cull(p, p, p, 4, 4, float("nan"), 8, p, p, None) == _lib.ART_EINVAL
    assert lib.art_shading_append(p, p, 4, 4, 8, 0, p, p, None) == _lib.ART_EINVAL
    # null pointers with work to do
    assert lib.art_shading_cull(None, p, p, 4, 4, 0.0, 8, p, p, None) == _lib.ART_EINVAL
    assert lib.art_shading_cull(p, p, p, 4, 4, 0.0, 8, None, p, None) == _lib.ART_EINVAL
    assert lib.art_shading_prims_fwd(p, p, p, None, 4, 4, 8, p, p, p, None) == _lib.ART_EINVAL
    assert lib.art_shading_prims_fwd(p, p, p, p, 4, 4, 8, ctypes.c_void_p(20), p, p, None) == _lib.ART_EINVAL    # alignment
    assert lib.art_shading_prims_bwd(p, p, p, p, p, p, p, 4, 4, 8, None, p, None) == _lib.ART_EINVAL
    assert lib.art_shading_prims_bwd(p, p, p, p, p, p, p, 4, 4, 8, p, None, None) == _lib.ART_EINVAL
    assert lib.art_shading_append(p, p, 4, 4, 8, 16, None, p, None) == _lib.ART_EINVAL


def test_cull_reference_lists_the_shaders_of_a_two_row_field():
    """The rule on a field whose answer is known by eye: under a low sun from the south the front row is free, every heliostat
    of the back row lists the one in front of it, and under a high sun nobody is listed."""
    positions = np.array([[-6.0, 100.0, 0.0], [0.0, 100.0, 0.0], [6.0, 100.0, 0.0], [-6.0, 105.0, 0.0], [0.0, 105.0, 0.0], [6.0, 105.0, 0.0]])
    low = np.array([0.0, np.cos(np.radians(15)), -np.sin(np.radians(15)), 0.0])
    points, _ = ref.field(positions, low, (0.0, 0.0, 55.0))
    corners = ref.corner_points(points)
    incident = np.tile(low, (6, 1))
    listed, margin = ref.cull(corners, np.arange(6), incident, 0.005)
    assert not listed[:3].any()
    for h in (3, 4, 5):
        assert listed[h, h - 3]
    assert margin[np.isfinite(margin)].min() > 1e-4
    listed32, _ = ref.cull(corners.astype(np.float32), np.arange(6), incident.astype(np.float32), 0.005, np.float32)
    assert (listed32 == listed).all()
    high = np.array([0.0, np.cos(np.radians(70)), -np.sin(np.radians(70)), 0.0])
    points, _ = ref.field(positions, high, (0.0, 0.0, 55.0))
    listed, _ = ref.cull(ref.corner_points(points), np.arange(6), np.tile(high, (6, 1)), 0.005)
    assert not listed.any()
    idx, count = ref.cull_lists(np.array([[False, True, True, False, True]]), 2)
    assert idx.tolist() == [[1, 2]] and count.tolist() == [3]


def _shaded_fractions(cant, lift, side=48):
    """Direct and shear shaded power fractions of a heliostat 5 m behind another under a sun 15 degrees up, and the model
    bound evaluated from the scene's own delta, eps, t and edge lengths."""
    positions = np.array([[0.0, 100.0, 0.0], [0.4, 105.0, 0.0]])
    low = np.array([0.0, np.cos(np.radians(15)), -np.sin(np.radians(15)), 0.0])
    points, normals = ref.field(positions, low, (0.0, 0.0, 55.0), cant=cant, side=side, lift=lift)
    corners = ref.corner_points(points)
    incident, owner = np.tile(low, (2, 1)), np.arange(2)
    listed, _ = ref.cull(corners, owner, incident, 0.0)
    idx, count = ref.cull_lists(listed, 8)
    assert count.tolist() == [0, 1]
    direct = 1.0 - ref.direct_transmittance(points, owner, incident, corners)
    sheared = 1.0 - ref.shear_transmittance(points, normals, owner, incident, corners, idx)
    assert float(direct[0].max()) < 1e-9                                  # the front heliostat is free
    c, n, s, sn, sp = ref.own_planes(corners, owner, incident)
    delta = float(np.abs(((points[1, :, :3] - c[1]) * n[1]).sum(-1)).max())
    eps = float(np.arccos(np.clip(np.abs((normals[1, :, :3] * n[1]).sum(-1)), -1, 1)).max())
    t = float(((corners[0, :, None, :3] - corners[1, None, :, :3]) * s[1]).sum(-1).max())
    tan_inc = float(np.linalg.norm(sp[1]) / abs(sn[1]))
    a, b = np.linalg.norm(corners[1, 1, :3] - corners[1, 0, :3]), np.linalg.norm(corners[1, 3, :3] - corners[1, 0, :3])
    pitch = max(a, b) / (2 * side - 1)
    edge = ref.shadow_edge_length(corners, 1, 0, low)
    w = 2.0 * delta * tan_inc + 2.0 * eps * t
    bound = (w + pitch) * (edge + pitch) / (a * b)
    return dict(direct=float(direct[1].mean()), sheared=float(sheared[1].mean()), delta=delta, eps=eps, t=t, w=w, edge=edge,
                pitch=pitch, bound=bound, idx=idx, points=points, normals=normals, corners=corners, owner=owner, incident=incident)


def test_shear_method_on_a_canted_heliostat_stays_within_the_model_bound():
    """The approximation, quantified: a heliostat half shaded by the one in front of it, (a) its facets canted (local normals
    tilted by eps from the rectangle's normal), (b) its facets 8 mm off the plane, (c) both.  Shaded power fraction by the
    direct method - sunward rays, no shear - against the shear method with the true points and normals.  The identity is
    exact for plane points reflecting about the plane's normal; a point delta off the plane moves its shadow edge by up to
    2 delta tan(incidence), a normal tilted by eps by up to 2 eps t at shader distance t.  Only points within that width w
    of the shadow's outline can change sides; a strip of width w along an outline of length L inside the mirror holds at most
    the grid points of a strip (w + pitch) x (L + pitch), so the two fractions differ by at most (w + pitch)(L + pitch)/area,
    with L the length of the shadow's outline inside the mirror (tests/shading_ref.py: shadow_edge_length)."""
    for name, cant, lift in (("canted", 0.004, 0.0), ("off the plane", 0.0, 0.008), ("both", 0.004, 0.008)):
        r = _shaded_fractions(cant, lift)
        diff = abs(r["direct"] - r["sheared"])
        print(f"{name}: shaded fraction direct {r['direct']:.4f}, shear {r['sheared']:.4f}, difference {diff:.2e}; delta {r['delta']:.1e} m, "
              f"eps {r['eps']:.1e} rad, t {r['t']:.2f} m, edge shift <= {r['w']:.3f} m over {r['edge']:.2f} m of outline, bound {r['bound']:.2e}")
        assert 0.2 < r["direct"] < 0.8                                     # half shaded
        # (lifted facets also tilt the rectangle through their corner points: eps and delta are measured against that plane)
        assert (r["eps"] > 3e-3 or cant == 0) and (r["delta"] > 4e-3) == (lift > 0)
        assert diff <= r["bound"], (name, r["direct"], r["sheared"], r["bound"])
    # and flat, in the plane, the two methods are the same thing
    r = _shaded_fractions(0.0, 0.0)
    same = ref.shear_transmittance(r["points"], r["normals"], r["owner"], r["incident"], r["corners"], r["idx"])
    assert np.abs(same - ref.direct_transmittance(r["points"], r["owner"], r["incident"], r["corners"])).max() < 1e-9
