/*
 * oracle_impl.inc - CPU restatement of the ARTIST hot path, precision-generic.
 *
 * TEST INFRASTRUCTURE ONLY.  Included twice by artist_oracle.c (REAL=float, SFX=_f32 and
 * REAL=double, SFX=_f64).  Nothing under artist_amd/ may include, link or call this; only
 * tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg use it, as the checker.
 *
 * Every function restates one piece of the reference (ARTIST v2.0.0, paths relative to
 * /root/reference) in the SAME operation order, with separate roundings (the file is compiled
 * with -ffp-contract=off), because eager PyTorch rounds after every elementwise op.
 * Parity is PINNED: tests/test_oracle_golden.py checks it against fixtures generated from the
 * imported reference (tests/golden/generate_golden.py) and against the reference's own inline
 * known-answer vectors (tests/golden/known_answers.npz).
 */

#define CAT_(a, b) a##b
#define CAT(a, b) CAT_(a, b)
#define FN(name) CAT(name, SFX)

/* ------------------------------------------------------------------------------------------
 * artist/raytracing/geometry.py:11-41  reflect(): i - 2 (i.n) n, all four components, no
 * re-normalisation.  incident [H,4], normals [H,P,4] -> out [H,P,4].
 * ---------------------------------------------------------------------------------------- */
static inline void FN(reflect1)(const REAL *i, const REAL *n, REAL *d)
{
    /* torch.sum over the last dim (size 4) of the elementwise product, sequential. */
    REAL s = ((i[0] * n[0] + i[1] * n[1]) + i[2] * n[2]) + i[3] * n[3];
    REAL s2 = (REAL)2 * s;
    for (int k = 0; k < 4; ++k) d[k] = i[k] - s2 * n[k];
}

int FN(orc_reflect)(const REAL *incident, const REAL *normals, int64_t H, int64_t P, REAL *out)
{
    for (int64_t h = 0; h < H; ++h)
        for (int64_t p = 0; p < P; ++p)
            FN(reflect1)(incident + 4 * h, normals + 4 * (h * P + p), out + 4 * (h * P + p));
    return 0;
}

/* ------------------------------------------------------------------------------------------
 * artist/geometry/transforms.py:52-83 rotate_distortions() + the matmul in
 * artist/raytracing/heliostat_ray_tracer.py:547-552: r = M(e,u) d, rows
 *   [cu, -su, 0, 0], [ce*su, ce*cu, -se, 0], [se*su, se*cu, ce, 0], [0,0,0,1].
 * The 4-term dot products run k = 0..3 sequentially (ATen's small-matrix bmm loop); terms
 * with a literal 0 matrix entry contribute +-0 and are kept so signed zeros match.
 * ---------------------------------------------------------------------------------------- */
static inline void FN(scatter1)(REAL e, REAL u, const REAL *d, REAL *r)
{
    REAL ce = COS(e), se = SIN(e), cu = COS(u), su = SIN(u);
    REAL m10 = ce * su, m11 = ce * cu, m20 = se * su, m21 = se * cu;
    REAL z = (REAL)0;
    r[0] = ((cu * d[0] + (-su) * d[1]) + z * d[2]) + z * d[3];
    r[1] = ((m10 * d[0] + m11 * d[1]) + (-se) * d[2]) + z * d[3];
    r[2] = ((m20 * d[0] + m21 * d[1]) + ce * d[2]) + z * d[3];
    r[3] = ((z * d[0] + z * d[1]) + z * d[2]) + (REAL)1 * d[3];
}

/* Per-heliostat constants of line_plane_intersections (geometry.py:100-104, 145-146). */
typedef struct {
    REAL c[3], m[3];      /* plane centre, plane normal (xyz) */
    REAL w, h;            /* plane dimensions */
    REAL half_w, half_h;  /* dims / 2 */
    REAL wm1, hm1;        /* bitmap_resolution - 1 as REAL */
} FN(plane_t);

/* ------------------------------------------------------------------------------------------
 * artist/raytracing/geometry.py:116-197 for one ray.  `numer` is (c - o).m (per point,
 * geometry.py:126-128).  Outputs the four returned tensors' elements.
 * ---------------------------------------------------------------------------------------- */
static inline void FN(plane1)(const FN(plane_t) * pl, const REAL *o, REAL numer, const REAL *r, REAL mag,
                              REAL *e_px, REAL *u_px, REAL *dist, REAL *inten)
{
    REAL a = (r[0] * pl->m[0] + r[1] * pl->m[1]) + r[2] * pl->m[2];   /* :116-118 */
    int front = a < (REAL)0;                                            /* :119 */
    REAL den = front ? a : (REAL)1;                                     /* :130 */
    REAL t = (numer / den) * (REAL)front;                               /* :131 */
    REAL hx = o[0] + r[0] * t;                                          /* :133-136 (E) */
    REAL hz = o[2] + r[2] * t;                                          /*          (U) */
    REAL I = mag * (-a);                                                /* :139 */
    REAL te = (hx + pl->half_w) - pl->c[0];                             /* :148-152 */
    REAL tu = (hz + pl->half_h) - pl->c[2];                             /* :154-158 */
    REAL be = (te / pl->w) * pl->wm1;                                   /* :165-169 */
    REAL bu = (tu / pl->h) * pl->hm1;                                   /* :170-174 */
    int valid = ((REAL)0 <= be) && (be <= pl->wm1) && ((REAL)0 <= bu) && (bu <= pl->hm1) && front; /* :178-184 */
    REAL v = (REAL)valid;
    be = be * v;                                                        /* :186-189 */
    bu = bu * v;
    t = t * v;
    I = I * v;
    be = pl->wm1 - be;                                                  /* :195-197 */
    *e_px = be; *u_px = bu; *dist = t; *inten = I;
}

/* ------------------------------------------------------------------------------------------
 * artist/raytracing/heliostat_ray_tracer.py:674-770 bilinear_splatting() for one ray into
 * the un-flipped flat bitmap `flat` [Hh*W].  Returns 1 if the ray was splatted.
 * ---------------------------------------------------------------------------------------- */
static inline int FN(splat1)(REAL be, REAL bu, REAL I, int64_t W, int64_t Hh, REAL *flat)
{
    int64_t ie = (int64_t)be, iu = (int64_t)bu;      /* .long(): truncation toward zero (:674-675) */
    REAL cle = (REAL)(ie + 1) - be;                  /* :694 */
    REAL clu = (REAL)(iu + 1) - bu;                  /* :696 */
    REAL che = be - (REAL)ie;                        /* :698 */
    REAL chu = bu - (REAL)iu;                        /* :700 */
    REAL p1 = cle * chu * I, p2 = che * chu * I, p3 = che * clu * I, p4 = cle * clu * I; /* :706-717 */
    int on = (0 <= ie) && (ie + 1 < W) && (0 <= iu) && (iu + 1 < Hh);                    /* :723-728 */
    if (!on) return 0;
    flat[(iu + 1) * W + ie] += p1;                   /* :748,767 */
    flat[(iu + 1) * W + ie + 1] += p2;               /* :749,768 */
    flat[iu * W + ie + 1] += p3;                     /* :750,769 */
    flat[iu * W + ie] += p4;                         /* :751,770 */
    return 1;
}

static void FN(make_plane)(FN(plane_t) * pl, const REAL *centers, const REAL *pnormals, const REAL *dims,
                           int64_t t, int64_t W, int64_t Hh)
{
    for (int k = 0; k < 3; ++k) { pl->c[k] = centers[4 * t + k]; pl->m[k] = pnormals[4 * t + k]; }
    pl->w = dims[2 * t + 0]; pl->h = dims[2 * t + 1];
    pl->half_w = pl->w / (REAL)2; pl->half_h = pl->h / (REAL)2;
    pl->wm1 = (REAL)(W - 1); pl->hm1 = (REAL)(Hh - 1);
}

/* ------------------------------------------------------------------------------------------
 * Cylindrical receivers: artist/raytracing/geometry.py:287-445 for one ray.
 * Per-heliostat constants (:291-300, :399-405).
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    REAL c[3];        /* cylinder centre */
    REAL R[3][3];     /* rows u = n x axis, n, axis  (rotations, :299-300) */
    REAL r2;          /* radius ** 2 (:320) */
    REAL height, half_height, opening;
    REAL ang0;        /* atan2(n_y, n_x) - opening / 2 with the WORLD normal components (:399-405) */
    REAL wm1, hm1;
} FN(cyl_t);

static void FN(make_cyl)(FN(cyl_t) * cy, const REAL *centers, const REAL *normals, const REAL *axes,
                         const REAL *radii, const REAL *heights, const REAL *opening, int64_t t, int64_t W, int64_t Hh)
{
    const REAL *n = normals + 4 * t, *a = axes + 4 * t;
    for (int k = 0; k < 3; ++k) { cy->c[k] = centers[4 * t + k]; cy->R[1][k] = n[k]; cy->R[2][k] = a[k]; }
    cy->R[0][0] = n[1] * a[2] - n[2] * a[1];      /* torch.cross(normals, axes) */
    cy->R[0][1] = n[2] * a[0] - n[0] * a[2];
    cy->R[0][2] = n[0] * a[1] - n[1] * a[0];
    cy->r2 = radii[t] * radii[t];
    cy->height = heights[t]; cy->half_height = heights[t] / (REAL)2; cy->opening = opening[t];
    cy->ang0 = ATAN2(n[1], n[0]) - opening[t] / (REAL)2;
    cy->wm1 = (REAL)(W - 1); cy->hm1 = (REAL)(Hh - 1);
}

/* v @ rotations^T: out_j = sum_k v_k R[j][k], k sequential */
static inline void FN(cyl_rot)(const FN(cyl_t) * cy, const REAL *v, REAL *out)
{
    for (int j = 0; j < 3; ++j) out[j] = (v[0] * cy->R[j][0] + v[1] * cy->R[j][1]) + v[2] * cy->R[j][2];
}

typedef struct {   /* intermediates the backward needs */
    REAL dl[3], a, b, c, sq, t, x, y, rho, nx, ny, abi;
    int near, hit, on;
} FN(cylray_t);

/* ol = (o - centre) @ R^T (per point, :303-305), r = world ray direction. */
static inline void FN(cyl1)(const FN(cyl_t) * cy, const REAL *ol, const REAL *r, REAL mag,
                            REAL *e_px, REAL *u_px, REAL *dist, REAL *inten, FN(cylray_t) * S)
{
    FN(cyl_rot)(cy, r, S->dl);                                                  /* :306 */
    const REAL ox = ol[0], oy = ol[1], dx = S->dl[0], dy = S->dl[1];
    S->a = dx * dx + dy * dy;                                                   /* :318 */
    S->b = (REAL)2 * (ox * dx + oy * dy);                                       /* :319 */
    S->c = (ox * ox + oy * oy) - cy->r2;                                        /* :320 */
    const REAL disc = S->b * S->b - ((REAL)4 * S->a) * S->c;                    /* :322 */
    const int mask = (disc >= (REAL)0) && (FABS(S->a) > (REAL)1e-8);            /* :326 */
    S->sq = SQRT(disc * (REAL)mask + (REAL)1e-12);                              /* :336 */
    REAL tn = (-S->b - S->sq) / ((REAL)2 * S->a), tf = (-S->b + S->sq) / ((REAL)2 * S->a);   /* :343-348 */
    if (!(tn > (REAL)0)) tn = INFINITY;                                         /* :351-355 */
    if (!(tf > (REAL)0)) tf = INFINITY;
    S->near = tn <= tf;                                                         /* torch.min picks the smaller */
    REAL t = S->near ? tn : tf;                                                 /* :356 */
    S->hit = isfinite(t) && mask;                                               /* :357-359 */
    t = S->hit ? t : (REAL)0;                                                   /* :360-364 */
    S->t = t;
    S->x = ol[0] + t * S->dl[0]; S->y = ol[1] + t * S->dl[1];                   /* :374-381 */
    REAL z = ol[2] + t * S->dl[2];
    S->rho = SQRT((S->x * S->x + S->y * S->y) + (REAL)0);                       /* :384-385 */
    S->nx = S->x / S->rho; S->ny = S->y / S->rho;
    REAL dot = ((-S->dl[0]) * S->nx + (-S->dl[1]) * S->ny) + (-S->dl[2]) * ((REAL)0 / S->rho);   /* :388-390 */
    S->abi = dot < (REAL)0 ? (REAL)0 : dot;                                     /* clamp(min=0) (NaN stays NaN) */
    if (dot != dot) S->abi = dot;
    z = z + cy->half_height;                                                    /* :397 */
    const REAL ang = ATAN2(S->y, S->x) - cy->ang0;                              /* :399-405 */
    S->on = (z >= (REAL)0) && (z <= cy->height) && (ang >= (REAL)0) && (ang <= cy->opening);   /* :407-412 */
    const REAL m1 = (REAL)S->on, m2 = (REAL)S->hit;
    *u_px = ((z / cy->height) * cy->hm1) * m1 * m2;                             /* :414-429 */
    *e_px = ((ang / cy->opening) * cy->wm1) * m1 * m2;
    *dist = (t * m1) * m2;                                                      /* :430-432 */
    *inten = ((mag * S->abi) * m1) * m2;                                        /* :433-438 */
}

/* Backward of cyl1: (g_e, g_u, g_I) -> g_ol (local origin, 3) and g_r (world direction, 3). */
static inline void FN(cyl1_bwd)(const FN(cyl_t) * cy, const REAL *ol, REAL mag, const FN(cylray_t) * S,
                                REAL g_e, REAL g_u, REAL g_I, REAL *g_ol, REAL *g_r)
{
    REAL g_dl[3] = {0, 0, 0};
    g_ol[0] = g_ol[1] = g_ol[2] = 0;
    if (S->on && S->hit) {
        const REAL g_ang = g_e * cy->wm1 / cy->opening;
        const REAL g_z = g_u * cy->hm1 / cy->height;
        const REAL rho2 = S->x * S->x + S->y * S->y;
        REAL g_x = g_ang * (-S->y / rho2), g_y = g_ang * (S->x / rho2);
        if (S->abi > (REAL)0) {                       /* clamp passes the gradient only above 0 */
            const REAL g_abi = g_I * mag;
            g_dl[0] += -g_abi * S->nx; g_dl[1] += -g_abi * S->ny;
            const REAL gnx = -g_abi * S->dl[0], gny = -g_abi * S->dl[1];
            const REAL dotn = S->nx * gnx + S->ny * gny;
            g_x += (gnx - S->nx * dotn) / S->rho; g_y += (gny - S->ny * dotn) / S->rho;
        }
        /* intersection = ol + t dl */
        g_ol[0] += g_x; g_ol[1] += g_y; g_ol[2] += g_z;
        g_dl[0] += g_x * S->t; g_dl[1] += g_y * S->t; g_dl[2] += g_z * S->t;
        const REAL g_t = g_x * S->dl[0] + g_y * S->dl[1] + g_z * S->dl[2];
        /* t = (-b -/+ sq) / (2a) */
        const REAL inv2a = (REAL)1 / ((REAL)2 * S->a);
        REAL g_b = -g_t * inv2a;
        const REAL g_sq = (S->near ? -g_t : g_t) * inv2a;
        REAL g_a = -g_t * S->t / S->a;
        const REAL g_disc = g_sq / ((REAL)2 * S->sq);
        g_b += (REAL)2 * S->b * g_disc;
        g_a += (REAL)-4 * S->c * g_disc;
        const REAL g_c = (REAL)-4 * S->a * g_disc;
        g_dl[0] += (REAL)2 * S->dl[0] * g_a + (REAL)2 * ol[0] * g_b;
        g_dl[1] += (REAL)2 * S->dl[1] * g_a + (REAL)2 * ol[1] * g_b;
        g_ol[0] += (REAL)2 * S->dl[0] * g_b + (REAL)2 * ol[0] * g_c;
        g_ol[1] += (REAL)2 * S->dl[1] * g_b + (REAL)2 * ol[1] * g_c;
    }
    for (int k = 0; k < 3; ++k) g_r[k] = g_dl[0] * cy->R[0][k] + g_dl[1] * cy->R[1][k] + g_dl[2] * cy->R[2][k];
}

/* Stage entry points (used by the known-answer tests only). ------------------------------ */

/* rotate_distortions(e,u) @ d for N independent (e,u,d[4]) triples. */
int FN(orc_scatter)(const REAL *e, const REAL *u, const REAL *dirs, int64_t N, REAL *out)
{
    for (int64_t i = 0; i < N; ++i) FN(scatter1)(e[i], u[i], dirs + 4 * i, out + 4 * i);
    return 0;
}

/* line_plane_intersections for N independent rays against ONE plane (target t of the tables). */
int FN(orc_line_plane)(const REAL *dirs, const REAL *mags, const REAL *origins, int64_t N,
                       const REAL *centers, const REAL *pnormals, const REAL *dims, int64_t t, int64_t W, int64_t Hh,
                       REAL *e_px, REAL *u_px, REAL *dist, REAL *inten)
{
    FN(plane_t) pl;
    FN(make_plane)(&pl, centers, pnormals, dims, t, W, Hh);
    for (int64_t i = 0; i < N; ++i) {
        const REAL *o = origins + 4 * i;
        REAL numer = ((pl.c[0] - o[0]) * pl.m[0] + (pl.c[1] - o[1]) * pl.m[1]) + (pl.c[2] - o[2]) * pl.m[2];
        FN(plane1)(&pl, o, numer, dirs + 4 * i, mags[i], e_px + i, u_px + i, dist + i, inten + i);
    }
    return 0;
}

/* line_cylinder_intersections for N independent rays against ONE cylinder (index t of the tables). */
int FN(orc_line_cylinder)(const REAL *dirs, const REAL *mags, const REAL *origins, int64_t N,
                          const REAL *centers, const REAL *normals, const REAL *axes, const REAL *radii,
                          const REAL *heights, const REAL *opening, int64_t t, int64_t W, int64_t Hh,
                          REAL *e_px, REAL *u_px, REAL *dist, REAL *inten)
{
    FN(cyl_t) cy;
    FN(make_cyl)(&cy, centers, normals, axes, radii, heights, opening, t, W, Hh);
    for (int64_t i = 0; i < N; ++i) {
        REAL rel[3] = {origins[4 * i] - cy.c[0], origins[4 * i + 1] - cy.c[1], origins[4 * i + 2] - cy.c[2]}, ol[3];
        FN(cyl_rot)(&cy, rel, ol);
        FN(cylray_t) S;
        FN(cyl1)(&cy, ol, dirs + 4 * i, mags[i], e_px + i, u_px + i, dist + i, inten + i, &S);
    }
    return 0;
}

/* bilinear_splatting of N rays into one bitmap [Hh,W] (zeroed here, flipped like :778). */
int FN(orc_splat)(const REAL *e_px, const REAL *u_px, const REAL *inten, int64_t N, int64_t W, int64_t Hh, REAL *bitmap)
{
    REAL *flat = (REAL *)calloc((size_t)(W * Hh), sizeof(REAL));
    if (!flat) return -3;
    for (int64_t i = 0; i < N; ++i) FN(splat1)(e_px[i], u_px[i], inten[i], W, Hh, flat);
    for (int64_t row = 0; row < Hh; ++row)
        memcpy(bitmap + row * W, flat + (Hh - 1 - row) * W, (size_t)W * sizeof(REAL));
    free(flat);
    return 0;
}

/* ------------------------------------------------------------------------------------------
 * Blocking: artist/raytracing/blocking.py.
 *
 * Primitive tables use the reference's layout: corners [N,4,4], spans [N,2,4], normals [N,4]
 * (create_blocking_primitives_rectangles_by_index, :123-209).
 * ---------------------------------------------------------------------------------------- */

/* blocking.py:170-207: corners picked by point index from [N,P,4] aligned surfaces (four facets of
 * sqrt(P/4)^2 row-major points), spans = corner1 - corner0 / corner3 - corner0, normal = normalize(su x sv). */
int FN(orc_blocking_primitives)(const REAL *surfaces, int64_t N, int64_t P, REAL *corners, REAL *spans, REAL *pnormals)
{
    const int64_t side = (int64_t)sqrt((double)P / 4.0);
    const int64_t idx[4] = {(int64_t)((double)P / 2.0), (int64_t)(sqrt((double)P / 4.0) - 1.0),
                            (int64_t)((double)P / 2.0 - 1.0), (int64_t)((double)P - sqrt((double)P / 4.0))};
    (void)side;
    for (int64_t i = 0; i < N; ++i) {
        for (int c = 0; c < 4; ++c)
            for (int k = 0; k < 4; ++k) corners[(i * 4 + c) * 4 + k] = surfaces[(i * P + idx[c]) * 4 + k];
        REAL *c0 = corners + (i * 4 + 0) * 4, *c1 = corners + (i * 4 + 1) * 4, *c3 = corners + (i * 4 + 3) * 4;
        REAL *su = spans + (i * 2 + 0) * 4, *sv = spans + (i * 2 + 1) * 4;
        for (int k = 0; k < 4; ++k) { su[k] = c1[k] - c0[k]; sv[k] = c3[k] - c0[k]; }
        REAL cx = su[1] * sv[2] - su[2] * sv[1], cy = su[2] * sv[0] - su[0] * sv[2], cz = su[0] * sv[1] - su[1] * sv[0];
        REAL nn = SQRT((cx * cx + cy * cy) + cz * cz);
        if (nn < (REAL)1e-12) nn = (REAL)1e-12;               /* F.normalize eps */
        pnormals[4 * i] = cx / nn; pnormals[4 * i + 1] = cy / nn; pnormals[4 * i + 2] = cz / nn; pnormals[4 * i + 3] = 0;
    }
    return 0;
}

static inline REAL FN(sigmoid)(REAL x) { return (REAL)1 / ((REAL)1 + EXP(-x)); }

/* ray vs the axis-aligned box of the four corners of primitive k: blocking.py:787-791 + the hit test :928-932.
 * The reference walks an LBVH (:357-995); an internal node's box contains its children's, entry/exit distances are
 * monotone in the box bounds, so a leaf is reached exactly when its own box passes this test: the traversal
 * result equals the brute-force loop over the primitives restated here (pinned on reference-generated vectors). */
static inline int FN(aabb_hit)(const REAL *corners4, const REAL *o, const REAL *dir, REAL t_target)
{
    REAL entry = -INFINITY, exit_ = INFINITY;
    for (int k = 0; k < 3; ++k) {
        REAL lo = corners4[k], hi = corners4[k];
        for (int c = 1; c < 4; ++c) {
            REAL v = corners4[4 * c + k];
            if (v < lo) lo = v;
            if (v > hi) hi = v;
        }
        const REAL inv = (REAL)1 / (dir[k] + (REAL)1e-12);                          /* :912 */
        const REAL t0 = (lo - o[k]) * inv, t1 = (hi - o[k]) * inv;
        const REAL tmin = t0 < t1 ? t0 : t1, tmax = t0 < t1 ? t1 : t0;
        if (tmin > entry) entry = tmin;
        if (tmax < exit_) exit_ = tmax;
    }
    return (exit_ >= entry) && (exit_ > (REAL)1e-6) && (entry <= t_target);
}

/* ------------------------------------------------------------------------------------------
 * The reference's LBVH (blocking.py:357-749), restated node by node.
 *
 * build_linear_bounding_volume_hierarchies follows Karras (2012) but halves the step of the split search by
 * floor division (:640-650, "t = t // 2" from (l + 1) // 2) instead of the ceil schedule of the paper, so for
 * more than ~4 primitives some splits land on the wrong position: part of the internal nodes - and with them
 * their leaves - hang off no path from the root, and lbvh_filter_blocking_planes (:832-995) can never return
 * those primitives.  Which primitives stay reachable is therefore part of the reference's observable result,
 * and this restatement reproduces it: live[k] = 1 iff the leaf of primitive k can be reached from node 0
 * through internal nodes whose boxes were completed by the bottom-up pass (:705-733).
 * For a live leaf the traversal itself adds nothing: every box on the path contains the leaf's box and
 * entry/exit distances are monotone in the box bounds, so the leaf is reported exactly when its own box passes
 * the test (aabb_hit above).
 * ---------------------------------------------------------------------------------------- */
static inline int32_t FN(expand_bits)(int32_t v)                                  /* :357-389 */
{
    uint32_t x = (uint32_t)v & 0x3FFu;
    x = (x | (x << 16)) & 0x030000FFu;
    x = (x | (x << 8)) & 0x0300F00Fu;
    x = (x | (x << 4)) & 0x030C30C3u;
    x = (x | (x << 2)) & 0x09249249u;
    return (int32_t)x;
}

static inline int FN(lcp)(const int32_t *codes, int64_t N, int64_t i, int64_t j)   /* :446-510 */
{
    if (j < 0 || j >= N) return -1;
    const uint32_t x = (uint32_t)(codes[i] ^ codes[j]);
    if (x == 0) return 30;
    int msb = 31;
    while (!((x >> msb) & 1u)) --msb;
    return 29 - msb;
}

int FN(orc_lbvh_live)(const REAL *corners, int64_t N, int32_t *live)
{
    if (N <= 0) return 0;
    if (N == 1) { live[0] = 1; return 0; }                                       /* the root is the only leaf */
    REAL *cen = (REAL *)malloc((size_t)(3 * N) * sizeof(REAL));
    int32_t *codes = (int32_t *)malloc((size_t)N * sizeof(int32_t));
    int32_t *order = (int32_t *)malloc((size_t)N * sizeof(int32_t));
    int32_t *left = (int32_t *)malloc((size_t)N * sizeof(int32_t)), *right = (int32_t *)malloc((size_t)N * sizeof(int32_t));
    char *complete = (char *)calloc((size_t)N, 1), *reach = (char *)calloc((size_t)(2 * N), 1);
    if (!cen || !codes || !order || !left || !right || !complete || !reach) return -3;
    /* centroids (:570) and Morton codes (:392-443): n bits above e bits above u bits */
    REAL mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t k = 0; k < N; ++k)
        for (int a = 0; a < 3; ++a) {
            const REAL *c = corners + 16 * k + a;
            const REAL m = (((c[0] + c[4]) + c[8]) + c[12]) / (REAL)4;
            cen[3 * k + a] = m;
            if (m < mn[a]) mn[a] = m;
            if (m > mx[a]) mx[a] = m;
        }
    REAL span = mx[0] - mn[0];
    if (mx[1] - mn[1] > span) span = mx[1] - mn[1];
    if (mx[2] - mn[2] > span) span = mx[2] - mn[2];
    const REAL scale = (REAL)1023 / (span + (REAL)1e-6);
    for (int64_t k = 0; k < N; ++k) {
        const int32_t e = (int32_t)((cen[3 * k] - mn[0]) * scale), n = (int32_t)((cen[3 * k + 1] - mn[1]) * scale),
                      u = (int32_t)((cen[3 * k + 2] - mn[2]) * scale);
        codes[k] = (FN(expand_bits)(n) << 2) | (FN(expand_bits)(e) << 1) | FN(expand_bits)(u);
        order[k] = (int32_t)k;
    }
    /* stable insertion sort by code (:573) */
    for (int64_t a = 1; a < N; ++a) {
        const int32_t c = codes[a], o = order[a];
        int64_t b = a - 1;
        while (b >= 0 && codes[b] > c) { codes[b + 1] = codes[b]; order[b + 1] = order[b]; --b; }
        codes[b + 1] = c; order[b + 1] = o;
    }
    const int64_t leaf_offset = N - 1;
    for (int64_t i = 0; i < N - 1; ++i) {                                          /* internal nodes only */
        const int lr = FN(lcp)(codes, N, i, i + 1), ll = FN(lcp)(codes, N, i, i - 1);
        const int64_t d = lr > ll ? 1 : -1;                                        /* :595 */
        const int dmin = lr < ll ? lr : ll;                                        /* :600 */
        int64_t lmax = 2;                                                          /* :604-615 */
        while (FN(lcp)(codes, N, i, i + lmax * d) > dmin) lmax *= 2;
        int64_t l = 0;                                                             /* :617-628 */
        for (int64_t t = lmax / 2; t >= 1; t /= 2)
            if (FN(lcp)(codes, N, i, i + (l + t) * d) > dmin) l += t;
        const int64_t j = i + l * d;                                               /* :630 */
        const int dnode = FN(lcp)(codes, N, i, j);                                 /* :635-637 */
        int64_t split = 0;                                                         /* :638-650, floor halving */
        for (int64_t t = (l + 1) / 2; t >= 1; t /= 2)
            if (FN(lcp)(codes, N, i, i + (split + t) * d) > dnode) split += t;
        const int64_t gamma = i + split * d + (d < 0 ? d : 0);                     /* :652-656 */
        const int64_t lo = i < j ? i : j, hi = i < j ? j : i;
        left[i] = (int32_t)(lo == gamma ? leaf_offset + gamma : gamma);            /* :689-693 */
        right[i] = (int32_t)(hi == gamma + 1 ? leaf_offset + gamma + 1 : gamma + 1);   /* :695-699 */
    }
    /* bottom-up box pass (:705-733): an internal node is complete once both children are leaves or complete */
    for (int64_t round = 0, changed = 1; changed && round < 2 * (N - 1); ++round) {
        changed = 0;
        for (int64_t i = 0; i < N - 1; ++i) {
            if (complete[i]) continue;
            const int l_ok = left[i] >= leaf_offset || (left[i] >= 0 && complete[left[i]]);
            const int r_ok = right[i] >= leaf_offset || (right[i] >= 0 && complete[right[i]]);
            if (l_ok && r_ok) { complete[i] = 2; changed = 1; }
        }
        for (int64_t i = 0; i < N - 1; ++i)
            if (complete[i] == 2) complete[i] = 1;                                 /* visible from the next round on */
    }
    /* top-down: nodes a ray can get to.  An incomplete node keeps the all-zero box it was created with (:666-667),
     * which no ray of a heliostat field passes through. */
    for (int64_t k = 0; k < N; ++k) live[k] = 0;
    if (complete[0]) {
        reach[0] = 1;
        for (int64_t changed = 1; changed;) {
            changed = 0;
            for (int64_t i = 0; i < N - 1; ++i) {
                if (!reach[i]) continue;
                const int32_t ch[2] = {left[i], right[i]};
                for (int c = 0; c < 2; ++c) {
                    if (ch[c] < 0 || ch[c] >= 2 * N - 1 || reach[ch[c]]) continue;
                    if (ch[c] >= leaf_offset || complete[ch[c]]) { reach[ch[c]] = 1; changed = 1; }
                }
            }
        }
        for (int64_t k = 0; k < N; ++k)
            if (reach[leaf_offset + k]) live[order[k]] = 1;
    }
    free(cen); free(codes); free(order); free(left); free(right); free(complete); free(reach);
    return 0;
}

/* Stage entry: lbvh_filter_blocking_planes (:832-995) for NR independent rays: flags[k] = 1 iff primitive k is
 * live in the reference's tree (compat != 0; every primitive is live otherwise) and some ray whose owner is not
 * k passes aabb_hit for it. */
int FN(orc_blocking_filter)(const REAL *origins3, const REAL *dirs3, const REAL *t_target, const int32_t *owner,
                            int64_t NR, const REAL *corners, int64_t N, int compat, int32_t *flags)
{
    int32_t *live = (int32_t *)malloc((size_t)(N > 0 ? N : 1) * sizeof(int32_t));
    if (!live) return -3;
    for (int64_t k = 0; k < N; ++k) { flags[k] = 0; live[k] = 1; }
    if (compat) FN(orc_lbvh_live)(corners, N, live);
    for (int64_t i = 0; i < NR; ++i)
        for (int64_t k = 0; k < N; ++k)
            if (live[k] && !flags[k] && owner[i] != k &&
                FN(aabb_hit)(corners + 16 * k, origins3 + 3 * i, dirs3 + 3 * i, t_target[i]))
                flags[k] = 1;
    free(live);
    return 0;
}

typedef struct {   /* per (ray, primitive) intermediates of soft_ray_blocking_mask (:314-354) */
    REAL den, den_safe, d, f, off[3], suu, svv, suv, pu, pv, det, det_safe, u, v, Au, Bu, Av, Bv, sigma_raw;
} FN(soft_t);

#define ORC_SOFTNESS ((REAL)1000)
#define ORC_ALPHA ((REAL)100)
#define ORC_OFFSET ((REAL)0.05)
#define ORC_EPS ((REAL)1e-12)

/* sigma of one ray against one primitive (c0 = corner 0, su/sv spans, n normal; xyz only). */
static inline REAL FN(soft1)(const REAL *c0, const REAL *su, const REAL *sv, const REAL *n, const REAL *o,
                             const REAL *dir, FN(soft_t) * S)
{
    S->den = (dir[0] * n[0] + dir[1] * n[1]) + dir[2] * n[2];                                   /* :315 */
    S->den_safe = FABS(S->den) < ORC_EPS ? (S->den >= (REAL)0 ? ORC_EPS : -ORC_EPS) : S->den;   /* :316-320 */
    const REAL num = ((c0[0] - o[0]) * n[0] + (c0[1] - o[1]) * n[1]) + (c0[2] - o[2]) * n[2];   /* :322 */
    S->d = num / S->den_safe;                                                                   /* :321-324 */
    S->f = FN(sigmoid)(ORC_SOFTNESS * (S->d - ORC_OFFSET));                                     /* :325-327 */
    for (int k = 0; k < 3; ++k) S->off[k] = (o[k] + S->d * dir[k]) - c0[k];                     /* :328-331 */
    S->suu = (su[0] * su[0] + su[1] * su[1]) + su[2] * su[2];                                   /* :333-335 */
    S->svv = (sv[0] * sv[0] + sv[1] * sv[1]) + sv[2] * sv[2];
    S->suv = (su[0] * sv[0] + su[1] * sv[1]) + su[2] * sv[2];
    S->pu = (S->off[0] * su[0] + S->off[1] * su[1]) + S->off[2] * su[2];                        /* :336-337 */
    S->pv = (S->off[0] * sv[0] + S->off[1] * sv[1]) + S->off[2] * sv[2];
    S->det = S->suu * S->svv - S->suv * S->suv;                                                 /* :338 */
    const REAL sgn = S->det > (REAL)0 ? (REAL)1 : (S->det < (REAL)0 ? (REAL)-1 : (REAL)0);
    S->det_safe = FABS(S->det) < ORC_EPS ? sgn * ORC_EPS : S->det;                              /* :339 */
    S->u = (S->pu * S->svv - S->pv * S->suv) / S->det_safe;                                     /* :340-345 */
    S->v = (S->pv * S->suu - S->pu * S->suv) / S->det_safe;
    S->Au = FN(sigmoid)(ORC_SOFTNESS * S->u); S->Bu = FN(sigmoid)(ORC_SOFTNESS * ((REAL)1 - S->u));   /* :353-358 */
    S->Av = FN(sigmoid)(ORC_SOFTNESS * S->v); S->Bv = FN(sigmoid)(ORC_SOFTNESS * ((REAL)1 - S->v));
    const REAL inside = (S->Au * S->Bu) * (S->Av * S->Bv);                                      /* :359 */
    S->sigma_raw = inside * S->f;                                                               /* :360 */
    REAL sg = S->sigma_raw;
    if (sg < (REAL)0) sg = 0;                                                                   /* :361 clamp */
    if (sg > (REAL)1) sg = 1;
    return sg;
}

/* adjoint of soft1: g_sigma = dL/dsigma -> accumulates into g_o, g_dir (ray) and g_c0, g_su, g_sv, g_n (primitive) */
static inline void FN(soft1_bwd)(const REAL *c0, const REAL *su, const REAL *sv, const REAL *n, const REAL *o,
                                 const REAL *dir, const FN(soft_t) * S, REAL g_sigma, REAL *g_o, REAL *g_dir,
                                 REAL *g_c0, REAL *g_su, REAL *g_sv, REAL *g_n)
{
    if (!(S->sigma_raw >= (REAL)0 && S->sigma_raw <= (REAL)1)) return;          /* clamp passes inside [0,1] */
    const REAL s = ORC_SOFTNESS;
    const REAL iu = S->Au * S->Bu, iv = S->Av * S->Bv;
    const REAL g_u = g_sigma * iv * S->f * (s * iu * (S->Bu - S->Au));
    const REAL g_v = g_sigma * iu * S->f * (s * iv * (S->Bv - S->Av));
    REAL g_d = g_sigma * iu * iv * (S->f * ((REAL)1 - S->f) * s);
    const REAL idet = (REAL)1 / S->det_safe;
    const REAL g_pu = (g_u * S->svv - g_v * S->suv) * idet;
    const REAL g_pv = (g_v * S->suu - g_u * S->suv) * idet;
    REAL g_svv = g_u * S->pu * idet, g_suu = g_v * S->pv * idet, g_suv = -(g_u * S->pv + g_v * S->pu) * idet;
    if (!(FABS(S->det) < ORC_EPS)) {
        const REAL g_det = -(g_u * S->u + g_v * S->v) * idet;
        g_suu += g_det * S->svv; g_svv += g_det * S->suu; g_suv += (REAL)-2 * S->suv * g_det;
    }
    REAL g_off[3];
    for (int k = 0; k < 3; ++k) {
        g_off[k] = g_pu * su[k] + g_pv * sv[k];
        g_su[k] += g_pu * S->off[k] + (REAL)2 * g_suu * su[k] + g_suv * sv[k];
        g_sv[k] += g_pv * S->off[k] + (REAL)2 * g_svv * sv[k] + g_suv * su[k];
    }
    for (int k = 0; k < 3; ++k) { g_o[k] += g_off[k]; g_dir[k] += S->d * g_off[k]; g_c0[k] -= g_off[k]; g_d += g_off[k] * dir[k]; }
    const REAL g_num = g_d / S->den_safe;
    const REAL g_den = FABS(S->den) < ORC_EPS ? (REAL)0 : -g_d * S->d / S->den_safe;
    for (int k = 0; k < 3; ++k) {
        g_c0[k] += g_num * n[k]; g_o[k] -= g_num * n[k]; g_n[k] += g_num * (c0[k] - o[k]) + g_den * dir[k];
        g_dir[k] += g_den * n[k];
    }
}

/* Stage entry: soft_ray_blocking_mask (:212-354) for NR independent rays against K primitives (all of them). */
int FN(orc_soft_blocking)(const REAL *origins3, const REAL *dirs3, int64_t NR, const REAL *corners, const REAL *spans,
                          const REAL *pnormals, int64_t K, REAL *blocked)
{
    for (int64_t i = 0; i < NR; ++i) {
        REAL sum = 0;
        for (int64_t k = 0; k < K; ++k) {
            FN(soft_t) S;
            sum += FN(soft1)(corners + 16 * k, spans + 8 * k, spans + 8 * k + 4, pnormals + 4 * k, origins3 + 3 * i,
                             dirs3 + 3 * i, &S);
        }
        blocked[i] = (REAL)1 - EXP(-(ORC_ALPHA * sum));                                         /* :362-365 */
    }
    return 0;
}

/* One ray of trace_rays up to the target hit: reflect -> scatter -> plane / cylinder intersection. */
typedef struct {
    const REAL *origins, *normals, *incident, *dist_u, *dist_e;
    int64_t sh, sr, sp;
    REAL mag;
} FN(rayctx_t);

static inline void FN(ray_to_target)(const FN(rayctx_t) * c, int is_cyl, const FN(plane_t) * pl, const FN(cyl_t) * cy,
                                     int64_t h, int64_t r, int64_t p, int64_t P, REAL *rr, REAL *be, REAL *bu,
                                     REAL *t, REAL *I)
{
    const REAL *o = c->origins + 4 * (h * P + p);
    REAL d[4];
    FN(reflect1)(c->incident + 4 * h, c->normals + 4 * (h * P + p), d);
    REAL u = c->dist_u[h * c->sh + r * c->sr + p * c->sp], e = c->dist_e[h * c->sh + r * c->sr + p * c->sp];
    FN(scatter1)(e, u, d, rr);
    if (is_cyl) {
        REAL rel[3] = {o[0] - cy->c[0], o[1] - cy->c[1], o[2] - cy->c[2]}, ol[3];
        FN(cyl_rot)(cy, rel, ol);
        FN(cylray_t) S;
        FN(cyl1)(cy, ol, rr, c->mag, be, bu, t, I, &S);
    } else {
        REAL numer = ((pl->c[0] - o[0]) * pl->m[0] + (pl->c[1] - o[1]) * pl->m[1]) + (pl->c[2] - o[2]) * pl->m[2];
        FN(plane1)(pl, o, numer, rr, c->mag, be, bu, t, I);
    }
}

/* heliostat_ray_tracer.py:444-461: the set of blocking primitives the soft mask is evaluated against = every
 * primitive whose box is hit by at least one ray of the batch (all heliostats in one batch here) that does not
 * belong to the primitive's own heliostat (owner[h] = its index among the primitives). */
static void FN(blocking_flags)(const FN(rayctx_t) * c, const int32_t *target_idx, const REAL *centers,
                               const REAL *pnormals, const REAL *dims, const REAL *cyl_centers, const REAL *cyl_normals,
                               const REAL *cyl_axes, const REAL *cyl_radii, const REAL *cyl_heights,
                               const REAL *cyl_opening, int64_t H, int64_t R, int64_t P, int64_t T, int64_t W, int64_t Hh,
                               const REAL *prim_corners, const int32_t *owner, int64_t N, int compat, int32_t *flags)
{
    int32_t *live = (int32_t *)malloc((size_t)(N > 0 ? N : 1) * sizeof(int32_t));
    for (int64_t k = 0; k < N; ++k) { flags[k] = 0; live[k] = 1; }
    if (compat) FN(orc_lbvh_live)(prim_corners, N, live);
    for (int64_t h = 0; h < H; ++h) {
        const int is_cyl = target_idx[h] >= T;
        FN(plane_t) pl;
        FN(cyl_t) cy;
        if (is_cyl) FN(make_cyl)(&cy, cyl_centers, cyl_normals, cyl_axes, cyl_radii, cyl_heights, cyl_opening, target_idx[h] - T, W, Hh);
        else FN(make_plane)(&pl, centers, pnormals, dims, target_idx[h], W, Hh);
        for (int64_t r = 0; r < R; ++r)
            for (int64_t p = 0; p < P; ++p) {
                REAL rr[4], be, bu, t, I;
                FN(ray_to_target)(c, is_cyl, &pl, &cy, h, r, p, P, rr, &be, &bu, &t, &I);
                for (int64_t k = 0; k < N; ++k)
                    if (live[k] && !flags[k] && owner[h] != k &&
                        FN(aabb_hit)(prim_corners + 16 * k, c->origins + 4 * (h * P + p), rr, t))
                        flags[k] = 1;
            }
    }
    free(live);
}

/* ------------------------------------------------------------------------------------------
 * Flux epilogue: artist/flux/bitmap.py:121-246 crop_flux_distributions_around_center.
 *   flux [B,Hh,W]; dims [B,2] = (width, height) in metres of each bitmap's target area (the gather of
 *   :183-216 is host logic); out [B,Hh,W]; com [B,3] (optional) = x centre, y centre, sum + 1e-8.
 * ---------------------------------------------------------------------------------------- */
static inline REAL FN(lin)(int64_t k, int64_t n)       /* torch.linspace(-1, 1, n)[k] */
{
    if (n == 1) return (REAL)-1;
    const REAL step = (REAL)2 / (REAL)(n - 1);
    /* torch fills the first half from the start and the second half from the end */
    return k < n / 2 ? (REAL)-1 + step * (REAL)k : (REAL)1 - step * (REAL)(n - 1 - k);
}

int FN(orc_flux_crop_fwd)(const REAL *flux, const REAL *dims, int64_t B, int64_t Hh, int64_t W, double crop_w,
                          double crop_h, REAL *out, REAL *com)
{
    for (int64_t b = 0; b < B; ++b) {
        const REAL *f = flux + b * Hh * W;
        REAL S = 0;
        for (int64_t k = 0; k < Hh * W; ++k) S += f[k];
        S += (REAL)1e-8;                                                            /* :165-171 */
        REAL xc = 0, yc = 0;
        for (int64_t y = 0; y < Hh; ++y)
            for (int64_t x = 0; x < W; ++x) {
                const REAL nm = f[y * W + x] / S;
                xc += FN(lin)(x, W) * nm; yc += FN(lin)(y, Hh) * nm;               /* :172-182 */
            }
        REAL width = dims[2 * b], height = dims[2 * b + 1];
        if (width < (REAL)1e-8) width = (REAL)1e-8;                                 /* :218-221 */
        if (height < (REAL)1e-8) height = (REAL)1e-8;
        const REAL sx = (REAL)crop_w / width, sy = (REAL)crop_h / height;           /* :223-225 */
        if (com) { com[3 * b] = xc; com[3 * b + 1] = yc; com[3 * b + 2] = S; }
        for (int64_t i = 0; i < Hh; ++i) {
            const REAL gy = sy * FN(lin)(i, Hh) + yc;                               /* affine_grid, align_corners=True */
            const REAL iy = ((gy + (REAL)1) / (REAL)2) * (REAL)(Hh - 1);            /* grid_sample unnormalize */
            const REAL y0f = FLOOR(iy);
            const REAL ty = iy - y0f;
            const int64_t y0 = (int64_t)y0f;
            for (int64_t j = 0; j < W; ++j) {
                const REAL gx = sx * FN(lin)(j, W) + xc;
                const REAL ix = ((gx + (REAL)1) / (REAL)2) * (REAL)(W - 1);
                const REAL x0f = FLOOR(ix);
                const REAL tx = ix - x0f;
                const int64_t x0 = (int64_t)x0f;
                REAL acc = 0;
                /* bilinear, zeros padding: nw, ne, sw, se */
                if (y0 >= 0 && y0 < Hh && x0 >= 0 && x0 < W) acc += f[y0 * W + x0] * (((REAL)1 - tx) * ((REAL)1 - ty));
                if (y0 >= 0 && y0 < Hh && x0 + 1 >= 0 && x0 + 1 < W) acc += f[y0 * W + x0 + 1] * (tx * ((REAL)1 - ty));
                if (y0 + 1 >= 0 && y0 + 1 < Hh && x0 >= 0 && x0 < W) acc += f[(y0 + 1) * W + x0] * (((REAL)1 - tx) * ty);
                if (y0 + 1 >= 0 && y0 + 1 < Hh && x0 + 1 >= 0 && x0 + 1 < W) acc += f[(y0 + 1) * W + x0 + 1] * (tx * ty);
                out[(b * Hh + i) * W + j] = acc;
            }
        }
    }
    return 0;
}

/* autograd of the above w.r.t. flux: through the sampled values, and through the centre of mass that places the
 * sampling grid (grid_sample's gradient w.r.t. its grid, affine_grid, the normalised first moments). */
int FN(orc_flux_crop_bwd)(const REAL *flux, const REAL *dims, int64_t B, int64_t Hh, int64_t W, double crop_w,
                          double crop_h, const REAL *grad_out, REAL *grad_flux)
{
    for (int64_t b = 0; b < B; ++b) {
        const REAL *f = flux + b * Hh * W, *g = grad_out + b * Hh * W;
        REAL *gf = grad_flux + b * Hh * W;
        REAL S = 0;
        for (int64_t k = 0; k < Hh * W; ++k) { S += f[k]; gf[k] = 0; }
        S += (REAL)1e-8;
        REAL xc = 0, yc = 0;
        for (int64_t y = 0; y < Hh; ++y)
            for (int64_t x = 0; x < W; ++x) {
                const REAL nm = f[y * W + x] / S;
                xc += FN(lin)(x, W) * nm; yc += FN(lin)(y, Hh) * nm;
            }
        REAL width = dims[2 * b], height = dims[2 * b + 1];
        if (width < (REAL)1e-8) width = (REAL)1e-8;
        if (height < (REAL)1e-8) height = (REAL)1e-8;
        const REAL sx = (REAL)crop_w / width, sy = (REAL)crop_h / height;
        REAL g_xc = 0, g_yc = 0;
        for (int64_t i = 0; i < Hh; ++i) {
            const REAL gy = sy * FN(lin)(i, Hh) + yc;
            const REAL iy = ((gy + (REAL)1) / (REAL)2) * (REAL)(Hh - 1);
            const REAL y0f = FLOOR(iy), ty = iy - y0f;
            const int64_t y0 = (int64_t)y0f;
            for (int64_t j = 0; j < W; ++j) {
                const REAL gx = sx * FN(lin)(j, W) + xc;
                const REAL ix = ((gx + (REAL)1) / (REAL)2) * (REAL)(W - 1);
                const REAL x0f = FLOOR(ix), tx = ix - x0f;
                const int64_t x0 = (int64_t)x0f;
                const REAL go = g[i * W + j];
                REAL v[2][2];
                for (int dy = 0; dy < 2; ++dy)
                    for (int dx = 0; dx < 2; ++dx) {
                        const int64_t yy = y0 + dy, xx = x0 + dx;
                        const int in = yy >= 0 && yy < Hh && xx >= 0 && xx < W;
                        v[dy][dx] = in ? f[yy * W + xx] : (REAL)0;
                        if (in) gf[yy * W + xx] += go * ((dx ? tx : (REAL)1 - tx) * (dy ? ty : (REAL)1 - ty));
                    }
                const REAL d_ix = (v[0][1] - v[0][0]) * ((REAL)1 - ty) + (v[1][1] - v[1][0]) * ty;
                const REAL d_iy = (v[1][0] - v[0][0]) * ((REAL)1 - tx) + (v[1][1] - v[0][1]) * tx;
                g_xc += go * d_ix * ((REAL)(W - 1) / (REAL)2);
                g_yc += go * d_iy * ((REAL)(Hh - 1) / (REAL)2);
            }
        }
        for (int64_t y = 0; y < Hh; ++y)
            for (int64_t x = 0; x < W; ++x)
                gf[y * W + x] += g_xc * (FN(lin)(x, W) - xc) / S + g_yc * (FN(lin)(y, Hh) - yc) / S;
    }
    return 0;
}

/* artist/optim/loss.py:251-318 PixelLoss, reduction over the two bitmap dimensions:
 * loss[b] = sum (p - g)^2 / sum g ;  grad_pred = dL/dloss[b] * 2 (p - g) / sum g  (when grad_pred != NULL). */
int FN(orc_pixel_loss)(const REAL *pred, const REAL *truth, int64_t B, int64_t npix, REAL *loss, const REAL *grad_loss,
                       REAL *grad_pred)
{
    for (int64_t b = 0; b < B; ++b) {
        const REAL *p = pred + b * npix, *g = truth + b * npix;
        REAL se = 0, sg = 0;
        for (int64_t k = 0; k < npix; ++k) { const REAL d = p[k] - g[k]; se += d * d; sg += g[k]; }
        loss[b] = se / sg;
        if (grad_pred)
            for (int64_t k = 0; k < npix; ++k) grad_pred[b * npix + k] = grad_loss[b] * ((REAL)2 * (p[k] - g[k])) / sg;
    }
    return 0;
}

/* artist/optim/loss.py:321-410 KLDivergenceLoss: both bitmaps L1-normalised (F.normalize p=1, eps 1e-12), then
 * KLDivLoss(log_target=True) on log(. + 1e-12): loss[b] = sum exp(t) (t - q), t = log(P + eps), q = log(Q + eps). */
int FN(orc_kl_loss)(const REAL *pred, const REAL *truth, int64_t B, int64_t npix, REAL *loss, const REAL *grad_loss,
                    REAL *grad_pred)
{
    const REAL eps = (REAL)1e-12;
    for (int64_t b = 0; b < B; ++b) {
        const REAL *p = pred + b * npix, *g = truth + b * npix;
        REAL np_ = 0, ng = 0;
        for (int64_t k = 0; k < npix; ++k) { np_ += FABS(p[k]); ng += FABS(g[k]); }
        const REAL dp = np_ > eps ? np_ : eps, dg = ng > eps ? ng : eps;
        REAL acc = 0, dot = 0;
        for (int64_t k = 0; k < npix; ++k) {
            const REAL t = LOG(g[k] / dg + eps), q = LOG(p[k] / dp + eps);
            acc += EXP(t) * (t - q);
            dot += (-EXP(t) / (p[k] / dp + eps)) * p[k];
        }
        loss[b] = acc;
        if (grad_pred)
            for (int64_t k = 0; k < npix; ++k) {
                const REAL t = LOG(g[k] / dg + eps);
                const REAL a = -EXP(t) / (p[k] / dp + eps);
                const REAL sgn = p[k] > (REAL)0 ? (REAL)1 : (p[k] < (REAL)0 ? (REAL)-1 : (REAL)0);
                const REAL through_norm = np_ > eps ? sgn * dot / (dp * dp) : (REAL)0;     /* clamp_min passes no gradient */
                grad_pred[b * npix + k] = grad_loss[b] * (a / dp - through_norm);
            }
    }
    return 0;
}

/* ------------------------------------------------------------------------------------------
 * Rigid-body kinematics: artist/field/kinematics_rigid_body.py:194-634 with the ideal and linear actuators
 * (artist/field/actuators_ideal.py, actuators_linear.py), one heliostat at a time.
 * Matrices are row-major 4x4; e, n, u = 0, 1, 2.
 * ---------------------------------------------------------------------------------------- */
typedef struct { REAL m[16]; } FN(mat4);

static FN(mat4) FN(m_eye)(void) { FN(mat4) r; for (int i = 0; i < 16; ++i) r.m[i] = (i % 5 == 0); return r; }
static FN(mat4) FN(m_mul)(const FN(mat4) * a, const FN(mat4) * b)
{
    FN(mat4) r;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            REAL acc = 0;
            for (int k = 0; k < 4; ++k) acc += a->m[4 * i + k] * b->m[4 * k + j];
            r.m[4 * i + j] = acc;
        }
    return r;
}
static FN(mat4) FN(m_rot_e)(REAL x) { FN(mat4) r = FN(m_eye)(); REAL c = COS(x), s_ = SIN(x); r.m[5] = c; r.m[6] = -s_; r.m[9] = s_; r.m[10] = c; return r; }   /* transforms.py:86-128 */
static FN(mat4) FN(m_rot_n)(REAL x) { FN(mat4) r = FN(m_eye)(); REAL c = COS(x), s_ = SIN(x); r.m[0] = c; r.m[2] = -s_; r.m[8] = s_; r.m[10] = c; return r; }   /* :131-170 */
static FN(mat4) FN(m_rot_u)(REAL x) { FN(mat4) r = FN(m_eye)(); REAL c = COS(x), s_ = SIN(x); r.m[0] = c; r.m[1] = -s_; r.m[4] = s_; r.m[5] = c; return r; }    /* :173-212 */
static FN(mat4) FN(m_trans)(REAL e, REAL n, REAL u) { FN(mat4) r = FN(m_eye)(); r.m[3] = e; r.m[7] = n; r.m[11] = u; return r; }                            /* :215-262 */

static inline REAL FN(clampr)(REAL x, REAL lo, REAL hi) { return x < lo ? lo : (x > hi ? hi : x); }
static inline REAL FN(softplus100)(REAL x)   /* F.softplus(x, beta=100), threshold 20: log1p(exp(.)), as ATen has it */
{
    const REAL bx = (REAL)100 * x;
    return bx > (REAL)20 ? x : LOG1P(EXP(bx)) / (REAL)100;
}

/* one actuator column: non-optimisable rows (type, clockwise, min, max[, increment, offset, pivot radius]) and
 * optimisable rows (initial angle, initial stroke length) */
typedef struct { int linear, clockwise; REAL min_pos, max_pos, increment, offset, pivot, init_angle, init_stroke; } FN(act_t);

static FN(act_t) FN(load_act)(const REAL *nonopt, int n_rows, const REAL *opt, int col)
{
    FN(act_t) a;
    a.linear = n_rows >= 7;
    a.clockwise = nonopt[1 * 2 + col] == (REAL)1;
    a.min_pos = nonopt[2 * 2 + col]; a.max_pos = nonopt[3 * 2 + col];
    if (a.linear) {   /* actuators_linear.py:105-178 physics-informed parameters */
        a.increment = FN(softplus100)(nonopt[4 * 2 + col]) + (REAL)1e-6;
        a.offset = FN(softplus100)(nonopt[5 * 2 + col]) + (REAL)1e-6;
        a.pivot = FN(softplus100)(nonopt[6 * 2 + col]) + (REAL)1e-6;
        a.init_angle = opt[0 * 2 + col];
        a.init_stroke = FN(softplus100)(opt[1 * 2 + col]) + (REAL)1e-6;
    } else {
        a.increment = a.offset = a.pivot = a.init_angle = a.init_stroke = 0;
    }
    return a;
}

static REAL FN(act_abs_angle)(const FN(act_t) * a, REAL motor)    /* actuators_linear.py:206-233 */
{
    REAL stroke = motor / a->increment + a->init_stroke;
    stroke = FN(clampr)(stroke, FABS(a->offset - a->pivot) + (REAL)1e-6, a->offset + a->pivot - (REAL)1e-6);
    const REAL num = a->offset * a->offset + a->pivot * a->pivot - stroke * stroke;
    const REAL den = (REAL)2 * a->offset * a->pivot;
    return ACOS(FN(clampr)(num / den, (REAL)-1 + (REAL)1e-6, (REAL)1 - (REAL)1e-6));
}

static REAL FN(act_to_angle)(const FN(act_t) * a, REAL motor)     /* ideal :87 / linear :260-291 */
{
    if (!a->linear) return motor;
    const REAL delta = FN(act_abs_angle)(a, (REAL)0) - FN(act_abs_angle)(a, motor);
    return a->clockwise ? a->init_angle + delta : a->init_angle - delta;
}

static REAL FN(act_to_motor)(const FN(act_t) * a, REAL angle)     /* ideal :111 / linear :319-370 */
{
    if (!a->linear) return angle;
    const REAL delta = a->clockwise ? angle - a->init_angle : a->init_angle - angle;
    const REAL init = FN(act_abs_angle)(a, (REAL)0) - delta;
    const REAL c = FN(clampr)(COS(init), (REAL)-1 + (REAL)1e-6, (REAL)1 - (REAL)1e-6);
    REAL stroke = SQRT(a->offset * a->offset + a->pivot * a->pivot - (REAL)2 * a->offset * a->pivot * c);
    stroke = FN(clampr)(stroke, FABS(a->offset - a->pivot) + (REAL)1e-6, a->offset + a->pivot - (REAL)1e-6);
    return (stroke - a->init_stroke) * a->increment;
}

/* kinematics_rigid_body.py:194-330 */
static FN(mat4) FN(kin_forward)(const REAL *pos, const REAL *rot, const REAL *tr, const FN(act_t) * a1,
                                const FN(act_t) * a2, const REAL *motor)
{
    const REAL th1 = FN(act_to_angle)(a1, motor[0]), th2 = FN(act_to_angle)(a2, motor[1]);
    FN(mat4) t0 = FN(m_trans)(pos[0], pos[1], pos[2]);
    FN(mat4) A = FN(m_rot_n)(rot[0]), B = FN(m_rot_u)(rot[1]), C = FN(m_trans)(tr[0], tr[1], tr[2]), D = FN(m_rot_e)(th1);
    FN(mat4) j1 = FN(m_mul)(&A, &B); j1 = FN(m_mul)(&j1, &C); j1 = FN(m_mul)(&j1, &D);
    FN(mat4) E = FN(m_rot_e)(rot[2]), F = FN(m_rot_n)(rot[3]), G = FN(m_trans)(tr[3], tr[4], tr[5]), Hm = FN(m_rot_u)(th2);
    FN(mat4) j2 = FN(m_mul)(&E, &F); j2 = FN(m_mul)(&j2, &G); j2 = FN(m_mul)(&j2, &Hm);
    FN(mat4) T = FN(m_trans)(tr[6], tr[7], tr[8]);
    FN(mat4) o = FN(m_mul)(&t0, &j1); o = FN(m_mul)(&o, &j2); o = FN(m_mul)(&o, &T);
    return o;
}

/* kinematics_rigid_body.py:331-507: both joint angles from the desired concentrator normal, then motor positions */
static void FN(kin_inverse)(const REAL *rot, const FN(act_t) * a1, const FN(act_t) * a2, const REAL *normal, REAL *motor)
{
    const REAL eps = (REAL)1e-8, PI_ = (REAL)3.14159265358979323846;
    FN(mat4) A = FN(m_rot_n)(rot[0]), B = FN(m_rot_u)(rot[1]);
    FN(mat4) F1 = FN(m_mul)(&A, &B);
    FN(mat4) E = FN(m_rot_e)(rot[2]), Fm = FN(m_rot_n)(rot[3]);
    FN(mat4) F2 = FN(m_mul)(&E, &Fm);
    REAL np[4];
    for (int i = 0; i < 4; ++i) {          /* F1^T n */
        REAL acc = 0;
        for (int k = 0; k < 4; ++k) acc += F1.m[4 * k + i] * normal[k];
        np[i] = acc;
    }
    const REAL f00 = F2.m[0], f01 = F2.m[1];
    const REAL den = SQRT(f00 * f00 + f01 * f01);
    const REAL phi = ATAN2(-f01, f00);
    const REAL ratio = FN(clampr)(np[0] / (den + eps), (REAL)-1 + eps, (REAL)1 - eps);
    REAL s2[2] = {ASIN(ratio) - phi, PI_ - ASIN(ratio) - phi}, s1[2];
    for (int k = 0; k < 2; ++k) {
        s2[k] = ATAN2(SIN(s2[k]), COS(s2[k]));
        FN(mat4) Ru = FN(m_rot_u)(s2[k]);
        FN(mat4) M = FN(m_mul)(&F2, &Ru);
        const REAL vn = -M.m[4 * 1 + 1], vu = -M.m[4 * 2 + 1];       /* M @ (0,-1,0,0) */
        REAL th = ATAN2(vn * np[2] - vu * np[1], vn * np[1] + vu * np[2]);
        s1[k] = ATAN2(SIN(th), COS(th));
    }
    REAL m1[2] = {FN(act_to_motor)(a1, s1[0]), FN(act_to_motor)(a2, s2[0])};
    REAL m2[2] = {FN(act_to_motor)(a1, s1[1]), FN(act_to_motor)(a2, s2[1])};
    const int ok1 = m1[0] >= a1->min_pos && m1[0] <= a1->max_pos && m1[1] >= a2->min_pos && m1[1] <= a2->max_pos;
    motor[0] = ok1 ? m1[0] : m2[0]; motor[1] = ok1 ? m1[1] : m2[1];
}

/* mode 0: motor_positions_to_orientations (:510-538) with the given motor positions;
 * mode 1: incident_ray_directions_to_orientations (:540-634): iterate until NO heliostat's loss moves by more than
 *         min_eps (one stopping decision for the whole batch), at most max_iter times.
 * act_nonopt [H,rows,2], act_opt [H,2,2] (ignored for ideal actuators), offsets [4,4] = initial_orientation_offsets;
 * outputs orientations [H,4,4], motor [H,2] (in/out); returns the number of forward evaluations. */
int FN(orc_rigid_body)(int mode, const REAL *positions, const REAL *rot_dev, const REAL *trans_dev, const REAL *act_nonopt,
                       int64_t act_rows, const REAL *act_opt, const REAL *offsets, const REAL *incident, const REAL *aim,
                       int64_t H, int max_iter, double min_eps, REAL *orientations, REAL *motor)
{
    FN(mat4) off;
    memcpy(off.m, offsets, sizeof(off.m));
    REAL *last = (REAL *)malloc((size_t)(H > 0 ? H : 1) * sizeof(REAL));
    FN(mat4) *ori = (FN(mat4) *)malloc((size_t)(H > 0 ? H : 1) * sizeof(FN(mat4)));
    if (!last || !ori) return -3;
    if (mode == 1) for (int64_t h = 0; h < 2 * H; ++h) motor[h] = 0;
    int evals = 0;
    for (int it = 0; it < (mode == 1 ? max_iter : 1); ++it) {
        int all_converged = it > 0;
        for (int64_t h = 0; h < H; ++h) {
            const REAL *opt = act_opt ? act_opt + 4 * h : NULL;
            FN(act_t) a1 = FN(load_act)(act_nonopt + act_rows * 2 * h, (int)act_rows, opt, 0);
            FN(act_t) a2 = FN(load_act)(act_nonopt + act_rows * 2 * h, (int)act_rows, opt, 1);
            ori[h] = FN(kin_forward)(positions + 4 * h, rot_dev + 4 * h, trans_dev + 9 * h, &a1, &a2, motor + 2 * h);
            if (mode != 1) continue;
            REAL cn[4], co[4], dr[3], dn[4] = {0, 0, 0, 0};
            for (int i = 0; i < 4; ++i) { cn[i] = -ori[h].m[4 * i + 1]; co[i] = ori[h].m[4 * i + 3]; }
            REAL nr = 0;
            for (int k = 0; k < 3; ++k) { dr[k] = aim[4 * h + k] - co[k]; nr += dr[k] * dr[k]; }
            nr = SQRT(nr); if (nr < (REAL)1e-8) nr = (REAL)1e-8;
            REAL nn = 0;
            for (int k = 0; k < 3; ++k) { dn[k] = -incident[4 * h + k] + dr[k] / nr; nn += dn[k] * dn[k]; }
            nn = SQRT(nn); if (nn < (REAL)1e-8) nn = (REAL)1e-8;
            REAL loss = 0;
            for (int k = 0; k < 3; ++k) dn[k] /= nn;
            for (int k = 0; k < 4; ++k) loss += FABS(dn[k] - cn[k]);
            loss /= (REAL)4;
            if (it > 0 && !(FABS(last[h] - loss) <= (REAL)min_eps)) all_converged = 0;
            last[h] = loss;
        }
        ++evals;
        if (mode != 1 || all_converged) break;
        for (int64_t h = 0; h < H; ++h) {        /* motor positions for the next evaluation (:630-632) */
            const REAL *opt = act_opt ? act_opt + 4 * h : NULL;
            FN(act_t) a1 = FN(load_act)(act_nonopt + act_rows * 2 * h, (int)act_rows, opt, 0);
            FN(act_t) a2 = FN(load_act)(act_nonopt + act_rows * 2 * h, (int)act_rows, opt, 1);
            REAL co[4], dr[3], dn[4] = {0, 0, 0, 0};
            for (int i = 0; i < 4; ++i) co[i] = ori[h].m[4 * i + 3];
            REAL nr = 0;
            for (int k = 0; k < 3; ++k) { dr[k] = aim[4 * h + k] - co[k]; nr += dr[k] * dr[k]; }
            nr = SQRT(nr); if (nr < (REAL)1e-8) nr = (REAL)1e-8;
            REAL nn = 0;
            for (int k = 0; k < 3; ++k) { dn[k] = -incident[4 * h + k] + dr[k] / nr; nn += dn[k] * dn[k]; }
            nn = SQRT(nn); if (nn < (REAL)1e-8) nn = (REAL)1e-8;
            for (int k = 0; k < 3; ++k) dn[k] /= nn;
            FN(kin_inverse)(rot_dev + 4 * h, &a1, &a2, dn, motor + 2 * h);
        }
    }
    for (int64_t h = 0; h < H; ++h) {
        FN(mat4) r = FN(m_mul)(&ori[h], &off);
        memcpy(orientations + 16 * h, r.m, sizeof(r.m));
    }
    free(last); free(ori);
    return evals;
}

/* ------------------------------------------------------------------------------------------
 * Fused forward = HeliostatRayTracer.trace_rays (heliostat_ray_tracer.py:285-506, 610-778), one batch holding
 * every heliostat.  Blocking is on when N > 0: prim_* are the tables of ALL blocking primitives, owner[h] the
 * primitive index of heliostat h's own rectangle; flags_out [N] (optional) receives the filtered set.
 *
 *   origins, normals   [H,P,4]    aligned surface points / normals
 *   incident           [H,4]
 *   dist_u, dist_e     element (h,r,p) at base[h*sh + r*sr + p*sp]  (strides in elements)
 *   target_idx         [H] int32 ; centers/pnormals [T,4] ; dims [T,2]
 *   flux               [H,Hh,W]  (zeroed here; row-flipped like :778)
 *   factors            [3,H]     intercept, on_target, blocking   (:498-506)
 *   dbg_*              optional per-stage outputs (NULL to skip): reflected [H,P,4],
 *                      scattered [H,R,P,4], e/u/t/i [H,R,P]
 * OpenMP over heliostats (rows are independent); nthreads<=0 -> runtime default.
 * ---------------------------------------------------------------------------------------- */
int FN(orc_trace_fwd)(const REAL *origins, const REAL *normals, const REAL *incident,
                      const REAL *dist_u, const REAL *dist_e, int64_t sh, int64_t sr, int64_t sp,
                      const int32_t *target_idx, const REAL *centers, const REAL *pnormals, const REAL *dims,
                      const REAL *cyl_centers, const REAL *cyl_normals, const REAL *cyl_axes, const REAL *cyl_radii,
                      const REAL *cyl_heights, const REAL *cyl_opening, int64_t Tc,
                      const REAL *prim_corners, const REAL *prim_spans, const REAL *prim_normals, const int32_t *owner,
                      int64_t N, int lbvh_compat, int32_t *flags_out,
                      double ray_magnitude, double extinction, double reflectivity,
                      int64_t H, int64_t R, int64_t P, int64_t T, int64_t W, int64_t Hh,
                      REAL *flux, REAL *factors, int nthreads,
                      REAL *dbg_reflected, REAL *dbg_scattered, REAL *dbg_e, REAL *dbg_u, REAL *dbg_t, REAL *dbg_i,
                      REAL *dbg_blocked)
{
    const REAL mag = (REAL)ray_magnitude;
    const REAL k_ext = (REAL)(1.0 - extinction);   /* python double folded to tensor dtype (:485) */
    const REAL k_refl = (REAL)reflectivity;        /* (:486) */
    for (int64_t h = 0; h < H; ++h)
        if (target_idx[h] < 0 || target_idx[h] >= T + Tc) return -2;
    int err = 0;
    int32_t *flags = NULL;
    if (N > 0) {
        flags = (int32_t *)malloc((size_t)N * sizeof(int32_t));
        if (!flags) return -3;
        const FN(rayctx_t) ctx = {origins, normals, incident, dist_u, dist_e, sh, sr, sp, mag};
        FN(blocking_flags)(&ctx, target_idx, centers, pnormals, dims, cyl_centers, cyl_normals, cyl_axes, cyl_radii,
                           cyl_heights, cyl_opening, H, R, P, T, W, Hh, prim_corners, owner, N, lbvh_compat, flags);
        if (flags_out) memcpy(flags_out, flags, (size_t)N * sizeof(int32_t));
    }
#ifdef _OPENMP
    if (nthreads <= 0) nthreads = omp_get_max_threads();
#pragma omp parallel for schedule(dynamic, 1) num_threads(nthreads)
#endif
    for (int64_t h = 0; h < H; ++h) {
        REAL *flat = (REAL *)calloc((size_t)(W * Hh), sizeof(REAL));
        if (!flat) { err = -3; continue; }
        /* heliostat_ray_tracer.py:338-346, 425-430: indices below the number of planar areas are planar */
        const int is_cyl = target_idx[h] >= T;
        FN(plane_t) pl;
        FN(cyl_t) cy;
        if (is_cyl) FN(make_cyl)(&cy, cyl_centers, cyl_normals, cyl_axes, cyl_radii, cyl_heights, cyl_opening, target_idx[h] - T, W, Hh);
        else FN(make_plane)(&pl, centers, pnormals, dims, target_idx[h], W, Hh);
        int64_t n_on_target = 0, n_intercept = 0, n_unblocked = 0;
        for (int64_t r = 0; r < R; ++r) {
            for (int64_t p = 0; p < P; ++p) {
                const REAL *o = origins + 4 * (h * P + p);
                REAL d[4], rr[4];
                FN(reflect1)(incident + 4 * h, normals + 4 * (h * P + p), d);
                if (dbg_reflected && r == 0) memcpy(dbg_reflected + 4 * (h * P + p), d, 4 * sizeof(REAL));
                REAL u = dist_u[h * sh + r * sr + p * sp], e = dist_e[h * sh + r * sr + p * sp];
                FN(scatter1)(e, u, d, rr);
                REAL be, bu, t, I;
                if (is_cyl) {
                    REAL rel[3] = {o[0] - cy.c[0], o[1] - cy.c[1], o[2] - cy.c[2]}, ol[3];
                    FN(cyl_rot)(&cy, rel, ol);
                    FN(cylray_t) S;
                    FN(cyl1)(&cy, ol, rr, mag, &be, &bu, &t, &I, &S);
                } else {
                    /* (c - o).m, geometry.py:126-128 */
                    REAL numer = ((pl.c[0] - o[0]) * pl.m[0] + (pl.c[1] - o[1]) * pl.m[1]) + (pl.c[2] - o[2]) * pl.m[2];
                    FN(plane1)(&pl, o, numer, rr, mag, &be, &bu, &t, &I);
                }
                int64_t ray = (h * R + r) * P + p;
                if (dbg_scattered) memcpy(dbg_scattered + 4 * ray, rr, 4 * sizeof(REAL));
                if (dbg_e) dbg_e[ray] = be;
                if (dbg_u) dbg_u[ray] = bu;
                if (dbg_t) dbg_t[ray] = t;
                if (dbg_i) dbg_i[ray] = I;
                REAL blocked = 0;                                  /* :439-443 */
                if (N > 0) {                                       /* :462-480: soft mask over the filtered set */
                    REAL sum = 0;
                    int any = 0;
                    for (int64_t k = 0; k < N; ++k) {
                        if (!flags[k]) continue;
                        FN(soft_t) S;
                        sum += FN(soft1)(prim_corners + 16 * k, prim_spans + 8 * k, prim_spans + 8 * k + 4,
                                         prim_normals + 4 * k, o, rr, &S);
                        any = 1;
                    }
                    if (any) blocked = (REAL)1 - EXP(-(ORC_ALPHA * sum));
                }
                if (dbg_blocked) dbg_blocked[ray] = blocked;
                REAL Iabs = ((I * ((REAL)1 - blocked)) * k_ext) * k_refl;      /* :482-487 */
                n_on_target += (I > (REAL)0);                      /* :498-500 */
                n_unblocked += (blocked < (REAL)1e-3);             /* :501-503 */
                n_intercept += (Iabs > (REAL)0);                   /* :504-506 */
                FN(splat1)(be, bu, Iabs, W, Hh, flat);
            }
        }
        for (int64_t row = 0; row < Hh; ++row)                      /* flip(dim=1), :778 */
            memcpy(flux + (h * Hh + row) * W, flat + (Hh - 1 - row) * W, (size_t)W * sizeof(REAL));
        free(flat);
        /* bool-sum (int64) / python int -> float32 true division (:498-506) */
        REAL denom = (REAL)(R * P);
        factors[0 * H + h] = (REAL)n_intercept / denom;
        factors[1 * H + h] = (REAL)n_on_target / denom;
        factors[2 * H + h] = (REAL)n_unblocked / denom;
    }
    free(flags);
    return err;
}

/* ------------------------------------------------------------------------------------------
 * Backward of the fused forward = what torch.autograd derives for
 * heliostat_ray_tracer.py:285-290, 328-335, 390-433, 482-494, 610-778:
 * indices (.long()), masks (front_facing, valid, on-bitmap, cylinder hit/sector) are constants;
 * gradients flow through the four bilinear weights, the Lambert intensity and the hit point.
 *   grad_flux [H,Hh,W] -> grad_origins [H,P,4], grad_normals [H,P,4]  (w components 0).
 * ---------------------------------------------------------------------------------------- */
int FN(orc_trace_bwd)(const REAL *origins, const REAL *normals, const REAL *incident,
                      const REAL *dist_u, const REAL *dist_e, int64_t sh, int64_t sr, int64_t sp,
                      const int32_t *target_idx, const REAL *centers, const REAL *pnormals, const REAL *dims,
                      const REAL *cyl_centers, const REAL *cyl_normals, const REAL *cyl_axes, const REAL *cyl_radii,
                      const REAL *cyl_heights, const REAL *cyl_opening, int64_t Tc,
                      const REAL *prim_corners, const REAL *prim_spans, const REAL *prim_normals, const int32_t *owner,
                      int64_t N, int lbvh_compat,
                      double ray_magnitude, double extinction, double reflectivity,
                      int64_t H, int64_t R, int64_t P, int64_t T, int64_t W, int64_t Hh,
                      const REAL *grad_flux, REAL *grad_origins, REAL *grad_normals,
                      REAL *grad_prim_corners, REAL *grad_prim_spans, REAL *grad_prim_normals, int nthreads)
{
    const REAL mag = (REAL)ray_magnitude;
    const REAL k_ext = (REAL)(1.0 - extinction);
    const REAL k_refl = (REAL)reflectivity;
    for (int64_t h = 0; h < H; ++h)
        if (target_idx[h] < 0 || target_idx[h] >= T + Tc) return -2;
    int32_t *flags = NULL;
    if (N > 0) {
        flags = (int32_t *)malloc((size_t)N * sizeof(int32_t));
        if (!flags) return -3;
        const FN(rayctx_t) ctx = {origins, normals, incident, dist_u, dist_e, sh, sr, sp, mag};
        FN(blocking_flags)(&ctx, target_idx, centers, pnormals, dims, cyl_centers, cyl_normals, cyl_axes, cyl_radii,
                           cyl_heights, cyl_opening, H, R, P, T, W, Hh, prim_corners, owner, N, lbvh_compat, flags);
        memset(grad_prim_corners, 0, (size_t)(N * 16) * sizeof(REAL));
        memset(grad_prim_spans, 0, (size_t)(N * 8) * sizeof(REAL));
        memset(grad_prim_normals, 0, (size_t)(N * 4) * sizeof(REAL));
    }
#ifdef _OPENMP
    if (nthreads <= 0) nthreads = omp_get_max_threads();
#pragma omp parallel for schedule(dynamic, 1) num_threads(nthreads)
#endif
    for (int64_t h = 0; h < H; ++h) {
        const int is_cyl = target_idx[h] >= T;
        FN(plane_t) pl;
        FN(cyl_t) cy;
        if (is_cyl) FN(make_cyl)(&cy, cyl_centers, cyl_normals, cyl_axes, cyl_radii, cyl_heights, cyl_opening, target_idx[h] - T, W, Hh);
        else FN(make_plane)(&pl, centers, pnormals, dims, target_idx[h], W, Hh);
        const REAL *G = grad_flux + h * Hh * W;
        const REAL *inc = incident + 4 * h;
        for (int64_t p = 0; p < P; ++p) {
            const REAL *o = origins + 4 * (h * P + p);
            const REAL *n = normals + 4 * (h * P + p);
            REAL d[4];
            FN(reflect1)(inc, n, d);
            REAL numer = 0, ol[3] = {0, 0, 0};
            if (is_cyl) {
                REAL rel[3] = {o[0] - cy.c[0], o[1] - cy.c[1], o[2] - cy.c[2]};
                FN(cyl_rot)(&cy, rel, ol);
            } else {
                numer = ((pl.c[0] - o[0]) * pl.m[0] + (pl.c[1] - o[1]) * pl.m[1]) + (pl.c[2] - o[2]) * pl.m[2];
            }
            REAL g_d[3] = {0, 0, 0}, g_o[3] = {0, 0, 0};
            for (int64_t r = 0; r < R; ++r) {
                REAL u = dist_u[h * sh + r * sr + p * sp], e = dist_e[h * sh + r * sr + p * sp];
                REAL ce = COS(e), se = SIN(e), cu = COS(u), su = SIN(u);
                REAL M[3][3] = {{cu, -su, 0}, {ce * su, ce * cu, -se}, {se * su, se * cu, ce}};
                REAL rr[4] = {0, 0, 0, 0};
                for (int k = 0; k < 3; ++k) rr[k] = (M[k][0] * d[0] + M[k][1] * d[1]) + M[k][2] * d[2];
                /* forward of this ray: bitmap coordinates + intensity */
                REAL be, bu, t, I0, a = 0;
                FN(cylray_t) S;
                if (is_cyl) {
                    FN(cyl1)(&cy, ol, rr, mag, &be, &bu, &t, &I0, &S);
                    if (!(S.on && S.hit)) continue;
                } else {
                    FN(plane1)(&pl, o, numer, rr, mag, &be, &bu, &t, &I0);
                    a = (rr[0] * pl.m[0] + rr[1] * pl.m[1]) + rr[2] * pl.m[2];
                    if (!(a < (REAL)0) || (t == (REAL)0 && I0 == (REAL)0 && bu == (REAL)0 && be == pl.wm1)) {
                        /* not front facing, or zeroed by the valid mask: distinguish a genuine (wm1, 0) hit */
                        REAL tt = numer / a, hx = o[0] + rr[0] * tt, hz = o[2] + rr[2] * tt;
                        REAL be0 = (((hx + pl.half_w) - pl.c[0]) / pl.w) * pl.wm1, bu0 = (((hz + pl.half_h) - pl.c[2]) / pl.h) * pl.hm1;
                        if (!(a < (REAL)0) || !(((REAL)0 <= be0) && (be0 <= pl.wm1) && ((REAL)0 <= bu0) && (bu0 <= pl.hm1))) continue;
                    }
                }
                REAL blocked = 0, trans = 1;
                int any_prim = 0;
                if (N > 0) {
                    REAL sum = 0;
                    for (int64_t k = 0; k < N; ++k) {
                        if (!flags[k]) continue;
                        FN(soft_t) Sk;
                        sum += FN(soft1)(prim_corners + 16 * k, prim_spans + 8 * k, prim_spans + 8 * k + 4,
                                         prim_normals + 4 * k, o, rr, &Sk);
                        any_prim = 1;
                    }
                    if (any_prim) { trans = EXP(-(ORC_ALPHA * sum)); blocked = (REAL)1 - trans; }
                }
                REAL I = ((I0 * ((REAL)1 - blocked)) * k_ext) * k_refl;
                int64_t ie = (int64_t)be, iu = (int64_t)bu;
                if (!((0 <= ie) && (ie + 1 < W) && (0 <= iu) && (iu + 1 < Hh))) continue;
                REAL cle = (REAL)(ie + 1) - be, clu = (REAL)(iu + 1) - bu, che = be - (REAL)ie, chu = bu - (REAL)iu;
                /* flat row k corresponds to output row Hh-1-k (flip) */
                REAL g1 = G[(Hh - 1 - (iu + 1)) * W + ie], g2 = G[(Hh - 1 - (iu + 1)) * W + ie + 1];
                REAL g3 = G[(Hh - 1 - iu) * W + ie + 1], g4 = G[(Hh - 1 - iu) * W + ie];
                REAL gIabs = cle * chu * g1 + che * chu * g2 + che * clu * g3 + cle * clu * g4;                     /* dL/dI */
                REAL gI = gIabs * (k_ext * k_refl) * ((REAL)1 - blocked);                                            /* dL/dI0 */
                REAL g_o_soft[3] = {0, 0, 0}, g_r_soft[3] = {0, 0, 0};
                if (any_prim) {
                    /* I = I0 (1 - blocked) k_ext k_refl, blocked = 1 - exp(-alpha sum sigma) */
                    const REAL g_sigma = -gIabs * (k_ext * k_refl) * I0 * ORC_ALPHA * trans;
                    for (int64_t k = 0; k < N; ++k) {
                        if (!flags[k]) continue;
                        const REAL *c0 = prim_corners + 16 * k, *su = prim_spans + 8 * k, *sv = prim_spans + 8 * k + 4,
                                   *pn = prim_normals + 4 * k;
                        FN(soft_t) Sk;
                        (void)FN(soft1)(c0, su, sv, pn, o, rr, &Sk);
                        REAL gc0[3] = {0, 0, 0}, gsu[3] = {0, 0, 0}, gsv[3] = {0, 0, 0}, gpn[3] = {0, 0, 0};
                        FN(soft1_bwd)(c0, su, sv, pn, o, rr, &Sk, g_sigma, g_o_soft, g_r_soft, gc0, gsu, gsv, gpn);
                        for (int c = 0; c < 3; ++c) {
#ifdef _OPENMP
#pragma omp atomic
#endif
                            grad_prim_corners[16 * k + c] += gc0[c];
#ifdef _OPENMP
#pragma omp atomic
#endif
                            grad_prim_spans[8 * k + c] += gsu[c];
#ifdef _OPENMP
#pragma omp atomic
#endif
                            grad_prim_spans[8 * k + 4 + c] += gsv[c];
#ifdef _OPENMP
#pragma omp atomic
#endif
                            grad_prim_normals[4 * k + c] += gpn[c];
                        }
                    }
                }
                REAL g_be = ((chu * g2 + clu * g3) - (chu * g1 + clu * g4)) * I;   /* dL/dche - dL/dcle */
                REAL g_bu = ((cle * g1 + che * g2) - (che * g3 + cle * g4)) * I;   /* dL/dchu - dL/dclu */
                REAL g_r[3];
                if (is_cyl) {
                    REAL g_ol[3];
                    FN(cyl1_bwd)(&cy, ol, mag, &S, g_be, g_bu, gI, g_ol, g_r);
                    for (int k = 0; k < 3; ++k)   /* ol = R (o - c)  ->  g_o = R^T g_ol */
                        g_o[k] += g_ol[0] * cy.R[0][k] + g_ol[1] * cy.R[1][k] + g_ol[2] * cy.R[2][k];
                } else {
                    REAL tt = numer / a;
                    REAL g_hx = (-g_be) * pl.wm1 / pl.w;       /* be = wm1 - te/w*wm1 */
                    REAL g_hz = g_bu * pl.hm1 / pl.h;
                    REAL g_t = g_hx * rr[0] + g_hz * rr[2];
                    g_r[0] = g_hx * tt; g_r[1] = 0; g_r[2] = g_hz * tt;
                    REAL g_a = -mag * gI;                      /* I0 = mag*(-a) */
                    g_a += -g_t * numer / (a * a);             /* t = numer / a */
                    REAL g_numer = g_t / a;
                    for (int k = 0; k < 3; ++k) g_r[k] += g_a * pl.m[k];
                    g_o[0] += g_hx; g_o[2] += g_hz;
                    for (int k = 0; k < 3; ++k) g_o[k] -= g_numer * pl.m[k];
                }
                for (int k = 0; k < 3; ++k) { g_r[k] += g_r_soft[k]; g_o[k] += g_o_soft[k]; }
                for (int k = 0; k < 3; ++k) g_d[k] += M[0][k] * g_r[0] + M[1][k] * g_r[1] + M[2][k] * g_r[2];
            }
            /* d = i - 2 (i.n) n  ->  dL/dn = -2 ( (g_d.n) i + (i.n) g_d ) */
            REAL s = ((inc[0] * n[0] + inc[1] * n[1]) + inc[2] * n[2]) + inc[3] * n[3];
            REAL gdn = g_d[0] * n[0] + g_d[1] * n[1] + g_d[2] * n[2];
            REAL *go = grad_origins + 4 * (h * P + p), *gn = grad_normals + 4 * (h * P + p);
            for (int k = 0; k < 3; ++k) { go[k] = g_o[k]; gn[k] = (REAL)-2 * (gdn * inc[k] + s * g_d[k]); }
            go[3] = 0;
            /* the w component of d is i_w - 2 s n_w; g_d_w = 0 here (scattered w never reaches the flux) */
            gn[3] = (REAL)-2 * (gdn * inc[3]);
        }
    }
    free(flags);
    return 0;
}

/* artist/raytracing/heliostat_ray_tracer.py:593-608 get_bitmaps_per_target():
 * out[t] = sum over heliostats with target_idx == t, in heliostat order. */
int FN(orc_per_target)(const REAL *bitmaps, const int32_t *target_idx, int64_t H, int64_t T, int64_t npix, REAL *out)
{
    memset(out, 0, (size_t)(T * npix) * sizeof(REAL));
    for (int64_t h = 0; h < H; ++h) {
        int64_t t = target_idx[h];
        if (t < 0 || t >= T) return -2;
        for (int64_t k = 0; k < npix; ++k) out[t * npix + k] += bitmaps[h * npix + k];
    }
    return 0;
}

/* ==========================================================================================
 * NURBS surface points + normals.
 * ======================================================================================== */

/* artist/nurbs/surfaces.py:198-207 (uniform) / :209-243 (search).  knots [K], K = n + deg + 1. */
static inline int64_t FN(find_span)(REAL x, const REAL *knots, int64_t n, int deg, int uniform, int64_t n_unique)
{
    if (uniform) return (int64_t)FLOOR(x * (REAL)(n_unique - 1)) + deg;
    /* first span k in [deg, n) with knots[k] <= x < knots[k+1]; argmax of an all-false row is 0 */
    int64_t span = deg;
    for (int64_t k = deg; k < n; ++k)
        if (x >= knots[k] && x < knots[k + 1]) { span = k; break; }
    /* isclose(x, knots[n], atol=1e-5, rtol=1e-5) -> last span (:234-243) */
    REAL last = knots[n];
    if (FABS(x - last) <= (REAL)1e-5 + (REAL)1e-5 * FABS(last)) span = n - 1;
    return span;
}

#define ORC_MAXDEG 7
/* artist/nurbs/surfaces.py:294-417 (The NURBS Book A2.3) for nth_derivative = 1.
 * N[r] = basis values, D[r] = first derivatives, r = 0..deg. */
static inline void FN(basis)(REAL x, const REAL *knots, int64_t span, int deg, REAL *N, REAL *D)
{
    REAL ndu[ORC_MAXDEG + 1][ORC_MAXDEG + 1], left[ORC_MAXDEG + 1], right[ORC_MAXDEG + 1];
    ndu[0][0] = (REAL)1;
    for (int j = 1; j <= deg; ++j) {
        left[j] = x - knots[span + 1 - j];
        right[j] = knots[span + j] - x;
        REAL saved = (REAL)0;
        for (int r = 0; r < j; ++r) {
            ndu[j][r] = right[r + 1] + left[j - r];
            REAL tmp = ndu[r][j - 1] / ndu[j][r];
            ndu[r][j] = saved + right[r + 1] * tmp;
            saved = left[j - r] * tmp;
        }
        ndu[j][j] = saved;
    }
    for (int j = 0; j <= deg; ++j) N[j] = ndu[j][deg];
    for (int r = 0; r <= deg; ++r) {
        /* k = 1 only: a[s1][0] = 1 */
        REAL d = (REAL)0;
        int pk = deg - 1;
        if (r >= 1) {
            REAL a0 = (REAL)1 / ndu[pk + 1][r - 1];
            d = a0 * ndu[r - 1][pk];
        }
        if (r <= pk) {
            REAL a1 = (REAL)-1 / ndu[pk + 1][r];
            d += a1 * ndu[r][pk];
        }
        D[r] = d * (REAL)deg;                       /* :411-415 */
    }
}

static inline REAL FN(norm3)(const REAL *v) { return SQRT((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }

/* artist/geometry/transforms.py:320-340: orthonormal basis from the two canting vectors.
 * B[0]=e, B[1]=n_ortho, B[2]=u (each xyz).  The rotation applied to a row vector `data` is
 * data @ R^T with R's columns e, n_ortho, u  =>  out = e*data_x + n_ortho*data_y + u*data_z. */
static void FN(canting_basis)(const REAL *cant /*[2,4]*/, REAL B[3][3])
{
    REAL e[3] = {cant[0], cant[1], cant[2]}, n[3] = {cant[4], cant[5], cant[6]};
    REAL ne = FN(norm3)(e); if (ne < (REAL)1e-12) ne = (REAL)1e-12;
    for (int k = 0; k < 3; ++k) e[k] = e[k] / ne;
    REAL u[3] = {e[1] * n[2] - e[2] * n[1], e[2] * n[0] - e[0] * n[2], e[0] * n[1] - e[1] * n[0]};
    REAL nu = FN(norm3)(u); if (nu < (REAL)1e-8) nu = (REAL)1e-8;
    for (int k = 0; k < 3; ++k) u[k] = u[k] / nu;
    REAL no[3] = {u[1] * e[2] - u[2] * e[1], u[2] * e[0] - u[0] * e[2], u[0] * e[1] - u[1] * e[0]};
    REAL nn = FN(norm3)(no); if (nn < (REAL)1e-8) nn = (REAL)1e-8;
    for (int k = 0; k < 3; ++k) { no[k] = no[k] / nn; B[0][k] = e[k]; B[1][k] = no[k]; B[2][k] = u[k]; }
}

/* One evaluation: fills S (point, 4 comps incl. weight), Su, Sv (xyz) with the loop order of
 * surfaces.py:592-613, and the span/basis data needed by the backward. */
typedef struct {
    int64_t su, sv;
    REAL Nu[ORC_MAXDEG + 1], Du[ORC_MAXDEG + 1], Nv[ORC_MAXDEG + 1], Dv[ORC_MAXDEG + 1];
    REAL S[4], Su[4], Sv[4];
} FN(eval_t);

static inline void FN(eval1)(const REAL *cp /*[nu,nv,3] of this facet*/, const REAL *ku, const REAL *kv,
                             int64_t nu, int64_t nv, int p, int q, int uniform, int64_t nuq_u, int64_t nuq_v,
                             REAL x, REAL y, FN(eval_t) * E)
{
    E->su = FN(find_span)(x, ku, nu, p, uniform, nuq_u);
    E->sv = FN(find_span)(y, kv, nv, q, uniform, nuq_v);
    /* keep gathers in range (the reference would raise an IndexError instead) */
    if (E->su < p) E->su = p; if (E->su > nu - 1) E->su = nu - 1;
    if (E->sv < q) E->sv = q; if (E->sv > nv - 1) E->sv = nv - 1;
    FN(basis)(x, ku, E->su, p, E->Nu, E->Du);
    FN(basis)(y, kv, E->sv, q, E->Nv, E->Dv);
    for (int k = 0; k <= 1; ++k) {
        const REAL *Bu = k ? E->Du : E->Nu;
        REAL temp[ORC_MAXDEG + 1][4];
        for (int s = 0; s <= q; ++s) {
            for (int c = 0; c < 4; ++c) temp[s][c] = (REAL)0;
            for (int r = 0; r <= p; ++r) {
                const REAL *c3 = cp + ((E->su - p + r) * nv + (E->sv - q + s)) * 3;
                for (int c = 0; c < 3; ++c) temp[s][c] += Bu[r] * c3[c];
                temp[s][3] += Bu[r] * (REAL)1;          /* control-point weight == 1 (:524-537) */
            }
        }
        int dd = 1 - k;                                  /* min(nth_derivative - k, dv), dv = 1 */
        for (int t = 0; t <= dd; ++t) {
            const REAL *Bv = t ? E->Dv : E->Nv;
            REAL *dst = (k == 0 && t == 0) ? E->S : (k == 1 ? E->Su : E->Sv);
            for (int c = 0; c < 4; ++c) dst[c] = (REAL)0;
            for (int s = 0; s <= q; ++s)
                for (int c = 0; c < 4; ++c) dst[c] += Bv[s] * temp[s][c];
        }
    }
}

/* artist/nurbs/surfaces.py:475-689 calculate_surface_points_and_normals().
 *   cp [H,F,nu,nv,3]; uv [H,F,M,2]; knots_u [H,F,nu+p+1]; knots_v [H,F,nv+q+1];
 *   canting [H,F,2,4] or NULL; transl [H,F,4] or NULL (used only when canting != NULL, :674-687)
 *   n_unique_u/v: number of distinct knot values (torch.unique, :199) for the uniform formula
 *   -> points, normals [H,F,M,4]. */
int FN(orc_nurbs_fwd)(const REAL *cp, const REAL *uv, const REAL *knots_u, const REAL *knots_v,
                      const REAL *canting, const REAL *transl, int p, int q, int uniform,
                      int64_t n_unique_u, int64_t n_unique_v,
                      int64_t H, int64_t F, int64_t M, int64_t nu, int64_t nv, REAL *points, REAL *normals)
{
    if (p < 1 || q < 1 || p > ORC_MAXDEG || q > ORC_MAXDEG || nu <= p || nv <= q) return -1;
    for (int64_t hf = 0; hf < H * F; ++hf) {
        const REAL *cpf = cp + hf * nu * nv * 3;
        const REAL *ku = knots_u + hf * (nu + p + 1), *kv = knots_v + hf * (nv + q + 1);
        REAL B[3][3];
        if (canting) FN(canting_basis)(canting + hf * 8, B);
        for (int64_t m = 0; m < M; ++m) {
            FN(eval_t) E;
            FN(eval1)(cpf, ku, kv, nu, nv, p, q, uniform, n_unique_u, n_unique_v,
                      uv[(hf * M + m) * 2], uv[(hf * M + m) * 2 + 1], &E);
            /* :615-632 cross(dS/du, dS/dv) */
            REAL c[3] = {E.Su[1] * E.Sv[2] - E.Su[2] * E.Sv[1], E.Su[2] * E.Sv[0] - E.Su[0] * E.Sv[2],
                         E.Su[0] * E.Sv[1] - E.Su[1] * E.Sv[0]};
            REAL pt[4] = {E.S[0] / E.S[3], E.S[1] / E.S[3], E.S[2] / E.S[3], (REAL)1};   /* :642-657 */
            REAL nc = FN(norm3)(c); if (nc < (REAL)1e-12) nc = (REAL)1e-12;               /* :659-661 */
            REAL nr[4] = {c[0] / nc, c[1] / nc, c[2] / nc, (REAL)0};
            REAL *po = points + (hf * M + m) * 4, *no = normals + (hf * M + m) * 4;
            if (canting) {
                /* data @ R^T, 4-term sequential dot with R[j][3] = 0 for j<3, R[3] = (0,0,0,1) (:334-347) */
                for (int j = 0; j < 3; ++j) {
                    po[j] = (((pt[0] * B[0][j] + pt[1] * B[1][j]) + pt[2] * B[2][j]) + pt[3] * (REAL)0)
                            + transl[hf * 4 + j];                                           /* :678-683 */
                    no[j] = ((nr[0] * B[0][j] + nr[1] * B[1][j]) + nr[2] * B[2][j]) + nr[3] * (REAL)0;
                }
                po[3] = (REAL)1 + transl[hf * 4 + 3];
                no[3] = (REAL)0;
            } else {
                memcpy(po, pt, 4 * sizeof(REAL));
                memcpy(no, nr, 4 * sizeof(REAL));
            }
        }
    }
    return 0;
}

/* Backward of orc_nurbs_fwd w.r.t. the control points (what autograd derives for
 * surfaces.py:578-689 + transforms.py:320-347; spans, knots and evaluation points constant).
 *   g_points, g_normals [H,F,M,4] -> g_cp [H,F,nu,nv,3] (zeroed here). */
int FN(orc_nurbs_bwd)(const REAL *cp, const REAL *uv, const REAL *knots_u, const REAL *knots_v,
                      const REAL *canting, int p, int q, int uniform, int64_t n_unique_u, int64_t n_unique_v,
                      int64_t H, int64_t F, int64_t M, int64_t nu, int64_t nv,
                      const REAL *g_points, const REAL *g_normals, REAL *g_cp)
{
    if (p < 1 || q < 1 || p > ORC_MAXDEG || q > ORC_MAXDEG || nu <= p || nv <= q) return -1;
    memset(g_cp, 0, (size_t)(H * F * nu * nv * 3) * sizeof(REAL));
    for (int64_t hf = 0; hf < H * F; ++hf) {
        const REAL *cpf = cp + hf * nu * nv * 3;
        REAL *gcf = g_cp + hf * nu * nv * 3;
        const REAL *ku = knots_u + hf * (nu + p + 1), *kv = knots_v + hf * (nv + q + 1);
        REAL B[3][3];
        if (canting) FN(canting_basis)(canting + hf * 8, B);
        for (int64_t m = 0; m < M; ++m) {
            FN(eval_t) E;
            FN(eval1)(cpf, ku, kv, nu, nv, p, q, uniform, n_unique_u, n_unique_v,
                      uv[(hf * M + m) * 2], uv[(hf * M + m) * 2 + 1], &E);
            const REAL *gp = g_points + (hf * M + m) * 4, *gn = g_normals + (hf * M + m) * 4;
            REAL gpt[3], gnr[3];
            if (canting) {   /* out_j = sum_k data_k B[k][j]  ->  g_data_k = sum_j g_out_j B[k][j] */
                for (int k = 0; k < 3; ++k) {
                    gpt[k] = gp[0] * B[k][0] + gp[1] * B[k][1] + gp[2] * B[k][2];
                    gnr[k] = gn[0] * B[k][0] + gn[1] * B[k][1] + gn[2] * B[k][2];
                }
            } else {
                for (int k = 0; k < 3; ++k) { gpt[k] = gp[k]; gnr[k] = gn[k]; }
            }
            REAL c[3] = {E.Su[1] * E.Sv[2] - E.Su[2] * E.Sv[1], E.Su[2] * E.Sv[0] - E.Su[0] * E.Sv[2],
                         E.Su[0] * E.Sv[1] - E.Su[1] * E.Sv[0]};
            REAL nc = FN(norm3)(c);
            REAL gc[3];
            if (nc < (REAL)1e-12) {   /* clamp_min branch: n = c / eps */
                for (int k = 0; k < 3; ++k) gc[k] = gnr[k] / (REAL)1e-12;
            } else {
                REAL nr[3] = {c[0] / nc, c[1] / nc, c[2] / nc};
                REAL dot = nr[0] * gnr[0] + nr[1] * gnr[1] + nr[2] * gnr[2];
                for (int k = 0; k < 3; ++k) gc[k] = (gnr[k] - nr[k] * dot) / nc;
            }
            /* c = Su x Sv : gSu = Sv x gc ; gSv = gc x Su */
            REAL gSu[3] = {E.Sv[1] * gc[2] - E.Sv[2] * gc[1], E.Sv[2] * gc[0] - E.Sv[0] * gc[2],
                           E.Sv[0] * gc[1] - E.Sv[1] * gc[0]};
            REAL gSv[3] = {gc[1] * E.Su[2] - gc[2] * E.Su[1], gc[2] * E.Su[0] - gc[0] * E.Su[2],
                           gc[0] * E.Su[1] - gc[1] * E.Su[0]};
            REAL gS[3] = {gpt[0] / E.S[3], gpt[1] / E.S[3], gpt[2] / E.S[3]};
            for (int r = 0; r <= p; ++r)
                for (int s = 0; s <= q; ++s) {
                    REAL w00 = E.Nu[r] * E.Nv[s], w10 = E.Du[r] * E.Nv[s], w01 = E.Nu[r] * E.Dv[s];
                    REAL *g3 = gcf + ((E.su - p + r) * nv + (E.sv - q + s)) * 3;
                    for (int k = 0; k < 3; ++k) g3[k] += w00 * gS[k] + w10 * gSu[k] + w01 * gSv[k];
                }
        }
    }
    return 0;
}

/* artist/raytracing/sampling.py:129-146 RestrictedDistributedSampler.rank_indices.
 * Writes at most cap indices; returns the count (or -1 if cap is too small). */
#ifndef ORC_SAMPLER_DEFINED
#define ORC_SAMPLER_DEFINED
int64_t orc_sampler_indices(int64_t n_samples, int64_t n_active_heliostats, int64_t world, int64_t rank,
                            int64_t *out, int64_t cap)
{
    int64_t active_ranks = n_active_heliostats < world ? n_active_heliostats : world;
    int64_t cnt = 0;
    if (rank >= active_ranks) return 0;
    int64_t per = n_samples / n_active_heliostats;
    for (int64_t i = 0; i < n_active_heliostats; ++i)
        if (i % active_ranks == rank)
            for (int64_t k = i * per; k < i * per + per; ++k) {
                if (cnt >= cap) return -1;
                out[cnt++] = k;
            }
    return cnt;
}
#endif

#undef FN
#undef CAT
#undef CAT_
