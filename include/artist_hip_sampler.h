/*
 * artist_hip_sampler.h - the sun-shape distortion samplers of libartist_hip.so, Gaussian and radially symmetric (same
 * library, same conventions and return codes as include/artist_hip.h: device pointers, `stream` is a hipStream_t passed as
 * void*, asynchronous).
 */
#ifndef ARTIST_HIP_SAMPLER_H
#define ARTIST_HIP_SAMPLER_H

#include <stdint.h>

#include "artist_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * art_sample_distortions - Sun.get_distortions on the device (artist/scene/sun.py:199-234): rows `rows` of the
 *   [H,R,P] Gaussian sun-shape sample, written as one interleaved buffer out[k,r,p,0:2] = (u, e) of heliostat
 *   row rows[k] (fp32, contiguous [n_rows,R,P,2]; Sun.get_distortions_rows returns its stride-2 views).
 *
 *   Stream: Philox4x32-10 (Random123), key = (seed_lo, seed_hi) = the seed as a 64-bit two's-complement value,
 *   counter = (j_lo, j_hi, row_lo, row_hi) with j the pair index inside the row: one call serves rays 2j and
 *   2j+1 (ray index r*P + p; if R*P is odd the last call writes ray 2j only).  Box-Muller on (x0, x1) for ray 2j
 *   and on (x2, x3) for ray 2j+1: a = x_even * 2^-32 + 2^-33 (fp32, in (0, 1]), b = x_odd * 2^-32,
 *   z0 = sqrt(-2 ln a) cos 2 pi b, z1 = sqrt(-2 ln a) sin 2 pi b.  Law (loc + scale_tril @ z, as
 *   MultivariateNormal.sample): u = loc_u + l00 z0, e = loc_e + (l10 z0 + l11 z1).
 *
 *   The bits of a row depend on (seed, row, R, P, law) only: not on the launch, the order of `rows` or the other
 *   rows of the call, so a rank that draws the rows it owns gets exactly those rows of an unsharded draw.
 *   The law comes in as host scalars: nothing is read back from the device, and no state is kept.
 *
 *   rows  [n_rows] int64 (device), any values;  out [n_rows,R,P,2] fp32 (device, 8-byte aligned).
 *   ART_EINVAL for negative sizes, or null pointers when n_rows*R*P > 0; n_rows*R*P == 0 launches nothing.
 */
int art_sample_distortions(int64_t seed, const int64_t *rows, int64_t n_rows, int64_t R, int64_t P,
                           float loc_u, float loc_e, float l00, float l10, float l11,
                           float *out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * art_sample_radial_distortions - the same sample for a radially symmetric sun shape (pillbox, Buie, a measured
 *   profile: artist_amd.scene.Sun) given as a quantile table of squared radii.
 *
 *   table [K+1] fp32 (device), non-decreasing: table[k] is the squared angular radius (rad^2) below which the
 *   fraction k/K of the energy lies; between two nodes theta^2 is linear in the quantile, which is K annuli of
 *   equal energy with constant radiance inside each.  A uniform disc is exact with K = 1, table = {0, theta_max^2}.
 *
 *   Stream, counter layout, key, ray order, odd tail, output layout, the float4 / float2 store paths and the
 *   argument checks are those of art_sample_distortions (above).  Per ray, from the same 32-bit pair (x_even, x_odd):
 *   q = x_even * 2^-32 + 2^-33 (fp32, in (0, 1]), b = x_odd * 2^-32, t = q * K, i = min((int)t, K-1), f = t - i,
 *   theta = sqrt(table[i] + f * (table[i+1] - table[i])) (fp32, the product and the sum rounded separately),
 *   u = loc_u + theta cos 2 pi b, e = loc_e + theta sin 2 pi b: the radius has the table's law, the azimuth is
 *   uniform, and (u, e) are read as small angles like the Gaussian's (relative error O(theta^2)).
 *
 *   Every workgroup copies the table into LDS once, as K pairs (table[i], table[i+1] - table[i]) of 8 bytes (32 KiB
 *   at K = 4096), before its first lookup; the lookup is one 8-byte LDS read.  The bits of a row depend on
 *   (seed, row, R, P, loc, table) only: not on the launch, the order of `rows` or the other rows of the call.
 *   loc comes in as host scalars, the table stays on the device: nothing is read back, and no state is kept.
 *
 *   rows  [n_rows] int64 (device), any values;  out [n_rows,R,P,2] fp32 (device, 8-byte aligned).
 *   ART_EINVAL for negative sizes, for K < 1 or K > 4096 (whatever the other sizes), or for null pointers (rows,
 *   table, out) when n_rows*R*P > 0; n_rows*R*P == 0 launches nothing.
 */
int art_sample_radial_distortions(int64_t seed, const int64_t *rows, int64_t n_rows, int64_t R, int64_t P,
                                  float loc_u, float loc_e, const float *table, int64_t K,
                                  float *out, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ARTIST_HIP_SAMPLER_H */
