/*
 * artist_hip_regularizers.h - the surface regularisers of libartist_hip.so (same library, same conventions and return codes
 * as include/artist_hip.h: device pointers, `stream` is a hipStream_t passed as void*, asynchronous).
 */
#ifndef ARTIST_HIP_REGULARIZERS_H
#define ARTIST_HIP_REGULARIZERS_H

#include <stdint.h>

#include "artist_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * art_surface_regularizers_fwd - SmoothnessRegularizer and IdealSurfaceRegularizer before their reduction over
 *   `reduction_dimensions` (artist/optim/regularizers.py:83-131 and :154-186), both in ONE launch.  For every net n of
 *   the contiguous fp32 batch current, original [N,U,V,3], with d = current - original:
 *     smoothness[n] = mean over (u, v, c) of lap^2,  lap = (((4 d - d[u-1]) - d[u+1]) - d[v-1]) - d[v+1]
 *                     (neighbour indices clamped to the net: the reference's replicate padding; lap is its fp32 value
 *                      bit for bit, only the order of the final sum differs);
 *     ideal[n]      = mean of d^2.
 *   Either output [N] may be null (that term is not computed), not both.
 *
 * art_surface_regularizers_bwd - their autograd w.r.t. current (what torch derives for the lines above):
 *     grad_current = grad_ideal[n] * 2 d / m + grad_smoothness[n] * (2 / m) * L^T(lap),  m = U*V*3,
 *   L^T the adjoint of the clamped stencil.  grad_smoothness / grad_ideal [N] may each be null (the term is dropped; both
 *   null writes zeros).  grad_current [N,U,V,3] is fully written; the gradient w.r.t. original is its negative.
 *
 *   Both: a net's bits depend on that net alone (one wave per net, fixed-order sums, no atomics), so rows of a larger call
 *   equal the same nets called alone.  A net is staged in LDS: U*V*3 <= 8192.  ART_EINVAL for negative N, U or V < 1,
 *   larger nets, or null pointers when N > 0; N == 0 launches nothing.
 * ------------------------------------------------------------------------------------------- */
int art_surface_regularizers_fwd(const float *current, const float *original, int64_t N, int64_t U, int64_t V,
                                 float *smoothness, float *ideal, void *stream);
int art_surface_regularizers_bwd(const float *current, const float *original, int64_t N, int64_t U, int64_t V,
                                 const float *grad_smoothness, const float *grad_ideal, float *grad_current, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ARTIST_HIP_REGULARIZERS_H */
