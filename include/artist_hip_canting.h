/*
 * artist_hip_canting.h - the facet canting rotation on its own, with its gradients, in libartist_hip.so (same library, same
 * conventions and return codes as include/artist_hip.h: device pointers, contiguous fp32, `stream` is a hipStream_t passed
 * as void*, asynchronous).
 */
#ifndef ARTIST_HIP_CANTING_H
#define ARTIST_HIP_CANTING_H

#include <stdint.h>

#include "artist_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * Both entry points: HF facets, M points per facet.  canting [HF,2,4] holds the facet's e and n vectors; the basis
 *   B = (e^, n_ortho, u) is built as artist/geometry/transforms.py:320-340 does: e^ = e / max(|e|, 1e-12),
 *   u = e^ x n / max(|.|, 1e-8), n_ortho = u x e^ / max(|.|, 1e-8), B[k][j] = component j of basis vector k.
 *   data_points / data_normals [HF,M,4] are two independent arrays of homogeneous row vectors; either may be null (that
 *   array is not processed), not both.
 *
 * art_cant_facets_fwd - artist/geometry/transforms.py:276-347 (perform_canting) and the facet translation of
 *   artist/nurbs/surfaces.py:674-687.
 *     inverse == 0:  out_j = ((x B[0][j] + y B[1][j]) + z B[2][j]) + w 0  (j = 0..2),  out_w = w      (data @ R^T)
 *                    points additionally + translations[hf] on all four components when translations [HF,4] is not null;
 *                    normals never (their rotation is the three products alone).
 *     inverse != 0:  out_k = ((x B[k][0] + y B[k][1]) + z B[k][2]) + w 0,  out_w = w                   (data @ R)
 *                    translations must be null.
 *   The products and sums are rounded one by one in this order: given the points and normals that art_nurbs_fwd writes
 *   with canting = NULL, the outputs equal those of art_nurbs_fwd with the canting and translations bit for bit.
 *   ART_EINVAL for negative sizes, sizes beyond 2^31 - 1, translations with inverse, or - when HF*M > 0 - a null
 *   canting, both data arrays null, translations without data_points, or a data array without its output; HF*M == 0
 *   launches nothing (and looks at no pointer: an empty array may have none).
 *
 * art_cant_facets_bwd - what autograd derives for the lines above (transforms.py:276-347, surfaces.py:674-687), in one
 *   launch.  grad_out_points / grad_out_normals [HF,M,4] are the gradients w.r.t. the two outputs (null: zero).
 *   Every output is optional (null: not computed), at least one is required:
 *     grad_data_points / grad_data_normals [HF,M,4]  g @ B (inverse: g @ B^T) on x, y, z and g_w on w;
 *                                                    needs the matching grad_out array.
 *     grad_canting [HF,2,4]      dL/dB[k][j] = sum over the facet's points AND normals of data_k g_j (inverse: g_k data_j),
 *                                chained through the adjoint of the basis (three normalisations with their clamps - a
 *                                clamped norm passes no gradient, as clamp_min does - and two cross products); the two w
 *                                components are 0.  Needs canting and, for every grad_out array given, its data array.
 *     grad_translations [HF,4]   sum over the facet's points of grad_out_points, all four components; inverse must be 0.
 *   One workgroup per facet; partial sums in fp64 registers, combined by a fixed shuffle tree inside a wave and in wave
 *   order across waves, the basis adjoint in fp64 by one thread: no atomics, and a facet's bits depend on that facet alone
 *   - not on HF, its position in the batch or the run.  grad_canting and grad_translations are written in full.
 *   ART_EINVAL for negative sizes, sizes beyond 2^31 - 1, no output at all, grad_translations with inverse, or - when
 *   HF*M > 0 - a null pointer that a requested output needs; HF*M == 0 launches no kernel but still zero-fills
 *   grad_canting / grad_translations when HF > 0.
 * ------------------------------------------------------------------------------------------- */
int art_cant_facets_fwd(const float *canting, const float *translations, const float *data_points, const float *data_normals,
                        int inverse, int64_t HF, int64_t M, float *out_points, float *out_normals, void *stream);
int art_cant_facets_bwd(const float *canting, const float *data_points, const float *data_normals,
                        const float *grad_out_points, const float *grad_out_normals, int inverse, int64_t HF, int64_t M,
                        float *grad_data_points, float *grad_data_normals, float *grad_canting, float *grad_translations,
                        void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ARTIST_HIP_CANTING_H */
