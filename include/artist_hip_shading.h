/*
 * artist_hip_shading.h - heliostat shading as blocking by per-heliostat sheared rectangles, in libartist_hip.so (same library,
 * same conventions and return codes as include/artist_hip.h: device pointers, contiguous fp32 / int32, `stream` is a
 * hipStream_t passed as void*, asynchronous, no allocation).
 */
#ifndef ARTIST_HIP_SHADING_H
#define ARTIST_HIP_SHADING_H

#include <stdint.h>

#include "artist_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * Common: prim_corners [N,4,4] the rectangles of create_blocking_primitives_rectangles_by_index (corner order 0, 1, 2, 3;
 *   spans = corner 1 - corner 0, corner 3 - corner 0), owner [H] the rectangle of each traced heliostat, incident [H,4] the
 *   unit direction of the sun's rays (a constant: no gradient), S >= 1 slots per heliostat.  For heliostat h with
 *   c = corner 0 + (su + sv)/2 and n = normalize(su x sv) of its own rectangle, s = -incident[h], the shear
 *   A_h(x) = x - 2 ((x - c).n)/(s.n) (s - (s.n) n) maps the sunward ray of a plane point onto its reflected ray at the same
 *   parameter, so that rectangle j shades h exactly where the parallelogram A_h(j) blocks it.
 *   ART_EINVAL for negative sizes, S < 1 or S > 4096, H, N or H*S beyond 2^22, or a null pointer with work to do; H == 0
 *   launches nothing.
 *
 * art_shading_cull - which rectangles can shade which heliostat.  shader_idx [H,S] int32: the rectangles j != owner[h] that
 *   pass the rule stated at the top of artist_amd/csrc/shading_kernels.hip (a conservative test of centres and bounding radii:
 *   the component along s, the distance from the sun line through c, the side of h's plane; a superset of every rectangle
 *   whose soft-mask term can reach 1e-11), ascending, the first S of them, -1 in the empty slots; shade_count [H] the number
 *   FOUND, which may exceed S.  |s.n| < 1e-3 or an owner outside [0, N): no shaders.  One workgroup per heliostat, ordered
 *   compaction: the lists do not depend on the launch.  max_scatter_angle >= 0: the largest |distortion angle| of the trace.
 *
 * art_shading_prims_fwd - the tables of the virtual parallelograms, H*S rows: shade_corners [H*S,4,4] = A_h of the four
 *   corners of shader_idx[h][k] (w copied), shade_spans [H*S,2,4] = sheared corner 1 - corner 0, corner 3 - corner 0,
 *   shade_normals [H*S,4] = normalize(span_u x span_v) (w = 0).  Rows of empty slots are zeros; nothing refers to them.
 *   The three outputs are 16-byte aligned.
 *
 * art_shading_prims_bwd - the adjoint: grad_shade_* are the gradients w.r.t. the three tables (what art_trace_bwd leaves in
 *   the rows N ... N + H*S - 1 of its rectangle gradients), grad_prim_corners [N,4,4] receives the gradient w.r.t. the real
 *   corners through both paths - the shader's corners and the corners of h's own rectangle (c and n).  scratch: H*S*24
 *   floats.  Every row of grad_prim_corners is written (w = 0); per rectangle the slots are added in slot order by thread and
 *   the threads by a fixed tree: no float atomics, the same bits in every run.  H == 0 zero-fills; N == 0 does nothing.
 *   Each of the N workgroups scans all H*S slot indices: N*H*S index reads, 32 M at 2000 heliostats of one field - sized for
 *   fields, and quadratic well before the 2^22 the size checks admit.
 *
 * art_shading_append - after art_blocking_filter (or on zeroed counts when blocking is off): the indices N + h*S + k of the
 *   filled slots of heliostat h are appended to row h of cand [H,Cmax] and cand_count[h] grows by their number.  They are
 *   larger than every real index, so the row stays ascending, and they enter the row of their own heliostat only.  If the
 *   row has no room for them, or shade_count[h] > S, cand_count[h] = Cmax + 1 and the rest of the row is filled with a valid
 *   index: art_trace_fwd then writes NaN into that heliostat's bitmap and factors, as for a row the filter overflowed.  A row
 *   the filter overflowed (cand_count[h] > Cmax on entry) is left as it is.
 * ------------------------------------------------------------------------------------------- */
int art_shading_cull(const float *prim_corners, const int32_t *owner, const float *incident, int64_t H, int64_t N,
                     double max_scatter_angle, int64_t S, int32_t *shader_idx, int32_t *shade_count, void *stream);
int art_shading_prims_fwd(const float *prim_corners, const int32_t *owner, const float *incident, const int32_t *shader_idx,
                          int64_t H, int64_t N, int64_t S, float *shade_corners, float *shade_spans, float *shade_normals,
                          void *stream);
int art_shading_prims_bwd(const float *prim_corners, const int32_t *owner, const float *incident, const int32_t *shader_idx,
                          const float *grad_shade_corners, const float *grad_shade_spans, const float *grad_shade_normals,
                          int64_t H, int64_t N, int64_t S, float *scratch, float *grad_prim_corners, void *stream);
int art_shading_append(const int32_t *shader_idx, const int32_t *shade_count, int64_t H, int64_t N, int64_t S, int64_t Cmax,
                       int32_t *cand, int32_t *cand_count, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ARTIST_HIP_SHADING_H */
