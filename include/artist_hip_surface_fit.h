/*
 * artist_hip_surface_fit.h - batched NURBS surface fitting of libartist_hip.so: SurfaceGenerator.fit_nurbs
 * (artist/scenario/surface_generator.py:71-223) for B independent facets at once.  Same library, conventions and return
 * codes as include/artist_hip.h: fp32 device pointers, `stream` is a hipStream_t passed as void*, asynchronous, arguments
 * checked before the first launch.
 *
 * Sizes: B facets, N rows of measured data per facet of which the first n_valid[b] count, a control net nu x nv of degrees
 * p, q (1..7, nu > p, nv > q) on clamped uniform knots.  ncells = (nu - p) * (nv - q) knot-span cells.
 * Limits: 1 <= N <= 1048576 (2^20; more is ART_EINVAL, never narrowed), ncells <= 4096.  The number of points is otherwise
 * no limit.  ART_EUNSUPPORTED is left for one case: the block of LDS that a workgroup keeps whatever N is - net, two Adam
 * moments, cell partial sums, cell offsets, the launch's bias-correction tables: 3 epochs + 9 nu nv + 3 ncells (p+1)(q+1) +
 * ncells + 3 floats - does not fit in 160 KiB beside 64 points.  Nothing falls back silently.
 * LDS: when a facet's per-point arrays (gradient and squared error of every point: 7 N floats) fit beside that block - for a
 * 10 x 10 degree-3 net and a 401-epoch launch up to N = 5207 - they stay resident for the whole launch, and the per-point
 * tables are staged in LDS as well when they fit too (streamed from `table` otherwise).  Beyond that the points are taken in
 * chunks of C sorted positions, C a multiple of 64 sized from what the block leaves (5184 in that example), table and
 * targets streamed; prepare likewise sorts in tiles of 16384 rows when 2 N ints do not fit (or N > 16384).  Every sum keeps
 * the owner and the order described below in every case - the running sum of a cell's control point and a lane's share of
 * the loss are carried from chunk to chunk - so all of these paths give the same bits.
 *
 * Determinism: no float atomics anywhere.  Points are grouped by span cell; a cell's (p+1)(q+1) control points receive the
 * cell's points in index order, a control point then adds its at most (p+1)(q+1) cell sums in cell order, and the loss adds
 * the points in sorted order with lane l of one wave owning positions l, l + 64, ... in fp64 followed by a fixed shuffle tree.
 * A facet's bits depend on that facet's data alone: not on B, not on the padded row count N of its batch, not on the
 * neighbours, not on how epochs are chunked into launches - although N and the epochs of a launch decide whether a facet is
 * resident or taken in chunks, and how long a chunk is.
 */
#ifndef ARTIST_HIP_SURFACE_FIT_H
#define ARTIST_HIP_SURFACE_FIT_H

#include <stdint.h>

#include "artist_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ART_FIT_POINTS 0  /* loss = MSE(surface points,  targets_points)  over all N*4 components */
#define ART_FIT_NORMALS 1 /* loss = MSE(surface normals, targets_normals) over all N*4 components */

/* Floats per point of `table` for degrees (p, q): W = 3 + 4 (D + 1), D = p when p == q and a compile-time instantiation exists
 * (2, 3), else 7 (degree 3: 19).  Negative for degrees out of range.  Size the buffer with this function. */
int64_t art_surface_fit_table_words(int p, int q);

/* ---------------------------------------------------------------------------------------------
 * art_surface_fit_prepare - what fit_nurbs does before its loop (surface_generator.py:133-180, coordinates.normalize_points),
 *   one workgroup per facet:
 *     eval_uv [B,N,2]           (x - min + 1e-5) / (max(x - min) + 2e-5) of the e and n columns of targets_points over the valid
 *                               rows, in the reference's operation order (bit-equal to it); rows beyond n_valid are zero;
 *     control_points [B,nu,nv,3] linspace(-w/2, w/2, nu) x linspace(-h/2, h/2, nv), z = 0 (torch.linspace's fp32 values);
 *     perm [B,N] int32          the valid rows ordered by span cell (u-major), by row index inside a cell; -1 beyond n_valid;
 *     cell_start [B,ncells+1] int32  offsets of the cells in that order;
 *     table [B,N,W]             per sorted point: [spans (su | sv << 16, as int bits), sum_r Nu[r], Nu[D+1], Du[D+1], Nv[D+1],
 *                               Dv[D+1], cell (int bits)] - knot spans, A2.3 basis values and first derivatives, and the
 *                               point's cell; W = art_surface_fit_table_words(p, q) = 3 + 4 (D + 1).
 *   knots_u [nu+p+1], knots_v [nv+q+1]: the clamped uniform knot vectors (shared by all facets), the ones art_nurbs_fwd is given.
 *   n_valid [B] int32 may be null (all N rows count); values are clamped to [0, N].  A facet WITHOUT valid rows is not an
 *   error: its initial net is all zeros, its loss is NaN, loss_grad gives a zero gradient, and run gives it exactly one epoch
 *   (last_loss starts at +inf) whose NaN loss stops it: epochs_run = 1, done = 1, the net still zeros.
 *   loss_grad and run are meant to be given the n_valid that prepare was given; a larger value is cut to the number of rows
 *   prepare sorted (positions beyond those have no row).
 * ------------------------------------------------------------------------------------------- */
int art_surface_fit_prepare(const float *targets_points, const int32_t *n_valid, const float *knots_u, const float *knots_v,
                            int64_t B, int64_t N, int64_t nu, int64_t nv, int p, int q, float *eval_uv,
                            float *control_points, int32_t *perm, int32_t *cell_start, float *table, void *stream);

/* ---------------------------------------------------------------------------------------------
 * art_surface_fit_loss_grad - one epoch's forward and backward without an update, one launch:
 *     loss [B]                  torch.nn.MSELoss (mean over the n_valid * 4 components, w column included) of the surface
 *                               points (w = 1) or unit normals (w = 0) at the facet's points against `targets` [B,N,4]
 *                               (the points or the normals, by `method`);
 *     grad_control_points [B,nu,nv,3]  d loss / d control_points.
 *   points_out, normals_out [B,N,4] may be null; when given they receive the evaluated points / normals in the original row
 *   order (rows beyond n_valid untouched) - bit-equal to art_nurbs_fwd on the same net and eval_uv.
 *   perm, cell_start, table: as written by art_surface_fit_prepare for the same B, N, nu, nv, p, q.
 * ------------------------------------------------------------------------------------------- */
int art_surface_fit_loss_grad(const float *control_points, const float *targets, const int32_t *n_valid, const int32_t *perm,
                              const int32_t *cell_start, const float *table, int64_t B, int64_t N, int64_t nu, int64_t nv,
                              int p, int q, int method, float *loss, float *grad_control_points, float *points_out,
                              float *normals_out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * art_surface_fit_run - up to `epochs` (1..1024) epochs of evaluate -> loss -> gradient -> Adam -> plateau scheduler -> stop
 *   test in ONE launch, one workgroup per facet, no host involvement.  Per-facet state, read at the start and written back
 *   at the end (so 400 epochs in one launch and 4 x 100 give the same bits):
 *     control_points, exp_avg, exp_avg_sq [B,nu,nv,3]   (kept in LDS during the launch)
 *     state_f64 [B,2]   lr, scheduler best
 *     state_i32 [B,5]   Adam step, scheduler num_bad_epochs, scheduler cooldown_counter, epochs_run, done
 *     last_loss [B]     the loss computed by the last epoch that ran, BEFORE that epoch's update (+inf before the first)
 *   An epoch runs while `last_loss > tolerance and epochs_run <= max_epoch` (surface_generator.py:196; note <=); a facet
 *   that stops sets done = 1 and is frozen, the others go on.
 *   Adam: torch.optim.adam._single_tensor_adam in fp32 with the arithmetic of art_adam_step (bias corrections in double).
 *   Scheduler (use_scheduler != 0): torch.optim.lr_scheduler.ReduceLROnPlateau.step(loss) in double; mode_max 0 = "min",
 *   threshold_abs 0 = "rel".
 * ------------------------------------------------------------------------------------------- */
int art_surface_fit_run(float *control_points, float *exp_avg, float *exp_avg_sq, double *state_f64, int32_t *state_i32,
                        float *last_loss, const float *targets, const int32_t *n_valid, const int32_t *perm,
                        const int32_t *cell_start, const float *table, int64_t B, int64_t N, int64_t nu, int64_t nv, int p,
                        int q, int method, int64_t epochs, double tolerance, int64_t max_epoch, double beta1, double beta2,
                        double eps, double weight_decay, int maximize, int use_scheduler, int mode_max, double factor,
                        int64_t patience, double threshold, int threshold_abs, int64_t cooldown, double min_lr,
                        double scheduler_eps, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ARTIST_HIP_SURFACE_FIT_H */
