// surface_fit_kernels.hip - art_surface_fit_prepare / _loss_grad / _run (include/artist_hip_surface_fit.h): SurfaceGenerator.fit_nurbs
// (artist/scenario/surface_generator.py:71-223) for a batch of independent facets, gfx950.
//
// The reference fits one facet after the other, 400 Adam epochs each, every epoch a chain of some fifty small kernels and a host
// read of the loss.  Here ONE WORKGROUP owns one facet for the whole fit: the control net and its two Adam moments live in LDS,
// the evaluation points never change, so everything that depends on them alone - knot spans, A2.3 basis values and derivatives -
// is tabulated once by `prepare` and the epoch is three phases separated by barriers:
//
//   phase 1  (thread <-> point, in span-cell order)  S, dS/du, dS/dv from the table row and the (p+1)(q+1) control points the
//            cell touches; the point's squared error and its gradient w.r.t. S (points fit) or dS/du, dS/dv (normals fit,
//            through normalize(dS/du x dS/dv)) go to LDS;
//   phase 2  (thread <-> (cell, r, s))  the cell's points, in index order, contracted with Nu[r] Nv[s] (and the derivatives):
//            one partial sum per control point the cell touches; meanwhile wave 0 adds the squared errors (lane l owns positions
//            l, l + 64, ... in fp64, then a fixed shuffle tree);
//   phase 3  (thread <-> control-point component)  adds the at most (p+1)(q+1) cell partials in cell order -> gradient, and in
//            `run` steps Adam on that element right away; every thread then steps the plateau scheduler on the (uniform) loss.
//
// Every sum has one owner and a fixed order: no atomics of any kind, the bits of a facet depend on its own data only - not on
// B, not on the workgroup size (chosen from N), not on where the table lives (LDS when it fits, global otherwise), not on how
// the epochs are chunked into launches.
//
// A facet with more points than LDS holds beside its net (a measured facet has ~80 000) is still one workgroup's: the same
// fit_epoch then runs phases 1 and 2 per chunk of sorted positions with the running sums carried from chunk to chunk (FitMode),
// and prepare sorts in tiles (surface_fit_prepare_tiled_kernel).  There is one text of every expression of the fit, so the
// order of every sum, and with it the bits, cannot differ between the two.
// ARTIST_HIP_DEBUG=1 ARTIST_HIP_FIT_CHUNK=<points> forces both at any N with that chunk / tile length (tests).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "launch_common.hpp"
#include "nurbs_basis.hpp"

#include "../../include/artist_hip_surface_fit.h"

namespace art {
namespace {

constexpr int kFitMaxBlock = 512;              // run / loss_grad: launch bound (the block is sized from N, see fit_block)
constexpr int kFitPrepBlock = 256;
constexpr int64_t kFitLdsBudget = 160 * 1024;  // LDS of a CU (MI355X_MICROARCH: a single workgroup may take all of it)
constexpr int64_t kFitMaxN = 1 << 20;          // rows per facet: positions, j * W and C * ng stay far inside int
constexpr int64_t kFitResidentMaxN = 16384;    // the resident kernels (every per-point array of a facet in LDS) up to here
constexpr int kFitPrepTile = 16384;            // tiled prepare: cell ids staged in LDS per tile
constexpr int64_t kFitMaxCells = 4096;
constexpr int kFitMaxEpochs = 1024;            // per launch: the bias corrections of the launch's steps are tabulated in LDS

// Table row of one point: [spans, sum_r Nu[r], Nu[S], Du[S], Nv[S], Dv[S], cell]; the odd row length keeps the 64 rows a wave
// reads in phase 1 on different LDS banks.
template <int DEG> struct FitRec {
    static constexpr int S = (DEG > 0 ? DEG : kMaxDeg) + 1;
    static constexpr int W = 3 + 4 * S;
};

inline int fit_deg(int p, int q) { return (p == q && (p == 2 || p == 3)) ? p : 0; }

struct FitArgs {
    int N, nu, nv, p, q, method;
    const float* targets;        // [B,N,4] points or normals, by method
    const int32_t* n_valid;      // [B] or null
    const int32_t* perm;         // [B,N]
    const int32_t* cell_start;   // [B,ncells+1]
    const float* table;          // [B,N,W]
    // loss_grad
    const float* cp_in; float* loss; float* grad; float4* points_out; float4* normals_out;
    // run
    float* cp; float* m; float* v; double* sf64; int32_t* si32; float* last_loss;
    int epochs, max_epoch;
    float tolerance, beta1, beta2, one_minus_beta1, one_minus_beta2, eps, weight_decay, grad_sign;
    double beta1d, beta2d;
    int sched, mode_max, thr_abs, patience, cooldown;
    double factor, threshold, min_lr, sched_eps;
};

// Offsets (in floats) of a workgroup's LDS block.  [targets N x 4 | bc1 doubles | 1/sqrt(bc2) | cp | m | v | cell partials |
// point gradients | squared errors | cell offsets | loss | table]; the first two and the table only where used.
struct FitLayout { int tgt, bc1, ibc2, cp, m, v, part, g, sq, cells, red, tab, total; };

__host__ __device__ inline FitLayout fit_layout(int N, int nu, int nv, int p, int q, int method, int W, int epochs, bool tab_lds)
{
    const int ncp = nu * nv * 3, ncells = (nu - p) * (nv - q), PQ = (p + 1) * (q + 1), ng = method == ART_FIT_POINTS ? 3 : 6;
    FitLayout L;
    int o = 0;
    L.tgt = o;   o += tab_lds ? N * 4 : 0;
    L.bc1 = o;   o += 2 * epochs;                  // doubles: o is even here
    L.ibc2 = o;  o += epochs;
    L.cp = o;    o += ncp;
    L.m = o;     o += ncp;
    L.v = o;     o += ncp;
    L.part = o;  o += ncells * PQ * 3;
    L.g = o;     o += N * ng;
    L.sq = o;    o += N;
    L.cells = o; o += ncells + 1;
    L.red = o;   o += 2;
    L.tab = o;   o += tab_lds ? N * W : 0;
    L.total = o;
    return L;
}

// Workgroup size from N: as few rounds of phase 1 as a 512-thread group allows, the rounds filled evenly (N = 800: two rounds
// of 400 points on 448 threads instead of 800 on 1024 with a quarter of the group idle in every other phase).
inline int fit_block(int64_t N)
{
    const int64_t rounds = (N + kFitMaxBlock - 1) / kFitMaxBlock;
    const int64_t per = (N + rounds - 1) / rounds;
    return (int)(((per + 63) / 64) * 64);
}

// The arithmetic of eval_from_records (nurbs_kernels.hip), i.e. surfaces.py:592-613 in the reference's order, from a table row.
template <int DEG>
__device__ __forceinline__ void fit_eval_point(const FitArgs& a, const float* s_cp, const float* rec, float* S0, float* Su, float* Sv)
{
    constexpr int S = FitRec<DEG>::S;
    const int p = DEG > 0 ? DEG : a.p, q = DEG > 0 ? DEG : a.q;
    const int packed = __float_as_int(rec[0]);
    const int su = packed & 0xffff, sv = packed >> 16;
    const float wsum = rec[1];
    const float *Nu = rec + 2, *Du = Nu + S, *Nv = Du + S, *Dv = Nv + S;
    float d0[4] = {0.f, 0.f, 0.f, 0.f}, du[3] = {0.f, 0.f, 0.f}, dv[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < S; ++s) {
        if (s > q) break;
        float t[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < S; ++r) {
            if (r > p) break;
            const float* c3 = s_cp + ((su - p + r) * a.nv + (sv - q + s)) * 3;
            const float bn = Nu[r], bd = Du[r];
            t[0] += bn * c3[0]; t[1] += bn * c3[1]; t[2] += bn * c3[2];
            t[3] += bd * c3[0]; t[4] += bd * c3[1]; t[5] += bd * c3[2];
        }
        const float bn = Nv[s], bd = Dv[s];
        d0[0] += bn * t[0]; d0[1] += bn * t[1]; d0[2] += bn * t[2]; d0[3] += bn * wsum;
        du[0] += bn * t[3]; du[1] += bn * t[4]; du[2] += bn * t[5];
        dv[0] += bd * t[0]; dv[1] += bd * t[1]; dv[2] += bd * t[2];
    }
    S0[0] = d0[0]; S0[1] = d0[1]; S0[2] = d0[2]; S0[3] = d0[3];
    Su[0] = du[0]; Su[1] = du[1]; Su[2] = du[2];
    Sv[0] = dv[0]; Sv[1] = dv[1]; Sv[2] = dv[2];
}

__device__ __forceinline__ double fit_wave_sum_f64(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// Where an epoch finds a facet's per-point data.  kFitLds: table and sorted targets staged in LDS; kFitStream: read from the
// global buffers prepare wrote, every per-point array of the facet still in LDS; kFitChunked: streamed as well, and s_g / s_sq
// hold one chunk of sorted positions (L is then the layout of ONE CHUNK: fit_layout with N = chunk).
enum FitMode { kFitLds = 0, kFitStream = 1, kFitChunked = 2 };

// One epoch's forward and backward for facet b with n valid points; the control net is in s_cp.  Calls own(e, g) once for every
// control-point component e (by the thread that owns it) with its gradient g, and leaves the loss in lds[L.red] (valid after
// the caller's next barrier).  The caller has synchronised the workgroup since s_cp was last written.
//
// Phases 1 and 2 run per chunk of `chunk` sorted positions (a multiple of 64); a resident facet is ONE chunk, positions 0 .. n,
// and `chunk` is not read.  Every sum has the same order however the positions are chunked, so the result is the same bits: the
// running sum of a (cell, r, s) is carried in s_part from chunk to chunk - a cell's points are consecutive positions, taken in
// index order -, lane l of wave 0 carries its fp64 sum of the squared errors at positions l, l + 64, ... across the chunks (a
// chunk starts at a multiple of 64, so the positions keep their lane), and the shuffle tree and phase 3 run once, after the
// last chunk.  Only the cells that intersect a chunk have work in its phase 2.
template <int DEG, FitMode MODE, typename Own>
__device__ __forceinline__ void fit_epoch(const FitArgs& a, const FitLayout& L, float* lds, int b, int n, int chunk, Own own)
{
    constexpr int S = FitRec<DEG>::S, W = FitRec<DEG>::W;
    constexpr bool TAB_LDS = MODE == kFitLds, CHUNKED = MODE == kFitChunked;
    const int p = DEG > 0 ? DEG : a.p, q = DEG > 0 ? DEG : a.q;
    const int tid = threadIdx.x, T = blockDim.x;
    const int ncu = a.nu - p, ncv = a.nv - q, ncells = ncu * ncv, PQ = (p + 1) * (q + 1), ncp = a.nu * a.nv * 3;
    const bool fit_points = a.method == ART_FIT_POINTS;
    const int ng = fit_points ? 3 : 6;
    const float* s_cp = lds + L.cp;
    float* s_part = lds + L.part;
    float* s_g = lds + L.g;
    float* s_sq = lds + L.sq;
    const int* s_cells = reinterpret_cast<const int*>(lds + L.cells);
    const float* tab = TAB_LDS ? lds + L.tab : a.table + (int64_t)b * a.N * W;
    const int32_t* perm = a.perm + (int64_t)b * a.N;
    const float4* tgt_g = reinterpret_cast<const float4*>(a.targets) + (int64_t)b * a.N;
    const float4* tgt_s = reinterpret_cast<const float4*>(lds + L.tgt);

    const float scale = (float)(2.0 / (4.0 * (double)n));          // MSELoss backward: (2 / numel) * (input - target)
    double sq_acc = 0.0;
    // wave 0, once its lanes hold their sums over all positions: the fixed shuffle tree.  A resident facet has them in phase 2,
    // ahead of the chains; the chunked epoch after its last chunk (inside the chunk loop the tree costs the compiler 36 B of
    // scratch per lane in one instantiation).
    auto loss_tree = [&]() {
        const double sum = fit_wave_sum_f64(sq_acc);
        if (tid == 0) lds[L.red] = (float)(sum / (4.0 * (double)n));
    };
    int first = 0;                                                  // position j's slot in s_g / s_sq is j - first
    do {
        const int last = CHUNKED ? min(first + chunk, n) : n;
        // ---- phase 1: the chunk's points
        for (int j = first + tid; j < last; j += T) {
            const float* rec = tab + (int64_t)j * W;
            float* go = s_g + (j - first) * ng;
            float S0[4], Su[3], Sv[3];
            fit_eval_point<DEG>(a, s_cp, rec, S0, Su, Sv);
            // surfaces.py:615-661 (finish_point of nurbs_kernels.hip without canting)
            const float cx = Su[1] * Sv[2] - Su[2] * Sv[1];
            const float cy = Su[2] * Sv[0] - Su[0] * Sv[2];
            const float cz = Su[0] * Sv[1] - Su[1] * Sv[0];
            const float px = S0[0] / S0[3], py = S0[1] / S0[3], pz = S0[2] / S0[3];
            const float ncl = fmaxf(norm3(cx, cy, cz), 1e-12f);
            const float nx = cx / ncl, ny = cy / ncl, nz = cz / ncl;
            float4 t;
            if (TAB_LDS) t = tgt_s[j]; else t = tgt_g[perm[j]];
            float e0, e1, e2, e3;
            if (fit_points) { e0 = px - t.x; e1 = py - t.y; e2 = pz - t.z; e3 = 1.0f - t.w; }
            else { e0 = nx - t.x; e1 = ny - t.y; e2 = nz - t.z; e3 = 0.0f - t.w; }
            s_sq[j - first] = ((e0 * e0 + e1 * e1) + e2 * e2) + e3 * e3;
            const float g0 = scale * e0, g1 = scale * e1, g2 = scale * e2;
            if (fit_points) {
                const float iw = 1.0f / S0[3];
                go[0] = g0 * iw; go[1] = g1 * iw; go[2] = g2 * iw;
            } else {
                // point_adjoint of nurbs_kernels.hip: through normalize(c), c = Su x Sv
                const float nc = norm3(cx, cy, cz);
                float gc0, gc1, gc2;
                if (nc < 1e-12f) {
                    gc0 = g0 / 1e-12f; gc1 = g1 / 1e-12f; gc2 = g2 / 1e-12f;
                } else {
                    const float inv = 1.0f / nc;
                    const float ux = cx * inv, uy = cy * inv, uz = cz * inv;
                    const float dot = ux * g0 + uy * g1 + uz * g2;
                    gc0 = (g0 - ux * dot) * inv; gc1 = (g1 - uy * dot) * inv; gc2 = (g2 - uz * dot) * inv;
                }
                go[0] = Sv[1] * gc2 - Sv[2] * gc1; go[1] = Sv[2] * gc0 - Sv[0] * gc2; go[2] = Sv[0] * gc1 - Sv[1] * gc0;
                go[3] = gc1 * Su[2] - gc2 * Su[1]; go[4] = gc2 * Su[0] - gc0 * Su[2]; go[5] = gc0 * Su[1] - gc1 * Su[0];
            }
            if (a.points_out != nullptr) {
                const int64_t out_row = (int64_t)b * a.N + perm[j];
                a.points_out[out_row] = make_float4(px, py, pz, 1.0f);
                a.normals_out[out_row] = make_float4(nx, ny, nz, 0.0f);
            }
        }
        __syncthreads();

        // ---- phase 2: the loss (wave 0 first), then one running sum per (cell, r, s)
        if (tid < 64) {
            for (int j = first + tid; j < last; j += 64) sq_acc += (double)s_sq[j - first];
            if (!CHUNKED) loss_tree();
        }
        for (int it = tid; it < ncells * PQ; it += T) {
            const int c = it / PQ, rs = it - c * PQ;
            const int r = rs / (q + 1), s = rs - r * (q + 1);
            const int j0 = CHUNKED ? max(s_cells[c], first) : s_cells[c];
            const int j1 = CHUNKED ? min(s_cells[c + 1], last) : s_cells[c + 1];
            float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f;
            if (first > 0) {                                        // a later chunk: nothing to add, or the sum so far
                if (j0 >= j1) continue;
                acc0 = s_part[it * 3]; acc1 = s_part[it * 3 + 1]; acc2 = s_part[it * 3 + 2];
            }
            // (fetching the weights of eight positions ahead of their adds was tried and was about a quarter slower at
            // N = 20 000 and 80 000: DESIGN.md 4.7)
            for (int j = j0; j < j1; ++j) {
                const float* rec = tab + (int64_t)j * W;
                const float* gj = s_g + (j - first) * ng;
                if (fit_points) {
                    const float w00 = rec[2 + r] * rec[2 + 2 * S + s];
                    acc0 += w00 * gj[0]; acc1 += w00 * gj[1]; acc2 += w00 * gj[2];
                } else {
                    const float w10 = rec[2 + S + r] * rec[2 + 2 * S + s], w01 = rec[2 + r] * rec[2 + 3 * S + s];
                    acc0 += w10 * gj[0] + w01 * gj[3]; acc1 += w10 * gj[1] + w01 * gj[4]; acc2 += w10 * gj[2] + w01 * gj[5];
                }
            }
            s_part[it * 3] = acc0; s_part[it * 3 + 1] = acc1; s_part[it * 3 + 2] = acc2;
        }
        __syncthreads();
        first += chunk;
    } while (CHUNKED && first < n);
    if (CHUNKED && tid < 64) loss_tree();

    // ---- phase 3: a control-point component adds the partials of the cells that touch it, in cell order
    for (int e = tid; e < ncp; e += T) {
        const int cell = e / 3, k = e - 3 * cell;
        const int ar = cell / a.nv, ac = cell - ar * a.nv;
        float acc = 0.f;
        for (int cu = max(0, ar - p); cu <= min(ar, ncu - 1); ++cu)
            for (int cv = max(0, ac - q); cv <= min(ac, ncv - 1); ++cv)
                acc += s_part[((cu * ncv + cv) * PQ + (ar - cu) * (q + 1) + (ac - cv)) * 3 + k];
        own(e, acc);
    }
}

// Stage what an epoch reads besides the control net: the cell offsets, and - when they live in LDS - the table and the targets
// in sorted order.  Followed by the caller's barrier.
template <int DEG, FitMode MODE>
__device__ __forceinline__ void fit_stage(const FitArgs& a, const FitLayout& L, float* lds, int b, int n)
{
    constexpr int W = FitRec<DEG>::W;
    const int ncells = (a.nu - a.p) * (a.nv - a.q);
    int* s_cells = reinterpret_cast<int*>(lds + L.cells);
    for (int i = threadIdx.x; i <= ncells; i += blockDim.x) s_cells[i] = min(max(a.cell_start[(int64_t)b * (ncells + 1) + i], 0), n);
    if (MODE == kFitLds) {
        const float* g_tab = a.table + (int64_t)b * a.N * W;
        for (int i = threadIdx.x; i < n * W; i += blockDim.x) lds[L.tab + i] = g_tab[i];
        const float4* tgt_g = reinterpret_cast<const float4*>(a.targets) + (int64_t)b * a.N;
        const int32_t* perm = a.perm + (int64_t)b * a.N;
        float4* tgt_s = reinterpret_cast<float4*>(lds + L.tgt);
        for (int j = threadIdx.x; j < n; j += blockDim.x) tgt_s[j] = tgt_g[min(max(perm[j], 0), a.N - 1)];
    }
}

// The facet's point count: the caller's n_valid, but never more than the rows prepare sorted (the last cell offset) - positions
// beyond those have no row (perm = -1) and no table entry, so perm[j] is a row of the facet for every j the kernels touch.
__device__ __forceinline__ int fit_n_valid(const FitArgs& a, int b)
{
    const int ncells = (a.nu - a.p) * (a.nv - a.q);
    const int sorted = min(max(a.cell_start[(int64_t)b * (ncells + 1) + ncells], 0), a.N);
    return a.n_valid != nullptr ? min(max(a.n_valid[b], 0), sorted) : sorted;
}

// adam_element of optim_kernels.hip (torch/optim/adam.py, _single_tensor_adam) on component e with gradient g
__device__ __forceinline__ void fit_adam_element(const FitArgs& a, float* s_cp, float* s_m, float* s_v, int e, float g, float step_size,
                                                 float inv_bc2_sqrt)
{
    float pe = s_cp[e], me = s_m[e], ve = s_v[e];
    float gr = a.grad_sign * g;
    if (a.weight_decay != 0.0f) gr = gr + a.weight_decay * pe;
    me = me + (gr - me) * a.one_minus_beta1;
    ve = ve * a.beta2 + (a.one_minus_beta2 * gr) * gr;
    const float denom = sqrtf(ve) * inv_bc2_sqrt + a.eps;
    pe = pe - step_size * (me / denom);
    s_cp[e] = pe; s_m[e] = me; s_v[e] = ve;
}

// ReduceLROnPlateau.step(loss.abs().mean()) in Python's doubles
__device__ __forceinline__ void fit_plateau_step(const FitArgs& a, float loss, double& lr, double& best, int& num_bad, int& cool)
{
    const double cur = fabs((double)loss);
    bool better;
    if (a.mode_max) better = a.thr_abs ? cur > best + a.threshold : cur > best * (a.threshold + 1.0);
    else better = a.thr_abs ? cur < best - a.threshold : cur < best * (1.0 - a.threshold);
    if (better) { best = cur; num_bad = 0; } else num_bad += 1;
    if (cool > 0) { cool -= 1; num_bad = 0; }
    if (num_bad > a.patience) {
        const double new_lr = fmax(lr * a.factor, a.min_lr);
        if (lr - new_lr > a.sched_eps) lr = new_lr;
        cool = a.cooldown; num_bad = 0;
    }
}

// The two kernels, one instantiation per degree and FitMode.  `chunk` (kFitChunked only) is the last argument, behind what the
// resident launches have always passed.
template <int DEG, FitMode MODE>
__global__ __launch_bounds__(kFitMaxBlock) void surface_fit_loss_grad_kernel(FitArgs a, FitLayout L, int chunk)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int b = blockIdx.x, ncp = a.nu * a.nv * 3;
    const int n = fit_n_valid(a, b);
    for (int i = threadIdx.x; i < ncp; i += blockDim.x) lds[L.cp + i] = a.cp_in[(int64_t)b * ncp + i];
    fit_stage<DEG, MODE>(a, L, lds, b, n);
    __syncthreads();
    float* out = a.grad + (int64_t)b * ncp;
    fit_epoch<DEG, MODE>(a, L, lds, b, n, chunk, [&](int e, float g) { out[e] = g; });
    if (threadIdx.x == 0) a.loss[b] = lds[L.red];      // (written by this thread, before phase 3)
}

template <int DEG, FitMode MODE>
__global__ __launch_bounds__(kFitMaxBlock) void surface_fit_run_kernel(FitArgs a, FitLayout L, int chunk)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int b = blockIdx.x, ncp = a.nu * a.nv * 3, tid = threadIdx.x, T = blockDim.x;
    const int n = fit_n_valid(a, b);
    // the facet's scalars: every thread holds its own copy, all evolve alike
    double lr = a.sf64[2 * (int64_t)b], best = a.sf64[2 * (int64_t)b + 1];
    const int32_t* si = a.si32 + 5 * (int64_t)b;
    int step = si[0], num_bad = si[1], cool = si[2], epochs_run = si[3], done = si[4];
    float last = a.last_loss[b];
    float *s_cp = lds + L.cp, *s_m = lds + L.m, *s_v = lds + L.v;
    double* s_bc1 = reinterpret_cast<double*>(lds + L.bc1);
    float* s_ibc2 = lds + L.ibc2;
    for (int i = tid; i < ncp; i += T) {
        s_cp[i] = a.cp[(int64_t)b * ncp + i]; s_m[i] = a.m[(int64_t)b * ncp + i]; s_v[i] = a.v[(int64_t)b * ncp + i];
    }
    // bias corrections of this launch's steps (torch/optim/adam.py: 1 - beta ** step in double), one step per thread
    for (int i = tid; i < a.epochs; i += T) {
        const double st = (double)(step + 1 + i);
        s_bc1[i] = 1.0 - pow(a.beta1d, st);
        s_ibc2[i] = (float)(1.0 / sqrt(1.0 - pow(a.beta2d, st)));
    }
    fit_stage<DEG, MODE>(a, L, lds, b, n);
    __syncthreads();
    for (int it = 0; it < a.epochs && !done; ++it) {
        if (!(last > a.tolerance) || epochs_run > a.max_epoch) { done = 1; break; }     // surface_generator.py:196
        const float step_size = (float)(lr / s_bc1[it]);
        const float inv_bc2_sqrt = s_ibc2[it];
        fit_epoch<DEG, MODE>(a, L, lds, b, n, chunk, [&](int e, float g) {
            fit_adam_element(a, s_cp, s_m, s_v, e, g, step_size, inv_bc2_sqrt);
        });
        __syncthreads();
        const float loss = lds[L.red];
        if (a.sched) fit_plateau_step(a, loss, lr, best, num_bad, cool);
        last = loss; epochs_run += 1; step += 1;
    }
    if (!done && (!(last > a.tolerance) || epochs_run > a.max_epoch)) done = 1;
    for (int i = tid; i < ncp; i += T) {
        a.cp[(int64_t)b * ncp + i] = s_cp[i]; a.m[(int64_t)b * ncp + i] = s_m[i]; a.v[(int64_t)b * ncp + i] = s_v[i];
    }
    if (tid == 0) {
        a.sf64[2 * (int64_t)b] = lr; a.sf64[2 * (int64_t)b + 1] = best;
        int32_t* so = a.si32 + 5 * (int64_t)b;
        so[0] = step; so[1] = num_bad; so[2] = cool; so[3] = epochs_run; so[4] = done;
        a.last_loss[b] = last;
    }
}

// ---- prepare ---------------------------------------------------------------------------------------------------------------

struct PrepArgs {
    const float* targets_points; const int32_t* n_valid; const float* knots_u; const float* knots_v;
    int N, nu, nv, p, q;
    float* eval_uv; float* cp; int32_t* perm; int32_t* cell_start; float* table;
};

// torch.linspace's fp32 values on the CPU (aten RangeFactories: symmetric about the middle, each value ONE fused multiply-add -
// the only place in this library where a fused operation is asked for, because the reference's values are made by one)
__device__ __forceinline__ float fit_linspace(float start, float end, int steps, int i)
{
    const float step = (end - start) / (float)(steps - 1);
    return i < steps / 2 ? __fmaf_rn(step, (float)i, start) : __fmaf_rn(-step, (float)(steps - i - 1), end);
}

// ---- the stages both prepare kernels are written with
//
// What a facet's rows are normalised with: the minima of the e and n columns and the denominators of normalize_points.
struct PrepFrame { float mn_e, mn_n, den_e, den_n; };

// The start of prepare for facet b with n valid rows: the knots to LDS, the extrema, the initial net.  Holds a barrier.
template <int DEG>
__device__ __forceinline__ PrepFrame fit_prep_frame(const PrepArgs& a, int b, int n, float* s_ku, float* s_kv, float* s_ext)
{
    const int tid = threadIdx.x, T = blockDim.x;
    const int p = DEG > 0 ? DEG : a.p, q = DEG > 0 ? DEG : a.q;
    const int nku = a.nu + p + 1, nkv = a.nv + q + 1;
    const float4* tp = reinterpret_cast<const float4*>(a.targets_points) + (int64_t)b * a.N;
    for (int i = tid; i < nku; i += T) s_ku[i] = a.knots_u[i];
    for (int i = tid; i < nkv; i += T) s_kv[i] = a.knots_v[i];
    // extrema of the e and n columns over the valid rows (order does not matter for min / max)
    float mn_e = INFINITY, mx_e = -INFINITY, mn_n = INFINITY, mx_n = -INFINITY;
    for (int i = tid; i < n; i += T) {
        const float4 x = tp[i];
        mn_e = fminf(mn_e, x.x); mx_e = fmaxf(mx_e, x.x); mn_n = fminf(mn_n, x.y); mx_n = fmaxf(mx_n, x.y);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mn_e = fminf(mn_e, __shfl_down(mn_e, off, 64)); mx_e = fmaxf(mx_e, __shfl_down(mx_e, off, 64));
        mn_n = fminf(mn_n, __shfl_down(mn_n, off, 64)); mx_n = fmaxf(mx_n, __shfl_down(mx_n, off, 64));
    }
    if ((tid & 63) == 0) { float* e = s_ext + 4 * (tid >> 6); e[0] = mn_e; e[1] = mx_e; e[2] = mn_n; e[3] = mx_n; }
    __syncthreads();
    mn_e = s_ext[0]; mx_e = s_ext[1]; mn_n = s_ext[2]; mx_n = s_ext[3];
    for (int w = 1; w < T / 64; ++w) {
        mn_e = fminf(mn_e, s_ext[4 * w]); mx_e = fmaxf(mx_e, s_ext[4 * w + 1]);
        mn_n = fminf(mn_n, s_ext[4 * w + 2]); mx_n = fmaxf(mx_n, s_ext[4 * w + 3]);
    }
    // the initial net (surface_generator.py:148-174)
    const float width = n > 0 ? mx_e - mn_e : 0.0f, height = n > 0 ? mx_n - mn_n : 0.0f;      // (no valid rows: a zero net)
    float* cp = a.cp + (int64_t)b * a.nu * a.nv * 3;
    for (int i = tid; i < a.nu * a.nv; i += T) {
        const int r = i / a.nv, c = i - r * a.nv;
        cp[3 * i] = fit_linspace(-width / 2.0f, width / 2.0f, a.nu, r);
        cp[3 * i + 1] = fit_linspace(-height / 2.0f, height / 2.0f, a.nv, c);
        cp[3 * i + 2] = 0.0f;
    }
    // coordinates.normalize_points: (x - min + 1e-5) / max(x - min + 2e-5); the maximum is taken at the largest x (monotone)
    PrepFrame f;
    f.mn_e = mn_e; f.mn_n = mn_n; f.den_e = (mx_e - mn_e) + 2e-5f; f.den_n = (mx_n - mn_n) + 2e-5f;
    return f;
}

__device__ __forceinline__ float2 fit_prep_uv(const PrepFrame& f, const float4 t)
{
    return make_float2(((t.x - f.mn_e) + 1e-5f) / f.den_e, ((t.y - f.mn_n) + 1e-5f) / f.den_n);
}

// The span cell (u-major) of a normalised point.
template <int DEG>
__device__ __forceinline__ int fit_prep_cell(const PrepArgs& a, const float2 x, const float* s_ku, const float* s_kv)
{
    const int p = DEG > 0 ? DEG : a.p, q = DEG > 0 ? DEG : a.q;
    const int ncu = a.nu - p, ncv = a.nv - q;
    const int su = find_span(x.x, s_ku, a.nu, p, 1, ncu + 1), sv = find_span(x.y, s_kv, a.nv, q, 1, ncv + 1);
    return (su - p) * ncv + (sv - q);
}

// The table row of the point with target row t.
template <int DEG>
__device__ __forceinline__ void fit_prep_table_row(const PrepArgs& a, const PrepFrame& f, const float4 t, const float* s_ku,
                                                   const float* s_kv, float* rec)
{
    constexpr int S = FitRec<DEG>::S;
    const int p = DEG > 0 ? DEG : a.p, q = DEG > 0 ? DEG : a.q;
    const int ncu = a.nu - p, ncv = a.nv - q;
    const float2 x = fit_prep_uv(f, t);
    const float u = x.x, v = x.y;
    const int su = find_span(u, s_ku, a.nu, p, 1, ncu + 1), sv = find_span(v, s_kv, a.nv, q, 1, ncv + 1);
    float Nu[S], Du[S], Nv[S], Dv[S];
    basis<DEG>(u, s_ku, su, p, Nu, Du);
    basis<DEG>(v, s_kv, sv, q, Nv, Dv);
    rec[0] = __int_as_float(su | (sv << 16));
    float wsum = 0.f;
#pragma unroll
    for (int r = 0; r < S; ++r) {
        const bool in_u = r <= p, in_v = r <= q;
        if (in_u) wsum += Nu[r] * 1.0f;      // the homogeneous coordinate's inner sum (line_basis of nurbs_kernels.hip)
        rec[2 + r] = in_u ? Nu[r] : 0.0f; rec[2 + S + r] = in_u ? Du[r] : 0.0f;
        rec[2 + 2 * S + r] = in_v ? Nv[r] : 0.0f; rec[2 + 3 * S + r] = in_v ? Dv[r] : 0.0f;
    }
    rec[1] = wsum;
    rec[2 + 4 * S] = __int_as_float((su - p) * ncv + (sv - q));
}

// LDS: [cell of point i: N ints][perm: N ints][cell offsets: ncells + 1 ints][knots_u][knots_v][8 x 4 wave extrema]
template <int DEG>
__global__ __launch_bounds__(kFitPrepBlock) void surface_fit_prepare_kernel(PrepArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int W = FitRec<DEG>::W;
    const int b = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
    const int p = DEG > 0 ? DEG : a.p, q = DEG > 0 ? DEG : a.q;
    const int ncells = (a.nu - p) * (a.nv - q), nku = a.nu + p + 1, nkv = a.nv + q + 1;
    const int n = a.n_valid != nullptr ? min(max(a.n_valid[b], 0), a.N) : a.N;
    int* s_cell = reinterpret_cast<int*>(lds);
    int* s_perm = s_cell + a.N;
    int* s_start = s_perm + a.N;
    float* s_ku = reinterpret_cast<float*>(s_start + ncells + 1);
    float* s_kv = s_ku + nku;
    float* s_ext = s_kv + nkv;
    const float4* tp = reinterpret_cast<const float4*>(a.targets_points) + (int64_t)b * a.N;
    const PrepFrame f = fit_prep_frame<DEG>(a, b, n, s_ku, s_kv, s_ext);
    float2* uv = reinterpret_cast<float2*>(a.eval_uv) + (int64_t)b * a.N;
    for (int i = tid; i < a.N; i += T) {
        float2 x = make_float2(0.f, 0.f);
        if (i < n) {
            x = fit_prep_uv(f, tp[i]);
            s_cell[i] = fit_prep_cell<DEG>(a, x, s_ku, s_kv);
        }
        uv[i] = x;
    }
    __syncthreads();
    // counting sort by cell, stable in the row index: a thread per cell walks the rows in order (twice)
    for (int c = tid; c < ncells; c += T) {
        int cnt = 0;
        for (int i = 0; i < n; ++i) cnt += s_cell[i] == c ? 1 : 0;
        s_start[c + 1] = cnt;
    }
    __syncthreads();
    if (tid == 0) {
        s_start[0] = 0;
        for (int c = 0; c < ncells; ++c) s_start[c + 1] += s_start[c];
    }
    __syncthreads();
    for (int c = tid; c < ncells; c += T) {
        int o = s_start[c];
        for (int i = 0; i < n; ++i)
            if (s_cell[i] == c) s_perm[o++] = i;
    }
    for (int c = tid; c <= ncells; c += T) a.cell_start[(int64_t)b * (ncells + 1) + c] = s_start[c];
    __syncthreads();
    // the table rows, in sorted order
    float* tab = a.table + (int64_t)b * a.N * W;
    for (int j = tid; j < a.N; j += T) {
        a.perm[(int64_t)b * a.N + j] = j < n ? s_perm[j] : -1;
        float* rec = tab + (int64_t)j * W;
        if (j >= n) {
            for (int k = 0; k < W; ++k) rec[k] = 0.0f;
            continue;
        }
        fit_prep_table_row<DEG>(a, f, tp[s_perm[j]], s_ku, s_kv, rec);
    }
}

// The same for a facet whose rows do not fit in LDS.  The counting sort keeps its scheme - a thread per cell walks the rows in
// order, twice - over tiles of `tile` cell ids staged in LDS: a cell's thread carries its count, then its write offset, from
// tile to tile (in s_start / s_off: a thread may own several cells), and perm goes straight to global memory, which the table
// pass reads back after a barrier.  Row i's cell is computed again for each pass: the same arithmetic, the same value.
// LDS: [cell of the tile's rows: tile ints][cell offsets: ncells + 1 ints][write offsets: ncells ints][knots_u][knots_v][extrema]
template <int DEG>
__global__ __launch_bounds__(kFitPrepBlock) void surface_fit_prepare_tiled_kernel(PrepArgs a, int tile)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int W = FitRec<DEG>::W;
    const int b = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
    const int p = DEG > 0 ? DEG : a.p, q = DEG > 0 ? DEG : a.q;
    const int ncells = (a.nu - p) * (a.nv - q), nku = a.nu + p + 1, nkv = a.nv + q + 1;
    const int n = a.n_valid != nullptr ? min(max(a.n_valid[b], 0), a.N) : a.N;
    int* s_cell = reinterpret_cast<int*>(lds);
    int* s_start = s_cell + tile;
    int* s_off = s_start + ncells + 1;
    float* s_ku = reinterpret_cast<float*>(s_off + ncells);
    float* s_kv = s_ku + nku;
    float* s_ext = s_kv + nkv;
    const float4* tp = reinterpret_cast<const float4*>(a.targets_points) + (int64_t)b * a.N;
    int32_t* perm = a.perm + (int64_t)b * a.N;
    const PrepFrame f = fit_prep_frame<DEG>(a, b, n, s_ku, s_kv, s_ext);
    float2* uv = reinterpret_cast<float2*>(a.eval_uv) + (int64_t)b * a.N;
    for (int i = tid; i < a.N; i += T) uv[i] = i < n ? fit_prep_uv(f, tp[i]) : make_float2(0.f, 0.f);
    // first walk: the cells' counts
    for (int c = tid; c < ncells; c += T) s_start[c + 1] = 0;
    for (int first = 0; first < n; first += tile) {
        const int len = min(tile, n - first);
        for (int i = tid; i < len; i += T) s_cell[i] = fit_prep_cell<DEG>(a, fit_prep_uv(f, tp[first + i]), s_ku, s_kv);
        __syncthreads();
        for (int c = tid; c < ncells; c += T) {
            int cnt = s_start[c + 1];
            for (int i = 0; i < len; ++i) cnt += s_cell[i] == c ? 1 : 0;
            s_start[c + 1] = cnt;
        }
        __syncthreads();
    }
    __syncthreads();      // (a facet without rows ran no tile)
    if (tid == 0) {
        s_start[0] = 0;
        for (int c = 0; c < ncells; ++c) s_start[c + 1] += s_start[c];
    }
    __syncthreads();
    // second walk: the rows to their places
    for (int c = tid; c < ncells; c += T) s_off[c] = s_start[c];
    for (int first = 0; first < n; first += tile) {
        const int len = min(tile, n - first);
        for (int i = tid; i < len; i += T) s_cell[i] = fit_prep_cell<DEG>(a, fit_prep_uv(f, tp[first + i]), s_ku, s_kv);
        __syncthreads();
        for (int c = tid; c < ncells; c += T) {
            int o = s_off[c];
            for (int i = 0; i < len; ++i)
                if (s_cell[i] == c) perm[o++] = first + i;
            s_off[c] = o;
        }
        __syncthreads();
    }
    for (int c = tid; c <= ncells; c += T) a.cell_start[(int64_t)b * (ncells + 1) + c] = s_start[c];
    __syncthreads();      // perm, written by other threads of this workgroup, is read below
    // the table rows, in sorted order
    float* tab = a.table + (int64_t)b * a.N * W;
    for (int j = tid; j < a.N; j += T) {
        float* rec = tab + (int64_t)j * W;
        if (j >= n) {
            perm[j] = -1;
            for (int k = 0; k < W; ++k) rec[k] = 0.0f;
            continue;
        }
        fit_prep_table_row<DEG>(a, f, tp[perm[j]], s_ku, s_kv, rec);
    }
}

bool fit_shape_ok(int64_t B, int64_t N, int64_t nu, int64_t nv, int p, int q)
{
    if (B < 0 || B > 2147483647LL || N < 1 || N > kFitMaxN) return false;
    if (p < 1 || q < 1 || p > kMaxDeg || q > kMaxDeg || nu <= p || nv <= q || nu > 4096 || nv > 4096) return false;
    if ((nu - p) * (nv - q) > kFitMaxCells) return false;
    return true;
}

}  // namespace
}  // namespace art

using namespace art;

// A launch with dynamic LDS: more than 64 KB of it has to be asked for.
template <typename... Params>
static int fit_launch(void (*kernel)(Params...), int64_t blocks, int block, size_t lds, hipStream_t stream, Params... args)
{
    ART_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(block), lds, stream, args...);
    ART_HIP(hipGetLastError());
    return ART_OK;
}

// The statement(s) after `deg` with DEG the kernels' instantiation for deg = fit_deg(p, q): 2, 3, or 0 (degrees read at run time).
#define ART_FIT_BY_DEGREE(deg, ...)                                                                                            \
    do {                                                                                                                       \
        if ((deg) == 2) { constexpr int DEG = 2; __VA_ARGS__; }                                                                \
        else if ((deg) == 3) { constexpr int DEG = 3; __VA_ARGS__; }                                                           \
        else { constexpr int DEG = 0; __VA_ARGS__; }                                                                           \
    } while (0)

// KERNEL<DEG, mode> of run / loss_grad
#define ART_FIT_BY_MODE(KERNEL, DEG, mode)                                                                                     \
    ((mode) == kFitLds ? KERNEL<DEG, kFitLds> : (mode) == kFitStream ? KERNEL<DEG, kFitStream> : KERNEL<DEG, kFitChunked>)

extern "C" int64_t art_surface_fit_table_words(int p, int q)
{
    if (p < 1 || q < 1 || p > kMaxDeg || q > kMaxDeg) return -1;
    const int deg = fit_deg(p, q);
    return 3 + 4 * ((deg > 0 ? deg : kMaxDeg) + 1);
}

extern "C" int art_surface_fit_prepare(const float* targets_points, const int32_t* n_valid, const float* knots_u,
                                       const float* knots_v, int64_t B, int64_t N, int64_t nu, int64_t nv, int p, int q,
                                       float* eval_uv, float* control_points, int32_t* perm, int32_t* cell_start, float* table,
                                       void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!fit_shape_ok(B, N, nu, nv, p, q)) return ART_EINVAL;
    if (B == 0) return ART_OK;
    if (!targets_points || !knots_u || !knots_v || !eval_uv || !control_points || !perm || !cell_start || !table) return ART_EINVAL;
    PrepArgs a;
    a.targets_points = targets_points; a.n_valid = n_valid; a.knots_u = knots_u; a.knots_v = knots_v;
    a.N = (int)N; a.nu = (int)nu; a.nv = (int)nv; a.p = p; a.q = q;
    a.eval_uv = eval_uv; a.cp = control_points; a.perm = perm; a.cell_start = cell_start; a.table = table;
    const int64_t ncells = (nu - p) * (nv - q);
    const int64_t small = (nu + p + 1) + (nv + q + 1) + 4 * (kFitPrepBlock / 64);       // knots and wave extrema
    const int knob = debug_env_int("ARTIST_HIP_FIT_CHUNK", 0);
    const int deg = fit_deg(p, q);
    size_t lds = sizeof(float) * (size_t)(2 * N + ncells + 1 + small);
    if (knob <= 0 && N <= kFitResidentMaxN && (int64_t)lds <= kFitLdsBudget) {
        ART_FIT_BY_DEGREE(deg, return fit_launch(surface_fit_prepare_kernel<DEG>, B, kFitPrepBlock, lds, stream, a));
    } else {
        // the rows in tiles: what stays in LDS is at most 2 * 4096 + 1 offsets and 2 * (4096 + 8) knots, so a tile always fits
        const int64_t fixed = 2 * ncells + 1 + small;
        int64_t tile = std::min<int64_t>(std::min<int64_t>(kFitPrepTile, (N + 63) / 64 * 64), (kFitLdsBudget / 4 - fixed) / 64 * 64);
        if (knob > 0) tile = std::min<int64_t>(tile, ((int64_t)knob + 63) / 64 * 64);
        if (tile < 64) return ART_EUNSUPPORTED;
        lds = sizeof(float) * (size_t)(tile + fixed);
        ART_FIT_BY_DEGREE(deg,
                          return fit_launch(surface_fit_prepare_tiled_kernel<DEG>, B, kFitPrepBlock, lds, stream, a, (int)tile));
    }
}

// Fills what loss_grad and run share; decides where the table lives and, when a facet's per-point arrays do not fit in LDS
// beside the net's block, the chunk length (kFitChunked: L is one chunk's layout); *block is the workgroup size.  Returns an
// error code.
static int fit_common(FitArgs& a, FitLayout& L, const float* targets, const int32_t* n_valid, const int32_t* perm,
                      const int32_t* cell_start, const float* table, int64_t B, int64_t N, int64_t nu, int64_t nv, int p, int q,
                      int method, int epochs, FitMode* mode, int* chunk, int* block)
{
    *chunk = 0;
    if (!fit_shape_ok(B, N, nu, nv, p, q) || (method != ART_FIT_POINTS && method != ART_FIT_NORMALS)) return ART_EINVAL;
    if (!targets || !perm || !cell_start || !table) return B == 0 ? ART_OK : ART_EINVAL;
    a = FitArgs{};
    a.N = (int)N; a.nu = (int)nu; a.nv = (int)nv; a.p = p; a.q = q; a.method = method;
    a.targets = targets; a.n_valid = n_valid; a.perm = perm; a.cell_start = cell_start; a.table = table;
    const int W = (int)art_surface_fit_table_words(p, q);
    const int64_t ncells = (nu - p) * (nv - q);
    // (sizes in 64 bits first: the layout itself counts in int)
    const int64_t net = 3 * epochs + 3 * nu * nv * 3 + ncells * (p + 1) * (q + 1) * 3 + ncells + 3;      // what no chunk shrinks
    const int64_t fixed = net + N * 7;
    const int knob = debug_env_int("ARTIST_HIP_FIT_CHUNK", 0);
    if (knob > 0 || N > kFitResidentMaxN || fixed * 4 > kFitLdsBudget) {
        // per position: its gradient w.r.t. S or dS/du, dS/dv and its squared error; C a multiple of 64 (the loss lanes)
        const int64_t per = (method == ART_FIT_POINTS ? 3 : 6) + 1;
        int64_t C = (kFitLdsBudget / 4 - net) / per / 64 * 64;
        if (net * 4 > kFitLdsBudget || C < 64) return ART_EUNSUPPORTED;
        C = std::min<int64_t>(C, (N + 63) / 64 * 64);
        if (knob > 0) C = std::min<int64_t>(C, ((int64_t)knob + 63) / 64 * 64);
        *mode = kFitChunked;
        *chunk = (int)C;
        *block = fit_block(std::min<int64_t>(N, C));
        L = fit_layout((int)C, (int)nu, (int)nv, p, q, method, W, epochs, false);
        if ((int64_t)L.total * 4 > kFitLdsBudget) return ART_EUNSUPPORTED;
        return ART_OK;
    }
    *mode = (fixed + N * (4 + W)) * 4 <= kFitLdsBudget && debug_env_int("ARTIST_HIP_FIT_STREAM", 0) == 0 ? kFitLds : kFitStream;
    *block = fit_block(N);
    L = fit_layout((int)N, (int)nu, (int)nv, p, q, method, W, epochs, *mode == kFitLds);
    if ((int64_t)L.total * 4 > kFitLdsBudget) return ART_EUNSUPPORTED;
    return ART_OK;
}

extern "C" int art_surface_fit_loss_grad(const float* control_points, const float* targets, const int32_t* n_valid,
                                         const int32_t* perm, const int32_t* cell_start, const float* table, int64_t B, int64_t N,
                                         int64_t nu, int64_t nv, int p, int q, int method, float* loss,
                                         float* grad_control_points, float* points_out, float* normals_out, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    FitArgs a;
    FitLayout L;
    FitMode mode = kFitLds;
    int chunk = 0, block = 0;
    const int rc = fit_common(a, L, targets, n_valid, perm, cell_start, table, B, N, nu, nv, p, q, method, 0, &mode, &chunk, &block);
    if (rc != ART_OK) return rc;
    if (B == 0) return ART_OK;
    if (!control_points || !loss || !grad_control_points || (points_out == nullptr) != (normals_out == nullptr)) return ART_EINVAL;
    a.cp_in = control_points; a.loss = loss; a.grad = grad_control_points;
    a.points_out = reinterpret_cast<float4*>(points_out); a.normals_out = reinterpret_cast<float4*>(normals_out);
    const size_t lds = (size_t)L.total * sizeof(float);
    ART_FIT_BY_DEGREE(fit_deg(p, q),
                      return fit_launch(ART_FIT_BY_MODE(surface_fit_loss_grad_kernel, DEG, mode), B, block, lds, stream, a, L, chunk));
}

extern "C" int art_surface_fit_run(float* control_points, float* exp_avg, float* exp_avg_sq, double* state_f64,
                                   int32_t* state_i32, float* last_loss, const float* targets, const int32_t* n_valid,
                                   const int32_t* perm, const int32_t* cell_start, const float* table, int64_t B, int64_t N,
                                   int64_t nu, int64_t nv, int p, int q, int method, int64_t epochs, double tolerance,
                                   int64_t max_epoch, double beta1, double beta2, double eps, double weight_decay, int maximize,
                                   int use_scheduler, int mode_max, double factor, int64_t patience, double threshold,
                                   int threshold_abs, int64_t cooldown, double min_lr, double scheduler_eps, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (epochs < 1 || epochs > kFitMaxEpochs || max_epoch < 0 || max_epoch > 2147483646LL || !(tolerance == tolerance) ||
        !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !(weight_decay == weight_decay))
        return ART_EINVAL;
    if (use_scheduler && (!(factor < 1.0) || patience < 0 || patience > 2147483646LL || cooldown < 0 || cooldown > 2147483646LL ||
                          !(threshold == threshold) || !(min_lr == min_lr) || !(scheduler_eps == scheduler_eps)))
        return ART_EINVAL;
    FitArgs a;
    FitLayout L;
    FitMode mode = kFitLds;
    int chunk = 0, block = 0;
    const int rc = fit_common(a, L, targets, n_valid, perm, cell_start, table, B, N, nu, nv, p, q, method, (int)epochs, &mode, &chunk, &block);
    if (rc != ART_OK) return rc;
    if (B == 0) return ART_OK;
    if (!control_points || !exp_avg || !exp_avg_sq || !state_f64 || !state_i32 || !last_loss) return ART_EINVAL;
    a.cp = control_points; a.m = exp_avg; a.v = exp_avg_sq; a.sf64 = state_f64; a.si32 = state_i32; a.last_loss = last_loss;
    a.epochs = (int)epochs; a.max_epoch = (int)max_epoch; a.tolerance = (float)tolerance;
    a.beta1 = (float)beta1; a.beta2 = (float)beta2;
    a.one_minus_beta1 = (float)(1.0 - beta1); a.one_minus_beta2 = (float)(1.0 - beta2);
    a.eps = (float)eps; a.weight_decay = (float)weight_decay; a.grad_sign = maximize ? -1.0f : 1.0f;
    a.beta1d = beta1; a.beta2d = beta2;
    a.sched = use_scheduler ? 1 : 0; a.mode_max = mode_max ? 1 : 0; a.thr_abs = threshold_abs ? 1 : 0;
    a.patience = (int)patience; a.cooldown = (int)cooldown;
    a.factor = factor; a.threshold = threshold; a.min_lr = min_lr; a.sched_eps = scheduler_eps;
    const size_t lds = (size_t)L.total * sizeof(float);
    ART_FIT_BY_DEGREE(fit_deg(p, q),
                      return fit_launch(ART_FIT_BY_MODE(surface_fit_run_kernel, DEG, mode), B, block, lds, stream, a, L, chunk));
}
