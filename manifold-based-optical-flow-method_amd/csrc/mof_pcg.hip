// mof_pcg.hip -- batched preconditioned CG on gfx950 (2x2 block Jacobi, or
// the aggregation-multigrid V-cycle of mof_amg.hip).
//
// Replaces scipy.sparse.linalg.spsolve (compute_optical_flow.py:147) for B
// timesteps at once: every launch covers all B systems, so the per-iteration
// launch cost is shared. A_b is materialised per system in SELL-64 2x2 blocks
// (16 B per block in fp32, read with one dwordx4 per lane, 1 KiB per
// wave-instruction). The SpMV grid is XCD-aware: each XCD owns one
// contiguous eighth of the vertex rows of every system and walks it row
// block by row block, a group of 8 systems of a row block back to back, so
// the row block's column indices are read once per XCD and group and a
// system's neighbour rows are still in L2 at its next row block
// (mof_rowkern.h).
//
// The fp64 residual of the refinement (k_residual) applies A without the
// materialised blocks: lambda a2 (shared SELL blocks) plus a1 per incident
// triangle from the 6 values u_T of each triangle (a1 restricted to a
// triangle is u u^T (x) [A/6 on the diagonal, A/12 off it],
// compute_optical_flow.py:127-141):
//   (a1 x)_i = sum_{T ni i} u_{T,i} (A_T/12) (2 s_i + s_j + s_k),  s_v = u_{T,v} . x_v
//
// One CG iteration = two launches (+ the V-cycle with MOF_PRECOND_AMG):
//   k_pcg_spmv    w = A z ; q = w + beta q ; p = z + beta p ; partial p.q
//                 (q = A p without a separate p update: A(z + beta p) =
//                  A z + beta A p)
//   k_pcg_update  x += alpha p ; r -= alpha q ; z = D^-1 r ; partial r.z, r.r
//                 (multigrid: x0 = omega D^-1 r, the V-cycle's pre-smoothing,
//                  and partial r.r; the V-cycle's last kernel writes z, r.z)
// Scalars (alpha, beta, |r|) are never sent to the host: every workgroup
// re-reduces the per-workgroup partials of the previous launch in one fixed
// order, so all workgroups (and every run, on any GPU count) agree bit for
// bit. Convergence is checked on the device; the host polls a flag word every
// few iterations.
//
// MOF_PREC_MIXED: the inner CG runs on fp32 A and fp32 vectors (dot products
// in fp64) for the correction d of A d = r64, and the fp64 matrix-free
// residual refreshes r64 = f - A x64 between inner solves (iterative
// refinement).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cmath>
#include <memory>

#include <hip/hip_ext.h>

#include "mof_dd.h"
#include "mof_internal.h"
#include "mof_rowkern.h"
#include "mof_staged.h"

namespace mof {

thread_local double g_fetch_ms = 0.0;
thread_local int64_t g_fetch_n = 0;

// launches so far of each inner-PCG kernel instance (mof_test_pcg_launches):
// k_pcg_spmv<V, FIRST, ZH, PK> at (V == double) * 8 + FIRST * 4 + ZH * 2 + PK, then the rest;
// kPcCompact: the times pcg() switched its launches to a compacted system map
enum { kPcRedPq = 16, kPcRedRzrr, kPcUpdate, kPcConvEarly, kPcOuterUpdate, kPcOuterCheck, kPcCompact, kPcKernels };
std::atomic<int64_t> g_pcg_launches[kPcKernels];

namespace {

template <typename V>
struct PcgArgs {
    int32_t N, nblk, B;
    MatArgs<V> mat;
    const V *dinv;   // [B][N][4]
    V *x, *r, *z, *p, *q;  // [B][N][2]
    double *part_pq;       // [2][P][B][nmax] by iteration parity (single domain: P = 1, nmax = nblk)
    double *part_rzrr;     // [2][P][B][nmax][2]
    double *sysd;          // [B][8]
    int32_t *sysi;         // [B][8]
    int32_t ext;           // z and r.z come from an external preconditioner (AMG)
    V *x0;                 // ext: pre-smoothed x0 = omega D^-1 r for the V-cycle
    V omega;
    const uint2 *dA;       // ext (multigrid, fp32): the smoother's bf16 operator (its diagonal
                           // blocks give D for the pre-smoothing)
    int64_t dA_nb;
    const int32_t *dA_off;
    RedArgs red;           // partial-record layout; rows >= red.nown (ghosts) are not summed
    int32_t stall;         // stagnation window in iterations (0: off)
    double *sc;            // pre-reduced scalars (k_red_rzrr / k_red_pq), by iteration parity
    int32_t zh;            // z stored as bf16 pairs: the multigrid cycle's output on a single
                           // domain with the tentative prolongator (the decomposed path's
                           // halo exchange moves float2 z)
    SysMap sm;             // the systems the per-iteration launches cover (SysMap)
    int32_t selfred;       // small meshes: the SpMV and the update reduce the partial records
                           // they need themselves (no k_red_pq / k_red_rzrr launches)
};

// The per-system scalars every workgroup of the next launch needs, reduced
// once by one workgroup per system (the same order as reduce_sys, so the
// same bits) instead of by every workgroup from the partial records: r.z and
// |r|^2 at sc[(slot B + b) 2 + k], p.q at sc[4 B + slot B + b].
__device__ __forceinline__ double *sc_rzrr(double *sc, int32_t B, int32_t slot, int32_t b) {
    return sc + 2 * ((int64_t)slot * B + b);
}
__device__ __forceinline__ double *sc_pq(double *sc, int32_t B, int32_t slot, int32_t b) {
    return sc + 4 * (int64_t)B + (int64_t)slot * B + b;
}

// |r|^2 growth over the start of the inner solve taken as divergence (CG's
// residual is not monotone, but 1e5 in norm is far past any transient)
constexpr double kDiverge = 1e10;

// Safety factor on the refinement's error estimate (outer_check_sys): the
// estimate E was 0.5-1.8x the true max|V - V*| after the second step
// (tools/error_control_study.py).
constexpr double kErrSafety = 2.0;

// Record of (this part, system b, workgroup w) in a partial array.
__device__ __forceinline__ int64_t red_rec(const RedArgs &rd, int32_t B, int32_t b, int32_t w) {
    return ((int64_t)rd.part * B + b) * rd.nmax + w;
}

// Sum over all parts' partial records of system b, in one fixed order (part,
// then workgroup), so every part of a decomposed solve gets the same bits.
template <int NV, int NT = kWG>
__device__ __forceinline__ void reduce_sys(const double *slot, const RedArgs &rd, int32_t B, int32_t b,
                                           double (&out)[NV], double *lds) {
    if (rd.P == 1) {
        reduce_partials<NV, NT>(slot + (int64_t)NV * b * rd.nmax, rd.nmax, out, lds);
        return;
    }
#pragma unroll
    for (int k = 0; k < NV; ++k) out[k] = 0.0;
    for (int32_t q = 0; q < rd.P; ++q) {
        const double *p = slot + (int64_t)NV * ((int64_t)q * B + b) * rd.nmax;
        for (int32_t w = threadIdx.x < kWG ? (int32_t)threadIdx.x : rd.nmax; w < rd.nmax; w += kWG)
#pragma unroll
            for (int k = 0; k < NV; ++k) out[k] += p[(int64_t)w * NV + k];
    }
    block_sum<NV, NT>(out, lds);
}

// slots / incident triangles per load batch of the residual rows
// kRcU: incident triangles per load batch of the re-forming residual; 1
// instead of 2 (round 3): 126 instead of 202 VGPRs, 4 instead of 2 waves
// per SIMD, 5.73 -> 5.42 ms per 512-system launch (profiles/r03_ab/grp/)
constexpr int kResU = 4, kRcU = 1;
// incidence entries of a row preloaded by the re-forming residual (slices up
// to this wide; wider slices load them one at a time): 162 VGPRs and 3 waves instead of 128 and 4, the
// chains one round trip shorter -- 10.70 -> 10.61 ms per 1024-system launch,
// C3 +0.25 % (round 4, profiles/r04_ab/res_pre/: the lost wave eats most of
// the shorter chain)
constexpr int kRcPre = 8;
// y_i = (A_b x)_i for vertex row i of system b without materialised blocks
// (lambda a2 + per-triangle a1; x = that system's vector). Loads are batched
// U slots / incident triangles at a time as in spmv_row.
template <typename V>
__device__ __forceinline__ void apply_row_mf(const OpArgs<V> &op, int32_t b, int32_t i,
                                             const V *__restrict__ x, double &y0, double &y1) {
    using V2 = typename VT<V>::V2;
    constexpr int U = kResU;
    const int32_t s = i >> 6, l = i & 63;
    V a0 = 0, a1 = 0;
    // lambda a2 x
    {
        const int32_t o = op.sell_off[s];
        const int32_t w = (op.sell_off[s + 1] - o) >> 6;
        for (int32_t t0 = 0; t0 < w; t0 += U) {
            int32_t j[U];
            V blk[U][4];
#pragma unroll
            for (int u = 0; u < U; ++u) j[u] = op.sell_col[(int64_t)o + min(t0 + u, w - 1) * kSlice + l];
#pragma unroll
            for (int u = 0; u < U; ++u) ld_blk(op.a2s, (int64_t)o + min(t0 + u, w - 1) * kSlice + l, blk[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const V2 xj = ld2(x + 2 * (int64_t)j[u]);
                const bool on = t0 + u < w;
                a0 += on ? blk[u][0] * xj.x + blk[u][1] * xj.y : (V)0;
                a1 += on ? blk[u][2] * xj.x + blk[u][3] * xj.y : (V)0;
            }
        }
    }
    // a1_b x, per incident triangle (padding entries point at the zero slot M)
    {
        const V *ub = op.u + 6 * (int64_t)b * (op.M + 1);
        const V2 xi = ld2(x + 2 * (int64_t)i);
        const int32_t o = op.tsell_off[s];
        const int32_t w = (op.tsell_off[s + 1] - o) >> 6;
        for (int32_t t0 = 0; t0 < w; t0 += U) {
            int4 q[U];
#pragma unroll
            for (int u = 0; u < U; ++u) q[u] = op.tinc[(int64_t)o + min(t0 + u, w - 1) * kSlice + l];
            V2 P0[U], P1[U], P2[U], xj[U], xk[U];
            V w12[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const V *uT = ub + 6 * (int64_t)q[u].x;
                P0[u] = ld2(uT);
                P1[u] = ld2(uT + 2);
                P2[u] = ld2(uT + 4);
                xj[u] = ld2(x + 2 * (int64_t)q[u].z);
                xk[u] = ld2(x + 2 * (int64_t)q[u].w);
                w12[u] = op.w12[q[u].x];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int c = q[u].y;
                const V2 ui = c == 0 ? P0[u] : (c == 1 ? P1[u] : P2[u]);
                const V2 uj = c == 0 ? P1[u] : (c == 1 ? P2[u] : P0[u]);
                const V2 uk = c == 0 ? P2[u] : (c == 1 ? P0[u] : P1[u]);
                const V si = ui.x * xi.x + ui.y * xi.y;
                const V sj = uj.x * xj[u].x + uj.y * xj[u].y;
                const V sk = uk.x * xk[u].x + uk.y * xk[u].y;
                const V cc = (t0 + u < w) ? w12[u] * ((si + si) + sj + sk) : (V)0;
                a0 += ui.x * cc;
                a1 += ui.y * cc;
            }
        }
    }
    y0 = a0;
    y1 = a1;
}

// (a1_b x)_i of two systems at once with u re-formed per incident triangle
// from each system's I row and the mesh geometry, in k_tri_step's exact
// arithmetic (grad I without contraction, np.dot's fma chain), so r64 keeps
// its bits while the 15.7 MB/system u64 array is neither written nor
// gathered three times (once per incident row block); lambda a2 x as
// apply_row_mf. One system per thread was bound by the shared gathers (8.93
// vs 6.72 ms per 512-system launch, round 2).
__device__ __forceinline__ double dot3_np(const double *x, const double *y) {
    return fma(x[2], y[2], fma(x[1], y[1], __dmul_rn(x[0], y[0])));
}

// The re-forming residual's row pieces for NS systems of the batch at once:
// every a2 block and incident triangle's geometry is loaded once for all of
// them (the residual is bound by those shared gathers). No fp contraction, so
// every system slot rounds alike (a system's bits must not depend on the slot
// it lands in, i.e. on the batch split).
// One a2 slot's term of one system (shared by the row and the staged kernel).
__device__ __forceinline__ void rcn_a2_term(const double (&blk)[4], double2 xj, bool on, double (&acc)[2]) {
#pragma clang fp contract(off)
    acc[0] += on ? blk[0] * xj.x + blk[1] * xj.y : 0.0;
    acc[1] += on ? blk[2] * xj.x + blk[3] * xj.y : 0.0;
}
// rcn_a2: acc += (lambda a2 x)_i, slots in order, kResU per load batch.
template <int NS>
__device__ __forceinline__ void rcn_a2(const OpArgs<double> &op, const int32_t (&bs)[NS], int32_t i,
                                       const double *__restrict__ x64, double (&acc)[NS][2]) {
#pragma clang fp contract(off)
    const int32_t s = i >> 6, l = i & 63;
    const int32_t o = op.sell_off[s];
    const int32_t w = (op.sell_off[s + 1] - o) >> 6;
    for (int32_t t0 = 0; t0 < w; t0 += kResU) {
        int32_t j[kResU];
        double blk[kResU][4];
#pragma unroll
        for (int u = 0; u < kResU; ++u) j[u] = op.sell_col[(int64_t)o + min(t0 + u, w - 1) * kSlice + l];
#pragma unroll
        for (int u = 0; u < kResU; ++u) ld_blk(op.a2s, (int64_t)o + min(t0 + u, w - 1) * kSlice + l, blk[u]);
#pragma unroll
        for (int u = 0; u < kResU; ++u) {
            const bool on = t0 + u < w;
#pragma unroll
            for (int t = 0; t < NS; ++t)
                rcn_a2_term(blk[u], ld2(x64 + 2 * ((int64_t)bs[t] * op.N + j[u])), on, acc[t]);
        }
    }
}
// The row's own data the incidence terms need.
template <int NS>
struct RcnRow {
    double2 xi[NS];
    double Ii[NS];
    double ei[6];
};
template <int NS>
__device__ __forceinline__ void rcn_row(const OpArgs<double> &op, const int32_t (&bs)[NS], int32_t i,
                                        const double *__restrict__ x64, RcnRow<NS> &R) {
#pragma unroll
    for (int t = 0; t < NS; ++t) {
        R.xi[t] = ld2(x64 + 2 * ((int64_t)bs[t] * op.N + i));
        R.Ii[t] = op.I0[(int64_t)bs[t] * op.ldI + i];
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) R.ei[q] = op.e[6 * (int64_t)i + q];
}
// One incidence's term of one system from its operands (shared by the row
// and the staged kernel): corner c of the triangle, its hat gradients g, the
// tangent bases of the row and of the corner's two other vertices, A_T / 12,
// and the system's I values and x at the three vertices.
__device__ __forceinline__ void rcn_tri_term(int c, const double (&g)[9], const double (&ei)[6],
                                             const double (&ej)[6], const double (&ek)[6], double wt, double Ii,
                                             double Ij, double Ik, double2 xi, double2 xj, double2 xk,
                                             double (&val)[2]) {
#pragma clang fp contract(off)
    const double c0 = c == 0 ? Ii : (c == 1 ? Ik : Ij);
    const double c1 = c == 0 ? Ij : (c == 1 ? Ii : Ik);
    const double c2 = c == 0 ? Ik : (c == 1 ? Ij : Ii);
    double gI[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) gI[d] = (c0 * g[d] + c1 * g[3 + d]) + c2 * g[6 + d];
    const double2 ui = make_double2(dot3_np(gI, ei), dot3_np(gI, ei + 3));
    const double2 uj = make_double2(dot3_np(gI, ej), dot3_np(gI, ej + 3));
    const double2 uk = make_double2(dot3_np(gI, ek), dot3_np(gI, ek + 3));
    const double si = ui.x * xi.x + ui.y * xi.y;
    const double sj = uj.x * xj.x + uj.y * xj.y;
    const double sk = uk.x * xk.x + uk.y * xk.y;
    const double cc = wt * ((si + si) + sj + sk);
    val[0] = ui.x * cc;
    val[1] = ui.y * cc;
}
// rcn_tri: the term of incidence q (triangle, corner, the corner's two other
// vertices) of row i, (a1_T x)_i = u_{T,i} (A_T/12) (2 s_i + s_j + s_k) with
// u re-formed from the I row in k_tri_step's exact arithmetic (grad I
// without contraction, np.dot's fma chain); padding entries (T = M) have
// weight 0.
template <int NS>
__device__ __forceinline__ void rcn_tri(const OpArgs<double> &op, const int32_t (&bs)[NS], int4 q,
                                        const double *__restrict__ x64, const RcnRow<NS> &R,
                                        double (&val)[NS][2]) {
#pragma clang fp contract(off)
    double g[9], ej[6], ek[6], Ij[NS], Ik[NS], wt;
    double2 xj[NS], xk[NS];
    const int64_t T = min(q.x, op.M - 1);
#pragma unroll
    for (int k = 0; k < 9; ++k) g[k] = op.gw[9 * T + k];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        ej[k] = op.e[6 * (int64_t)q.z + k];
        ek[k] = op.e[6 * (int64_t)q.w + k];
    }
#pragma unroll
    for (int t = 0; t < NS; ++t) {
        const double *Ib = op.I0 + (int64_t)bs[t] * op.ldI;
        const int64_t vb = (int64_t)bs[t] * op.N;
        Ij[t] = Ib[q.z];
        Ik[t] = Ib[q.w];
        xj[t] = ld2(x64 + 2 * (vb + q.z));
        xk[t] = ld2(x64 + 2 * (vb + q.w));
    }
    wt = op.w12[q.x];
#pragma unroll
    for (int t = 0; t < NS; ++t) rcn_tri_term(q.y, g, R.ei, ej, ek, wt, R.Ii[t], Ij[t], Ik[t], R.xi[t], xj[t], xk[t], val[t]);
}

// (A x)_i of NS systems: the a2 slots, then the incident triangles in
// triangle order, one incidence per load batch (kRcU = 1).
template <int NS>
__device__ __forceinline__ void apply_row_rcn(const OpArgs<double> &op, const int32_t (&bs)[NS], int32_t i,
                                              const double *__restrict__ x64, double (&y)[NS][2]) {
#pragma clang fp contract(off)
    static_assert(kRcU == 1, "one incidence per load batch");
    const int32_t s = i >> 6, l = i & 63;
    double acc[NS][2];
#pragma unroll
    for (int t = 0; t < NS; ++t) acc[t][0] = acc[t][1] = 0.0;
    rcn_a2<NS>(op, bs, i, x64, acc);
    RcnRow<NS> R;
    rcn_row<NS>(op, bs, i, x64, R);
    const int32_t o = op.tsell_off[s];
    const int32_t w = (op.tsell_off[s + 1] - o) >> 6;
    if (kRcPre && w <= kRcPre) {
        // the row's incidence entries loaded up front: each incident
        // triangle's geometry and per-system gathers then wait on one round
        // trip, not on its entry first (the same terms in the same order)
        constexpr int P = kRcPre > 0 ? kRcPre : 1;
        int4 qs[P];
#pragma unroll
        for (int t0 = 0; t0 < P; ++t0)
            if (t0 < w) qs[t0] = op.tinc[(int64_t)o + t0 * kSlice + l];
#pragma unroll
        for (int t0 = 0; t0 < P; ++t0) {
            if (t0 >= w) break;
            double val[NS][2];
            rcn_tri<NS>(op, bs, qs[t0], x64, R, val);
#pragma unroll
            for (int t = 0; t < NS; ++t) {
                acc[t][0] += val[t][0];
                acc[t][1] += val[t][1];
            }
        }
    } else {
        for (int32_t t0 = 0; t0 < w; ++t0) {
            double val[NS][2];
            rcn_tri<NS>(op, bs, op.tinc[(int64_t)o + t0 * kSlice + l], x64, R, val);
#pragma unroll
            for (int t = 0; t < NS; ++t) {
                acc[t][0] += val[t][0];
                acc[t][1] += val[t][1];
            }
        }
    }
#pragma unroll
    for (int t = 0; t < NS; ++t) {
        y[t][0] = acc[t][0];
        y[t][1] = acc[t][1];
    }
}

constexpr int kForce = 1;  // bench: ignore convergence / activity flags


// The row kernels' bodies take their (row block, system) as arguments: the
// __global__ wrappers map blockIdx to them, and the fused small-mesh solve
// (k_solve_fused) runs the same bodies over every row block of its system in
// one workgroup -- the same arithmetic in the same order, so the same bits.
template <typename V, int NQ = 1>
__device__ __forceinline__ void pcg_init_rows(const PcgArgs<V> &a, const double *__restrict__ rhs, int32_t rb,
                                              int32_t b) {
    __shared__ double lds[8 * NQ];
    const int32_t tid = row_tid();
    if (!a.sysi[b * kSysStride + SI_ACTIVE]) return;
    using V2 = typename VT<V>::V2;
    double rz = 0.0, rr = 0.0;
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const int32_t i = rb * kRowsPerWG + r * kWG + tid;
        if (i >= a.N) break;
        const int64_t vi = (int64_t)b * a.N + i;
        const double2 f = *reinterpret_cast<const double2 *>(rhs + 2 * vi);
        // a decomposed part's ghost rows carry r = 0 (the multigrid cycle
        // reads every local row; the CG sums skip them anyway)
        const bool own = i < a.red.nown;
        const V r0 = own ? (V)f.x : (V)0, r1 = own ? (V)f.y : (V)0;
        *reinterpret_cast<V2 *>(a.r + 2 * vi) = V2{r0, r1};
        *reinterpret_cast<V2 *>(a.x + 2 * vi) = V2{(V)0, (V)0};
        if (!a.ext) {
            const V *d = a.dinv + 4 * vi;
            const V z0 = d[0] * r0 + d[1] * r1, z1 = d[2] * r0 + d[3] * r1;
            *reinterpret_cast<V2 *>(a.z + 2 * vi) = V2{z0, z1};
            if (i < a.red.nown) rz += (double)r0 * z0 + (double)r1 * z1;  // ghost rows: never summed
        } else if constexpr (sizeof(V) == 4) {
            // the smoother's D^-1 (bf16), as in every later sweep
            const float2 d = bf16_diag_solve(bf16_diag_block(a.dA, a.dA_nb, a.dA_off, b, i), r0, r1);
            st_x0(a.x0, vi, a.omega * d.x, a.omega * d.y);
        }
        if (i < a.red.nown) rr += (double)r0 * r0 + (double)r1 * r1;
    }
    double v[2] = {rz, rr};
    block_sum_q<2, NQ>(v, lds);
    if (tid == 0 && rb < a.nblk) {
        double *o = a.part_rzrr + 2 * red_rec(a.red, a.B, b, rb);  // slot 0
        o[0] = v[0];
        o[1] = v[1];
    }
}
template <typename V>
__global__ __launch_bounds__(kWG) void k_pcg_init(PcgArgs<V> a, const double *__restrict__ rhs) {
    pcg_init_rows<V>(a, rhs, blockIdx.x, blockIdx.y);
}

// The scalars of the PCG recurrences are reduced once per system
// (k_red_rzrr after the update / V-cycle, k_red_pq after the SpMV) and the
// row kernels read two doubles instead of re-reducing every workgroup's
// partial record -- which is what lets the row kernels use small (256-row)
// workgroups.
template <typename V, int NT = kWG>
__device__ __forceinline__ void red_rzrr_sys(const PcgArgs<V> &a, int32_t slot, int32_t b) {
    __shared__ double lds[2 * (NT / 64)];
    const int64_t ps = (int64_t)a.red.P * a.B * a.red.nmax * 2;
    double v[2];
    reduce_sys<2, NT>(a.part_rzrr + slot * ps, a.red, a.B, b, v, lds);
    if (threadIdx.x == 0) {
        double *o = sc_rzrr(a.sc, a.B, slot, b);
        o[0] = v[0];
        o[1] = v[1];
    }
}
template <typename V>
__global__ __launch_bounds__(kWG) void k_red_rzrr(PcgArgs<V> a, int32_t slot) {
    red_rzrr_sys<V>(a, slot, sm_b(a.sm, blockIdx.x));
}
template <typename V, int NT = kWG>
__device__ __forceinline__ void red_pq_sys(const PcgArgs<V> &a, int32_t slot, int32_t b) {
    __shared__ double lds[NT / 64];
    const int64_t pqs = (int64_t)a.red.P * a.B * a.red.nmax;
    double v[1];
    reduce_sys<1, NT>(a.part_pq + slot * pqs, a.red, a.B, b, v, lds);
    if (threadIdx.x == 0) *sc_pq(a.sc, a.B, slot, b) = v[0];
}
template <typename V>
__global__ __launch_bounds__(kWG) void k_red_pq(PcgArgs<V> a, int32_t slot) {
    red_pq_sys<V>(a, slot, sm_b(a.sm, blockIdx.x));
}

// One workgroup per system, between the update and the V-cycle: |r|^2 of the
// update's partials (the same records and reduction as k_red_rzrr's, so the
// same bits as the next SpMV's test) against the tolerance; a converged
// system gets SI_CONV = it + 1 now, the value that SpMV would write, and the
// V-cycle's kernels skip it -- its z was never used: the next SpMV only
// applies the deferred x update (round 5: one V-cycle per system and inner
// solve saved, and the batch's last iteration is an SpMV launch alone: C3
// 3689 -> 3845 / 3876, S1 1080 -> 1121, F3 2485 -> 2582 timesteps/s, same
// bits; profiles/r05_ab/conv_early/).
template <typename V>
__global__ __launch_bounds__(kWG) void k_pcg_conv_early(PcgArgs<V> a, int32_t it) {
    __shared__ double lds[2 * (kWG / 64)];
    const int32_t b = sm_b(a.sm, blockIdx.x);
    int32_t *si = a.sysi + b * kSysStride;
    if (!si[SI_ACTIVE] || si[SI_CONV] >= 0 || si[SI_FAILED]) return;
    const int64_t ps = (int64_t)a.red.P * a.B * a.red.nmax * 2;
    double v[2];
    reduce_sys<2, kWG>(a.part_rzrr + ((it + 1) & 1) * ps, a.red, a.B, b, v, lds);
    if (threadIdx.x == 0 && v[1] <= a.sysd[b * kSysStride + SD_TOL2]) si[SI_CONV] = it + 1;
}

// One workgroup per system: tolerance from |rhs|^2, reset the convergence word.
// outer_rtol > 0 (refinement steps after the first): each system's inner
// tolerance is what its own outer residual still needs, 0.3 rtol |f| / |r64|,
// kept within [rtol, 0.5] -- a system 3x above the outer target (R3 after two
// steps: the fp32 operator's rounding limits a step to ~3e-4 there) takes a
// short inner solve, not a full 1e-4 one. etol > 0 (error control): no
// looser than the error estimate of the last step still needs,
// 0.5 etol max|x64| / (kErrSafety E) -- a step that ends the residual's need
// but not the error's gets the reduction the error is short of.
template <typename V, int NT = kWG>
__device__ __forceinline__ void pcg_tol_sys(const PcgArgs<V> &a, double rtol, double outer_rtol, double etol,
                                            int32_t b) {
    __shared__ double lds[2 * (NT / 64)];
    int32_t *si = a.sysi + b * kSysStride;
    if (!si[SI_ACTIVE]) {
        if (threadIdx.x == 0) si[SI_CONV] = 0;
        return;
    }
    double v[2];
    reduce_sys<2, NT>(a.part_rzrr, a.red, a.B, b, v, lds);
    if (threadIdx.x == 0) {
        double t = rtol;
        if (outer_rtol > 0.0) {
            const double ff = a.sysd[b * kSysStride + SD_FF], rr = a.sysd[b * kSysStride + SD_RR];
            if (ff > 0.0 && rr > 0.0) {
                double need = 0.3 * outer_rtol * sqrt(ff / rr);
                const double est = a.sysd[b * kSysStride + SD_EST];
                if (etol > 0.0 && est > 0.0)
                    need = fmin(need, 0.5 * etol * a.sysd[b * kSysStride + SD_XMAX] / (kErrSafety * est));
                t = fmax(rtol, fmin(0.5, need));
            }
        }
        a.sysd[b * kSysStride + SD_TOL2] = t * t * v[1];
        a.sysd[b * kSysStride + SD_RR0] = v[1];
        a.sysd[b * kSysStride + SD_BEST] = v[1];
        si[SI_BEST_IT] = 0;
        si[SI_CONV] = -1;
    }
}
template <typename V>
__global__ __launch_bounds__(kWG) void k_pcg_tol(PcgArgs<V> a, double rtol, double outer_rtol, double etol) {
    pcg_tol_sys<V>(a, rtol, outer_rtol, etol, blockIdx.x);
}

// PK: the packed index words (mof_rowkern.h kIxPack; fp32 only) instead of
// the run-time choice between the plain and the mirrored 32-bit tables
template <typename V, bool FIRST, bool ZH = false, int NQ = 1, bool PK = false>
__device__ __forceinline__ void pcg_spmv_rows(const PcgArgs<V> &a, int32_t it, int32_t flags, int32_t rb, int32_t b) {
    constexpr int NT = kWG, RPT = kRows;  // rows per thread
    __shared__ double lds[NQ * (NT / 64)];
    const int32_t tid = row_tid();
    const bool force = flags & kForce;
    // retired systems: inactive, or converged in an earlier iteration (the
    // word is sticky, so no later launch re-reads a stale partial slot)
    // (a system that converges in this launch still finishes it: the deferred
    // x update below)
    const int32_t conv = a.sysi[b * kSysStride + SI_CONV];
    if (!force && (!a.sysi[b * kSysStride + SI_ACTIVE] || (conv >= 0 && conv != it))) return;
    const int64_t pqs = (int64_t)a.red.P * a.B * a.red.nmax;  // p.q slot stride
    using V2 = typename VT<V>::V2;
    const int64_t vb = (int64_t)b * a.N;
    double cur[2];
    // The previous iteration's x += alpha p, deferred to here: this launch
    // reads p anyway (p = z + beta p), so the update kernel reads neither p
    // nor x. alpha is the update's own value (same partials, same order).
    V alpha_prev = 0;
    double old[2] = {1.0, 1.0};  // the previous iteration's r.z, |r|^2
    bool self = false;
    if constexpr (NQ == 1) self = a.selfred != 0;
    if (self) {
        // the same reductions as k_red_rzrr / k_red_pq (reduce_sys), in every
        // workgroup of the system: the same bits, two launches fewer
        __shared__ double lds2[2 * (NT / 64)];
        const int64_t ps = (int64_t)a.red.P * a.B * a.red.nmax * 2;
        reduce_sys<2, NT>(a.part_rzrr + (it & 1) * ps, a.red, a.B, b, cur, lds2);
        if (!FIRST) {
            double pq1[1];
            reduce_sys<2, NT>(a.part_rzrr + ((it + 1) & 1) * ps, a.red, a.B, b, old, lds2);
            reduce_sys<1, NT>(a.part_pq + ((it + 1) & 1) * pqs, a.red, a.B, b, pq1, lds2);
            if (!force) alpha_prev = (V)(old[0] / pq1[0]);
        }
    } else {
        const double *c = sc_rzrr(a.sc, a.B, it & 1, b);
        cur[0] = c[0];
        cur[1] = c[1];
        if (!FIRST) {
            const double *o = sc_rzrr(a.sc, a.B, (it + 1) & 1, b);
            old[0] = o[0];
            old[1] = o[1];
            if (!force) alpha_prev = (V)(old[0] / *sc_pq(a.sc, a.B, (it + 1) & 1, b));
        }
    }
    if (!force && cur[1] <= a.sysd[b * kSysStride + SD_TOL2]) {
        if (!FIRST) {
#pragma unroll
            for (int r = 0; r < RPT; ++r) {
                const int32_t i = rb * kRowsPerWG + r * NT + tid;
                if (i >= a.N) break;
                const int64_t vi = vb + i;
                const V2 p0 = *reinterpret_cast<const V2 *>(a.p + 2 * vi);
                V2 xi = *reinterpret_cast<const V2 *>(a.x + 2 * vi);
                xi.x += alpha_prev * p0.x;
                xi.y += alpha_prev * p0.y;
                *reinterpret_cast<V2 *>(a.x + 2 * vi) = xi;
            }
        }
        if (rb == 0 && tid == 0 && a.sysi[b * kSysStride + SI_CONV] < 0)
            a.sysi[b * kSysStride + SI_CONV] = it;
        return;
    }
    // stagnation bookkeeping: one thread of the system's first row block (no
    // other workgroup reads these slots; k_pcg_update reads them next launch)
    if (!force && rb == 0 && tid == 0 && cur[1] < a.sysd[b * kSysStride + SD_BEST]) {
        a.sysd[b * kSysStride + SD_BEST] = cur[1];
        a.sysi[b * kSysStride + SI_BEST_IT] = it;
    }
    V beta = 0;
    if (!FIRST) beta = (V)(cur[0] / old[0]);
    double pq = 0.0;
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const int32_t i = rb * kRowsPerWG + r * NT + tid;
        if (i >= a.N) break;
        V y0, y1;
        const int64_t vi = vb + i;
        V2 zi;
        const V *zb = ZH ? reinterpret_cast<const V *>(reinterpret_cast<const uint32_t *>(a.z) + vb) : a.z + 2 * vb;
        if constexpr (PK)
            spmv_row_t<kIxPack, V, ZH>(a.mat, b, i, zb, y0, y1);
        else
            spmv_row<V, ZH>(a.mat, b, i, zb, y0, y1);
        if constexpr (ZH) {
            const uint32_t h = reinterpret_cast<const uint32_t *>(a.z)[vi];
            zi = V2{bf16_lo(h), bf16_hi(h)};
        } else {
            zi = *reinterpret_cast<const V2 *>(a.z + 2 * vi);
        }
        V2 qi, pi;
        if (FIRST) {
            qi = V2{y0, y1};
            pi = zi;
        } else {
            const V2 q0 = *reinterpret_cast<const V2 *>(a.q + 2 * vi);
            const V2 p0 = *reinterpret_cast<const V2 *>(a.p + 2 * vi);
            if constexpr (PK) {
                // Contraction of these updates is the code generator's choice
                // in the 32-bit instances, and it depends on the row product
                // before them: p and x fused, q = y + beta q fused with an
                // fp32 z and left as a product and a sum with a bf16 z (gfx950
                // ISA of k_pcg_spmv<float, false, ZH>). The packed instances
                // state that rounding, so a system's bits do not depend on its
                // index source (tests/test_gpu_index_word.py).
#pragma clang fp contract(off)
                if constexpr (ZH)
                    qi = V2{y0 + beta * q0.x, y1 + beta * q0.y};
                else
                    qi = V2{fmaf(beta, q0.x, y0), fmaf(beta, q0.y, y1)};
                pi = V2{fmaf(beta, p0.x, zi.x), fmaf(beta, p0.y, zi.y)};
                if (!force) {
                    V2 xi = *reinterpret_cast<const V2 *>(a.x + 2 * vi);
                    xi.x = fmaf(alpha_prev, p0.x, xi.x);
                    xi.y = fmaf(alpha_prev, p0.y, xi.y);
                    *reinterpret_cast<V2 *>(a.x + 2 * vi) = xi;
                }
            } else {
                qi = V2{y0 + beta * q0.x, y1 + beta * q0.y};
                pi = V2{zi.x + beta * p0.x, zi.y + beta * p0.y};
                if (!force) {
                    V2 xi = *reinterpret_cast<const V2 *>(a.x + 2 * vi);
                    xi.x += alpha_prev * p0.x;
                    xi.y += alpha_prev * p0.y;
                    *reinterpret_cast<V2 *>(a.x + 2 * vi) = xi;
                }
            }
        }
        *reinterpret_cast<V2 *>(a.q + 2 * vi) = qi;
        *reinterpret_cast<V2 *>(a.p + 2 * vi) = pi;
        if (i < a.red.nown) pq += (double)pi.x * qi.x + (double)pi.y * qi.y;
    }
    double v[1] = {pq};
    block_sum_q<1, NQ>(v, lds);
    if (tid == 0 && rb < a.nblk) a.part_pq[(it & 1) * pqs + red_rec(a.red, a.B, b, rb)] = v[0];
}
template <typename V, bool FIRST, bool ZH = false, bool PK = false>
__device__ __forceinline__ void pcg_spmv_body(const PcgArgs<V> &a, int32_t it, int32_t flags) {
    int32_t rb, bl;
    if (!xcd_map(a.nblk, a.sm.n, rb, bl, kGrpSpmv)) return;
    pcg_spmv_rows<V, FIRST, ZH, 1, PK>(a, it, flags, rb, sm_b(a.sm, bl));
}

// Measured and not kept (round 2, profiles/r02_ab/spmvns_*): two systems
// per thread sharing each slot's column index and mirror entry -- the main
// launch took the same time (1624.8 vs 1625.5 us at C3, B = 512: bound by
// its bytes, not by the index loads); 1024-thread workgroups running all
// rows of a row block at once (1614 -> 2890 us: one workgroup per CU).
// the fp32 instances run at >= 5 waves per SIMD (MOF_ROW_OCC: +1 % at C3);
// the fp64 ones keep the compiler's choice (the hint costs C2 fp64 2.7 %)
template <typename V, bool FIRST, bool ZH = false, bool PK = false>
__global__ __launch_bounds__(kWG) void k_pcg_spmv(PcgArgs<V> a, int32_t it, int32_t flags) {
    // bf16 z and the packed index words exist for the fp32 inner solve only
    // (the float specialisations)
    static_assert((!ZH && !PK) || sizeof(V) == 4, "bf16 z and packed indices need the fp32 SpMV");
    pcg_spmv_body<V, FIRST, ZH, PK>(a, it, flags);
}
#define MOF_SPMV_F32(FIRST, ZH, PK)                                                                          \
    template <>                                                                                              \
    __global__ __launch_bounds__(kWG) MOF_ROW_OCC void k_pcg_spmv<float, FIRST, ZH, PK>(PcgArgs<float> a,   \
                                                                                       int32_t it,          \
                                                                                       int32_t flags) {     \
        pcg_spmv_body<float, FIRST, ZH, PK>(a, it, flags);                                                   \
    }
MOF_SPMV_F32(true, false, false)
MOF_SPMV_F32(false, false, false)
MOF_SPMV_F32(true, true, false)
MOF_SPMV_F32(false, true, false)
MOF_SPMV_F32(true, false, true)
MOF_SPMV_F32(false, false, true)
MOF_SPMV_F32(true, true, true)
MOF_SPMV_F32(false, true, true)
#undef MOF_SPMV_F32
// workgroup size of an SpMV launch
template <typename V>
constexpr int spmv_wg() { return kWG; }
// grid of an SpMV launch over (row block, system) in the XCD order its body maps
template <typename V>
dim3 spmv_grid(const PcgArgs<V> &a) {
    return dim3(xcd_grid(a.nblk, a.sm.n, kGrpSpmv));
}
// the SpMV instance of a launch: first iteration or not, bf16 z, packed index words
template <typename V>
auto spmv_kernel(const PcgArgs<V> &a, bool first) -> void (*)(PcgArgs<V>, int32_t, int32_t) {
    if constexpr (sizeof(V) == 4) {
        if (a.mat.sell_idx) {
            if (a.zh) return first ? k_pcg_spmv<V, true, true, true> : k_pcg_spmv<V, false, true, true>;
            return first ? k_pcg_spmv<V, true, false, true> : k_pcg_spmv<V, false, false, true>;
        }
        if (a.zh) return first ? k_pcg_spmv<V, true, true> : k_pcg_spmv<V, false, true>;
    }
    return first ? k_pcg_spmv<V, true, false> : k_pcg_spmv<V, false, false>;
}
// its slot in g_pcg_launches
template <typename V>
int spmv_slot(const PcgArgs<V> &a, bool first) {
    const bool f32 = sizeof(V) == 4;
    return (f32 ? 0 : 8) + (first ? 4 : 0) + (f32 && a.zh ? 2 : 0) + (f32 && a.mat.sell_idx ? 1 : 0);
}
template <typename V>
void launch_spmv(const PcgArgs<V> &a, bool first, hipStream_t s, int32_t it, int32_t flags) {
    ++g_pcg_launches[spmv_slot(a, first)];
    spmv_kernel(a, first)<<<spmv_grid(a), spmv_wg<V>(), 0, s>>>(a, it, flags);
}

constexpr int kUpdRB = 4;  // row blocks per update workgroup
inline unsigned upd_blocks(int32_t nblk) { return (unsigned)((nblk + kUpdRB - 1) / kUpdRB); }

// g: the group of kUpdRB row blocks
template <typename V, int NQ = 1>
__device__ __forceinline__ void pcg_update_rows(const PcgArgs<V> &a, int32_t it, int32_t g, int32_t b) {
    __shared__ double lds[NQ * (kWG / 64) * 2 * kUpdRB];
    const int32_t tid = row_tid();
    int32_t *si = a.sysi + b * kSysStride;
    if (!si[SI_ACTIVE] || si[SI_CONV] >= 0) return;
    const int64_t ps = (int64_t)a.red.P * a.B * a.red.nmax * 2;
    double cur[2], pqv[1];
    bool self = false;
    if constexpr (NQ == 1) self = a.selfred != 0;
    if (self) {  // small meshes: k_red_rzrr's and k_red_pq's reductions here (same bits)
        __shared__ double lds2[2 * (kWG / 64)];
        reduce_sys<2, kWG>(a.part_rzrr + (it & 1) * ps, a.red, a.B, b, cur, lds2);
        reduce_sys<1, kWG>(a.part_pq + (it & 1) * ((int64_t)a.red.P * a.B * a.red.nmax), a.red, a.B, b, pqv, lds2);
    } else {
        const double *c = sc_rzrr(a.sc, a.B, it & 1, b);
        cur[0] = c[0];
        cur[1] = c[1];
        pqv[0] = *sc_pq(a.sc, a.B, it & 1, b);
    }
    if (cur[1] <= a.sysd[b * kSysStride + SD_TOL2]) return;
    // Every workgroup of the system reduces the same partials, so all take
    // the same decision: breakdown (p.q <= 0 or r.z <= 0: A or the
    // preconditioner is not SPD, e.g. an indefinite V-cycle; non-finite
    // values), divergence (|r|^2 grew kDiverge-fold), or stagnation (no new
    // smallest |r|^2 for `stall` iterations).
    int why = 0;
    if (!(pqv[0] > 0.0) || !(cur[0] > 0.0) || !isfinite(pqv[0]) || !isfinite(cur[0]) || !isfinite(cur[1]))
        why = FW_BREAKDOWN;
    else if (cur[1] > kDiverge * a.sysd[b * kSysStride + SD_RR0])
        why = FW_DIVERGED;
    else if (a.stall > 0 && it - si[SI_BEST_IT] > a.stall)
        why = FW_STALLED;
    if (why) {
        if (g == 0 && tid == 0) {
            si[SI_FAILED] = 1;
            si[SI_ACTIVE] = 0;
            si[SI_FAIL_IT] = it;
            si[SI_FAIL_WHY] = why;
        }
        return;
    }
    const V alpha = (V)(cur[0] / pqv[0]);
    using V2 = typename VT<V>::V2;
    // kUpdRB row blocks per workgroup (one partial record each): the update
    // has no gathers, so 1024 rows per workgroup amortise its fixed costs
    // whatever the row kernels' block size. Every load of the kUpdRB rows of
    // a thread is issued before the first use and the 2 kUpdRB partial sums
    // are formed by one block_sum (the same per-value order, so the same
    // bits as one block_sum<2> per row block).
    static_assert(kRows == 1, "one row per thread and row block");
    constexpr int R = kUpdRB;
    int32_t iv[R];
    V2 qv[R], rv[R];
#pragma unroll
    for (int q = 0; q < R; ++q) {
        iv[q] = (g * R + q) * kRowsPerWG + tid;
        const int64_t vi = (int64_t)b * a.N + min(iv[q], a.N - 1);
        qv[q] = *reinterpret_cast<const V2 *>(a.q + 2 * vi);
        rv[q] = *reinterpret_cast<const V2 *>(a.r + 2 * vi);
    }
    V dv[R][4];
    uint2 dh[R];
    if (!a.ext) {
#pragma unroll
        for (int q = 0; q < R; ++q) ld_blk(a.dinv, (int64_t)b * a.N + min(iv[q], a.N - 1), dv[q]);
    } else if constexpr (sizeof(V) == 4) {
#pragma unroll
        for (int q = 0; q < R; ++q) dh[q] = bf16_diag_block(a.dA, a.dA_nb, a.dA_off, b, min(iv[q], a.N - 1));
    }
    double v[2 * R];
#pragma unroll
    for (int q = 0; q < R; ++q) {
        const int32_t i = iv[q];
        double rz = 0.0, rr = 0.0;
        if (i < a.N) {
            const int64_t vi = (int64_t)b * a.N + i;
            // x += alpha p happens in the next SpMV launch (it reads p anyway)
            V2 ri = rv[q];
            ri.x = i < a.red.nown ? ri.x - alpha * qv[q].x : (V)0;
            ri.y = i < a.red.nown ? ri.y - alpha * qv[q].y : (V)0;
            *reinterpret_cast<V2 *>(a.r + 2 * vi) = ri;
            if (!a.ext) {
                const V *d = dv[q];
                const V z0 = d[0] * ri.x + d[1] * ri.y, z1 = d[2] * ri.x + d[3] * ri.y;
                *reinterpret_cast<V2 *>(a.z + 2 * vi) = V2{z0, z1};
                if (i < a.red.nown) rz += (double)ri.x * z0 + (double)ri.y * z1;
            } else if constexpr (sizeof(V) == 4) {
                // pre-smoothing of the V-cycle with the smoother's D^-1 (bf16)
                const float2 d = bf16_diag_solve(dh[q], ri.x, ri.y);
                st_x0(a.x0, vi, a.omega * d.x, a.omega * d.y);
            }
            if (i < a.red.nown) rr += (double)ri.x * ri.x + (double)ri.y * ri.y;
        }
        v[2 * q] = rz;
        v[2 * q + 1] = rr;
    }
    block_sum_q<2 * R, NQ>(v, lds);
    if (tid == 0) {
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const int32_t rbk = g * R + q;
            if (rbk >= a.nblk) break;
            double *o = a.part_rzrr + ((it + 1) & 1) * ps + 2 * red_rec(a.red, a.B, b, rbk);
            o[0] = v[2 * q];
            o[1] = v[2 * q + 1];
        }
    }
}
template <typename V>
__global__ __launch_bounds__(kWG) void k_pcg_update(PcgArgs<V> a, int32_t it) {
    pcg_update_rows<V>(a, it, blockIdx.x, sm_b(a.sm, blockIdx.y));
}

// x64 (+)= x_inner for systems active in the inner solve, and the block's
// max|d| and max|x64| over its owned rows (rdx.nown) into part_dx record
// red_rec(rdx, B, b, blk): the error control's inputs (k_outer_check).
template <typename V, int NQ = 1>
__device__ __forceinline__ void outer_update_rows(int32_t N, int32_t first, const V *__restrict__ xin,
                                                  const int32_t *__restrict__ sysi, double *__restrict__ x64,
                                                  const RedArgs &rdx, int32_t B, double *__restrict__ part_dx,
                                                  int32_t blk, int32_t b) {
    __shared__ double lds[8 * NQ];
    if (!sysi[b * kSysStride + SI_ACTIVE]) return;
    const int32_t i = blk * kWG + row_tid();
    double v[2] = {0.0, 0.0};
    if (i < N) {
        const int64_t vi = (int64_t)b * N + i;
        using V2 = typename VT<V>::V2;
        const V2 d = *reinterpret_cast<const V2 *>(xin + 2 * vi);
        double2 x = first ? make_double2(0.0, 0.0) : *reinterpret_cast<const double2 *>(x64 + 2 * vi);
        x.x += (double)d.x;
        x.y += (double)d.y;
        *reinterpret_cast<double2 *>(x64 + 2 * vi) = x;
        if (i < rdx.nown) {
            v[0] = fmax(fabs((double)d.x), fabs((double)d.y));
            v[1] = fmax(fabs(x.x), fabs(x.y));
        }
    }
    block_max_q<2, NQ>(v, lds);
    if (row_tid() == 0 && blk < rdx.nmax) {
        double *o = part_dx + 2 * red_rec(rdx, B, b, blk);
        o[0] = v[0];
        o[1] = v[1];
    }
}
template <typename V>
__global__ __launch_bounds__(kWG) void k_outer_update(int32_t N, int32_t first, const V *__restrict__ xin,
                                                      const int32_t *__restrict__ sysi, double *__restrict__ x64,
                                                      RedArgs rdx, int32_t B, double *__restrict__ part_dx) {
    outer_update_rows<V>(N, first, xin, sysi, x64, rdx, B, part_dx, blockIdx.x, blockIdx.y);
}

// r64 = f - A x64 in fp64 (lambda a2 + matrix-free a1 from the fp64 u) with
// partial |r|^2 and |f|^2.
template <int NQ = 1>
__device__ __forceinline__ void residual_rows(const OpArgs<double> &op, int32_t B, const RedArgs &rd,
                                              const double *__restrict__ rhs, const double *__restrict__ x64,
                                              const int32_t *__restrict__ sysi, double *__restrict__ r64,
                                              double *__restrict__ part, int32_t rb, int32_t b) {
    __shared__ double lds[8 * NQ];
    const int32_t tid = row_tid();
    if (!sysi[b * kSysStride + SI_ACTIVE]) return;
    const int32_t N = op.N;
    const int64_t vb = (int64_t)b * N;
    double rr = 0.0, ff = 0.0;
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const int32_t i = rb * kRowsPerWG + r * kWG + tid;
        if (i >= N) break;
        double y0, y1;
        apply_row_mf<double>(op, b, i, x64 + 2 * vb, y0, y1);
        const double2 f = *reinterpret_cast<const double2 *>(rhs + 2 * (vb + i));
        const double r0 = f.x - y0, r1 = f.y - y1;
        *reinterpret_cast<double2 *>(r64 + 2 * (vb + i)) = make_double2(r0, r1);
        if (i < rd.nown) {
            rr += r0 * r0 + r1 * r1;
            ff += f.x * f.x + f.y * f.y;
        }
    }
    double v[2] = {rr, ff};
    block_sum_q<2, NQ>(v, lds);
    if (tid == 0 && rb < rd.nmax) {
        double *o = part + 2 * red_rec(rd, B, b, rb);
        o[0] = v[0];
        o[1] = v[1];
    }
}
__global__ __launch_bounds__(kWG) void k_residual(OpArgs<double> op, int32_t nblk, int32_t B, RedArgs rd,
                                                  const double *__restrict__ rhs,
                                                  const double *__restrict__ x64,
                                                  const int32_t *__restrict__ sysi,
                                                  double *__restrict__ r64,
                                                  double *__restrict__ part) {
    int32_t rb, b;  // XCD-aware: the systems of a row block share its a2 blocks in L2
    if (!xcd_map(nblk, B, rb, b, kGrpRes)) return;
    residual_rows<1>(op, B, rd, rhs, x64, sysi, r64, part, rb, b);
}

// The re-forming residual, NS systems per thread (apply_row_rcn): grid
// over (row block, system group of NS) in the XCD-aware order; per-system
// partials summed in the same tree as k_residual's. NS = 2; 3 / 4 systems
// per thread (140 / 160 VGPRs, 3 waves): 5.73 / 6.78 vs 5.73 ms per launch
// (round 3, one incidence per load batch for 3 and 4). Measured and not kept
// (round 3, profiles/r03_ab/res_slot/): a row block's incidence slots spread
// over 4 / 2 thread groups of a 1024 / 512-thread workgroup, the terms
// staged in LDS and added by the row's thread in slot order (bit-identical):
// 8421 / 5539 vs 5093 us per launch.
constexpr int kResNS = 2;
// Row vi's r = f - y of one system, stored when the system is active, and its
// share of |r|^2, |f|^2 (owned rows only); shared by the row and the staged kernel.
__device__ __forceinline__ void rcn_out(int64_t vi, bool own, bool act, const double (&y)[2],
                                        const double *__restrict__ rhs, double *__restrict__ r64, double &rr,
                                        double &ff) {
    const double2 f = *reinterpret_cast<const double2 *>(rhs + 2 * vi);
    const double r0 = f.x - y[0], r1 = f.y - y[1];
    if (act) *reinterpret_cast<double2 *>(r64 + 2 * vi) = make_double2(r0, r1);
    if (own) {
        rr += r0 * r0 + r1 * r1;
        ff += f.x * f.x + f.y * f.y;
    }
}
// Pair bp's systems (the last pair of an odd batch repeats system B - 1) and
// which of them are live; false: none is.
template <int NS>
__device__ __forceinline__ bool res_pair(int32_t bp, int32_t B, const int32_t *__restrict__ sysi, int32_t (&bs)[NS],
                                         bool (&act)[NS]) {
    bool any = false;
#pragma unroll
    for (int t = 0; t < NS; ++t) {
        bs[t] = min(NS * bp + t, B - 1);
        act[t] = NS * bp + t < B && sysi[bs[t] * kSysStride + SI_ACTIVE] != 0;
        any |= act[t];
    }
    return any;
}
template <int NS>
__global__ __launch_bounds__(kWG) void k_residual_rcn(OpArgs<double> op, int32_t nblk, int32_t B, RedArgs rd,
                                                      const double *__restrict__ rhs,
                                                      const double *__restrict__ x64,
                                                      const int32_t *__restrict__ sysi,
                                                      double *__restrict__ r64,
                                                      double *__restrict__ part) {
    __shared__ double lds[8 * NS];
    int32_t rb, bp;
    if (!xcd_map(nblk, (B + NS - 1) / NS, rb, bp, kGrpRes)) return;
    int32_t bs[NS];
    bool act[NS];
    if (!res_pair<NS>(bp, B, sysi, bs, act)) return;
    const int32_t N = op.N;
    double v[2 * NS];  // rr, ff of each system
#pragma unroll
    for (int t = 0; t < 2 * NS; ++t) v[t] = 0.0;
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const int32_t i = rb * kRowsPerWG + r * kWG + threadIdx.x;
        if (i >= N) break;
        double y[NS][2];
        apply_row_rcn<NS>(op, bs, i, x64, y);
#pragma unroll
        for (int t = 0; t < NS; ++t) {
            rcn_out((int64_t)bs[t] * N + i, i < rd.nown, act[t], y[t], rhs, r64, v[2 * t], v[2 * t + 1]);
        }
    }
    block_sum<2 * NS>(v, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int t = 0; t < NS; ++t) {
            if (!act[t]) continue;
            double *o = part + 2 * red_rec(rd, B, bs[t], rb);
            o[0] = v[2 * t];
            o[1] = v[2 * t + 1];
        }
    }
}

// The re-forming residual with a row slice's geometry staged in LDS: a
// workgroup is one SELL-64 slice x W waves, lane l of every wave is row
// 64 s + l, and wave w takes the system pairs chunk (W TRIPS) + trip W + w.
// What apply_row_rcn gathers per system pair and that is the same for every
// system -- the slice's a2 columns and fp64 blocks, e_i, and per incidence
// the tinc record, the triangle's hat gradients and A_T / 12 and the tangent
// bases of the corner's two other vertices -- is loaded once by the whole
// workgroup into lane-major 16-byte planes (a wave's ds_read_b128 of a plane
// is 1 KiB of consecutive LDS) and read from there by every pair; only the
// per-system operands (x64, I, f) stay global gathers. The arithmetic is
// rcn_a2_term / rcn_tri_term's, the terms in the same slot and incidence
// order, so r64 keeps its bits. Per-system partials: each wave's wave_sum goes
// to a per-slice record and k_residual_fold adds a row block's four in
// block_sum's order.
//
// Staged bytes of a slice of wa a2 slots and wt incidence slots (double2
// units; kStagedRes, mof_internal.h): E 3 planes, BLK 2 wa, INC 12 wt
// {tinc | g0 g1 | g2 g3 | g4 g5 | g6 g7 | g8 w12 | ej x3 | ek x3}, then the wa
// 4-byte column planes. E and an incidence slot's first six planes are the
// ones the staged assembly has too (stage_e, stage_inc_geo, mof_staged.h).
//
// 16 waves x 4 trips (C3, 1536 systems: 10.27 / 9.15 / 8.78 ms per launch at
// 1 / 2 / 4 trips -- one workgroup per CU, so staging is not hidden and more
// pairs per workgroup amortise it; 8 waves with deeper load batches 10.4-10.5
// ms; profiles/res_lds/ab_levers.jsonl). Four a2 slots' gathers are issued
// before the first use, but one incidence's at a time: two per load batch
// need 68 B of scratch per lane at the 128 VGPRs a 1024-thread workgroup
// leaves a wave (110 and none as written, the trip loop not unrolled).
constexpr int kResLdsW = 16, kResLdsTrips = 4;
constexpr int kResLdsUA = 4;  // a2 slots per load batch
constexpr int32_t kGrpResLds = 1;  // an XCD walks consecutive slices of one pair chunk
constexpr int64_t kResLdsFill = 1024;  // workgroups (4 per CU) below which a launch takes one trip per wave
template <int NS, int W, int TRIPS>
__global__ __launch_bounds__(64 * W) void k_residual_lds(OpArgs<double> op, int32_t nsl, int32_t B, RedArgs rd,
                                                         const double *__restrict__ rhs,
                                                         const double *__restrict__ x64,
                                                         const int32_t *__restrict__ sysi,
                                                         double *__restrict__ r64,
                                                         double *__restrict__ spart) {
    extern __shared__ double2 sm[];
    constexpr int NT = 64 * W, PW = W * TRIPS;
    const int32_t npair = (B + NS - 1) / NS;
    int32_t s, chunk;
    if (!xcd_map(nsl, (npair + PW - 1) / PW, s, chunk, kGrpResLds)) return;  // workgroup-uniform
    const int32_t wv = threadIdx.x >> 6, l = threadIdx.x & 63;
    // any active system in the chunk? Every wave reads the same flags, so the
    // whole workgroup leaves here or nobody does (the barrier below).
    {
        bool any = false;
        for (int32_t q = l; q < PW * NS; q += 64) {
            const int32_t b = chunk * PW * NS + q;
            any |= b < B && sysi[min(b, B - 1) * kSysStride + SI_ACTIVE] != 0;
        }
        if (__ballot(any) == 0) return;
    }
    const int32_t N = op.N;
    const auto [o, wa, to, wt] = slice_view(op.sell_off, op.tsell_off, s);
    double2 *const E = sm, *const BLK = sm + 3 * 64, *const INC = BLK + 2 * 64 * wa;
    int32_t *const COL = reinterpret_cast<int32_t *>(INC + 12 * 64 * wt);
    // ---- staging (all NT threads; lanes past N - 1 of the last slice stage
    // the padding the tables hold for them and row N - 1's bases)
    for (int32_t q = threadIdx.x; q < wa * 64; q += NT) {
        const int32_t t = q >> 6, ll = q & 63;
        COL[q] = op.sell_col[(int64_t)o + q];
        const double2 *bp = reinterpret_cast<const double2 *>(op.a2s) + 2 * ((int64_t)o + q);
        BLK[(2 * t) * 64 + ll] = bp[0];
        BLK[(2 * t + 1) * 64 + ll] = bp[1];
    }
    stage_e<NT>(E, op.e, s, N);
    for (int32_t q = threadIdx.x; q < wt * 4 * 64; q += NT) {
        const int32_t ll = q & 63, part = (q >> 6) & 3, t = q >> 8;
        const int4 e = op.tinc[(int64_t)to + t * 64 + ll];
        double2 *P = stage_inc_geo<12>(INC, t, ll, part, e, op.gw, op.M, op.w12, e.x);
        if (part >= 2) {
            const double *ev = op.e + 6 * (int64_t)(part == 2 ? e.z : e.w);
            double2 *Q = P + (part == 2 ? 6 : 9) * 64;
            Q[0] = ld2(ev);
            Q[64] = ld2(ev + 2);
            Q[128] = ld2(ev + 4);
        }
    }
    __syncthreads();  // the only barrier: nothing below may wait for another wave
    // ---- compute: this wave's pairs
    const int32_t i = 64 * s + l;
#pragma unroll 1
    for (int trip = 0; trip < TRIPS; ++trip) {
        const int32_t bp = chunk * PW + trip * W + wv;
        if (bp >= npair) break;
        int32_t bs[NS];
        bool act[NS];
        if (!res_pair<NS>(bp, B, sysi, bs, act)) continue;
        double v[2 * NS];  // rr, ff of each system
#pragma unroll
        for (int t = 0; t < 2 * NS; ++t) v[t] = 0.0;
        if (i < N) {
            double acc[NS][2];
#pragma unroll
            for (int t = 0; t < NS; ++t) acc[t][0] = acc[t][1] = 0.0;
            // lambda a2 x, slots in order
            for (int32_t t0 = 0; t0 < wa; t0 += kResLdsUA) {
                double2 xj[kResLdsUA][NS];
#pragma unroll
                for (int u = 0; u < kResLdsUA; ++u) {
                    const int32_t j = COL[min(t0 + u, wa - 1) * 64 + l];
#pragma unroll
                    for (int t = 0; t < NS; ++t) xj[u][t] = ld2(x64 + 2 * ((int64_t)bs[t] * N + j));
                }
#pragma unroll
                for (int u = 0; u < kResLdsUA; ++u) {
                    const int32_t tt = min(t0 + u, wa - 1);
                    const double2 b0 = BLK[(2 * tt) * 64 + l], b1 = BLK[(2 * tt + 1) * 64 + l];
                    const double blk[4] = {b0.x, b0.y, b1.x, b1.y};
#pragma unroll
                    for (int t = 0; t < NS; ++t) rcn_a2_term(blk, xj[u][t], t0 + u < wa, acc[t]);
                }
            }
            // the row's own operands
            double2 xi[NS];
            double Ii[NS];
#pragma unroll
            for (int t = 0; t < NS; ++t) {
                xi[t] = ld2(x64 + 2 * ((int64_t)bs[t] * N + i));
                Ii[t] = op.I0[(int64_t)bs[t] * op.ldI + i];
            }
            double ei[6];
            ld_e(E, l, ei);
            // the incident triangles in order
            for (int32_t t0 = 0; t0 < wt; ++t0) {
                int4 q;
                const double2 *P = ld_inc_rec<12>(INC, t0, l, q);
                double Ij[NS], Ik[NS];
                double2 xj[NS], xk[NS];
#pragma unroll
                for (int t = 0; t < NS; ++t) {
                    const double *Ib = op.I0 + (int64_t)bs[t] * op.ldI;
                    const int64_t vb = (int64_t)bs[t] * N;
                    Ij[t] = Ib[q.z];
                    Ik[t] = Ib[q.w];
                    xj[t] = ld2(x64 + 2 * (vb + q.z));
                    xk[t] = ld2(x64 + 2 * (vb + q.w));
                }
                double g[9], w12;
                ld_inc_geo(P, g, w12);
                const double2 j0 = P[6 * 64], j1 = P[7 * 64], j2 = P[8 * 64];
                const double2 k0 = P[9 * 64], k1 = P[10 * 64], k2 = P[11 * 64];
                const double ej[6] = {j0.x, j0.y, j1.x, j1.y, j2.x, j2.y};
                const double ek[6] = {k0.x, k0.y, k1.x, k1.y, k2.x, k2.y};
#pragma unroll
                for (int t = 0; t < NS; ++t) {
                    double val[2];
                    rcn_tri_term(q.y, g, ei, ej, ek, w12, Ii[t], Ij[t], Ik[t], xi[t], xj[t], xk[t], val);
                    acc[t][0] += val[0];
                    acc[t][1] += val[1];
                }
            }
#pragma unroll
            for (int t = 0; t < NS; ++t)
                rcn_out((int64_t)bs[t] * N + i, i < rd.nown, act[t], acc[t], rhs, r64, v[2 * t], v[2 * t + 1]);
        }
#pragma unroll
        for (int t = 0; t < 2 * NS; ++t) v[t] = wave_sum(v[t]);
        if (l == 0) {
#pragma unroll
            for (int t = 0; t < NS; ++t) {
                if (!act[t]) continue;
                double *op_ = spart + 2 * ((int64_t)bs[t] * nsl + s);
                op_[0] = v[2 * t];
                op_[1] = v[2 * t + 1];
            }
        }
    }
}
// The (system, 256-row block) partial records from k_residual_lds's per-slice
// ones: the block's four wave sums added as block_sum adds them, slices past
// the last one counting 0.0 (as the waves past row N - 1 did).
__global__ __launch_bounds__(kWG) void k_residual_fold(int32_t nsl, int32_t nblk, int32_t B, RedArgs rd,
                                                       const int32_t *__restrict__ sysi,
                                                       const double *__restrict__ spart,
                                                       double *__restrict__ part) {
    const int64_t q = (int64_t)blockIdx.x * kWG + threadIdx.x;
    if (q >= (int64_t)B * nblk) return;
    const int32_t b = (int32_t)(q / nblk), rb = (int32_t)(q - (int64_t)b * nblk);
    if (!sysi[b * kSysStride + SI_ACTIVE]) return;
    double w[4][2];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int32_t s = 4 * rb + k;
        const double *p = spart + 2 * ((int64_t)b * nsl + min(s, nsl - 1));
        w[k][0] = s < nsl ? p[0] : 0.0;
        w[k][1] = s < nsl ? p[1] : 0.0;
    }
    double *out = part + 2 * red_rec(rd, B, b, rb);
    out[0] = ((w[0][0] + w[1][0]) + w[2][0]) + w[3][0];
    out[1] = ((w[0][1] + w[1][1]) + w[2][1]) + w[3][1];
}

// Max over all parts' max|d|, max|x64| records of system b (order-free).
template <int NT = kWG>
__device__ __forceinline__ void reduce_max_sys(const double *part, const RedArgs &rdx, int32_t B, int32_t b,
                                               double (&out)[2], double *lds) {
    out[0] = out[1] = 0.0;
    for (int32_t q = 0; q < rdx.P; ++q) {
        const double *p = part + 2 * ((int64_t)q * B + b) * rdx.nmax;
        for (int32_t w = threadIdx.x; w < rdx.nmax; w += NT) {
            out[0] = fmax(out[0], p[2 * (int64_t)w]);
            out[1] = fmax(out[1], p[2 * (int64_t)w + 1]);
        }
    }
    block_max<2, NT>(out, lds);
}

// One workgroup per system: relative true residual and error estimate;
// retire converged systems. The estimate of the error left after step k,
//   E = max|d_k| |r_{k+1}|_2 / |r_k|_2   (r_0 = f, so first: |r_k|^2 = |f|^2),
// is the last correction scaled by the step's residual reduction: A^-1's
// gain along r_k taken for r_{k+1}. From the second step on both residuals
// lie in the slow modes the first inner solve left, and E is within 0.5-1.8x
// of max|V - V*| (tools/error_control_study.py: S1-like patch, C2, C3; the
// first step's E underestimates ~100x on the open patch, but no first step
// of the mixed solve meets rtol). A system retires when rel <= rtol and, with
// etol > 0, kErrSafety E <= etol max|x64|.
template <int NT = kWG>
__device__ __forceinline__ void outer_check_sys(const RedArgs &rd, int32_t B, const double *__restrict__ part,
                                                const RedArgs &rdx, const double *__restrict__ part_dx,
                                                int32_t first, double rtol, double etol,
                                                double *__restrict__ sysd, int32_t *__restrict__ sysi,
                                                int32_t b) {
    __shared__ double lds[2 * (NT / 64)];
    int32_t *si = sysi + b * kSysStride;
    if (!si[SI_ACTIVE]) return;
    double v[2], dx[2];
    reduce_sys<2, NT>(part, rd, B, b, v, lds);
    reduce_max_sys<NT>(part_dx, rdx, B, b, dx, lds);
    if (threadIdx.x == 0) {
        double *sd = sysd + b * kSysStride;
        const double rel = v[1] > 0.0 ? sqrt(v[0] / v[1]) : (v[0] > 0.0 ? INFINITY : 0.0);
        const double rr_prev = first ? v[1] : sd[SD_RR];
        const double est = rr_prev > 0.0 ? dx[0] * sqrt(v[0] / rr_prev) : 0.0;
        sd[SD_REL] = rel;
        sd[SD_RR] = v[0];
        sd[SD_FF] = v[1];
        sd[SD_EST] = est;
        sd[SD_XMAX] = dx[1];
        if (!isfinite(rel) || !isfinite(est)) {
            si[SI_FAILED] = 1;
            si[SI_ACTIVE] = 0;
            si[SI_FAIL_WHY] = FW_RESIDUAL;
        } else {
            si[SI_MET] = rel <= rtol;
            if (rel <= rtol && (etol <= 0.0 || kErrSafety * est <= etol * dx[1])) si[SI_ACTIVE] = 0;
        }
    }
}
__global__ __launch_bounds__(kWG) void k_outer_check(RedArgs rd, int32_t B, const double *__restrict__ part,
                                                     RedArgs rdx, const double *__restrict__ part_dx,
                                                     int32_t first, double rtol, double etol,
                                                     double *__restrict__ sysd, int32_t *__restrict__ sysi) {
    outer_check_sys<kWG>(rd, B, part, rdx, part_dx, first, rtol, etol, sysd, sysi, blockIdx.x);
}

__global__ void k_sys_reset(int32_t B, int32_t *__restrict__ sysi, double *__restrict__ sysd) {
    const int32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    for (int k = 0; k < kSysStride; ++k) {
        sysi[b * kSysStride + k] = 0;
        sysd[b * kSysStride + k] = 0.0;
    }
    sysi[b * kSysStride + SI_ACTIVE] = 1;
    sysi[b * kSysStride + SI_CONV] = -1;
}

// Systems still active after the last refinement step fail -- except one
// whose residual met rtol and only the error estimate did not (kept; its
// estimate is reported through mof_stats.max_err_est). Likewise a system
// whose inner solve failed in a step after its residual had met rtol
// (SI_MET): the failed solve's correction was never added, x64 is the
// iterate that met rtol, and the system retires with it.
__device__ __forceinline__ void keep_met(int32_t *si) {
    if (si[SI_FAILED] && si[SI_MET] && si[SI_FAIL_WHY] != FW_RESIDUAL) {
        si[SI_FAILED] = 0;
        si[SI_FAIL_WHY] = 0;
    }
}
__global__ void k_mark_unconverged(int32_t B, double rtol, const double *__restrict__ sysd,
                                   int32_t *__restrict__ sysi) {
    const int32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    keep_met(sysi + b * kSysStride);
    if (sysi[b * kSysStride + SI_ACTIVE] && sysd[b * kSysStride + SD_REL] <= rtol) {
        sysi[b * kSysStride + SI_ACTIVE] = 0;
    } else if (sysi[b * kSysStride + SI_ACTIVE]) {
        sysi[b * kSysStride + SI_FAILED] = 1;
        sysi[b * kSysStride + SI_ACTIVE] = 0;
        sysi[b * kSysStride + SI_FAIL_WHY] = FW_MAXITER;
    }
}

// Systems still iterating when an inner solve ends at max_iter fail.
__global__ void k_fail_running(int32_t B, int32_t it, int32_t *__restrict__ sysi) {
    const int32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int32_t *si = sysi + b * kSysStride;
    if (si[SI_ACTIVE] && !si[SI_FAILED] && si[SI_CONV] < 0) {
        si[SI_FAILED] = 1;
        si[SI_ACTIVE] = 0;
        si[SI_FAIL_IT] = it;
        si[SI_FAIL_WHY] = FW_MAXITER;
    }
}

// u64 of the batch, or null when the mixed path left it unwritten (the
// residual then re-forms u from the batch's I rows)
OpArgs<double> op64(mof_mesh *m) {
    return make_op<double>(m, m->a2s64.p, m->w12_64.p, m->ws.u64_stale ? nullptr : m->ws.u64.p);
}

template <typename V>
MatArgs<V> make_mat(mof_mesh *m, const V *A) {
    MatArgs<V> mt;
    mt.sell_nb = m->pat.sell_nb();
    mt.sell_off = m->sell_off.p;
    mt.sell_col = m->sell_col.p;
    mt.sell_mir = m->sym_reads ? m->sell_mir.p : nullptr;
    mt.sell_idx = sizeof(V) == 4 && m->sym_reads && m->idx_packed ? m->sell_idx.p : nullptr;
    mt.vptr = m->sym_reads ? nullptr : m->vptr.p;
    mt.A = A;
    return mt;
}

// The staged residual of a mesh whose widest slice fits kStagedRes
// (mesh_set_own): k_residual_lds into the per-slice records (launch_staged,
// mof_staged.h), then the fold.
void launch_residual_lds(mof_mesh *m, const OpArgs<double> &op, int32_t nblk, int32_t B, hipStream_t s, RedArgs rd,
                         const double *rhs, const double *x64, const int32_t *sysi, double *r64, double *part) {
    static LdsLimit limit;
    const int32_t nsl = m->pat.nslices;
    MOF_REQUIRE(m->ws.res_spart.n >= (size_t)2 * nsl * B, "staged residual: workspace not set up");
    launch_staged<kResLdsW, kResLdsTrips>(&k_residual_lds<kResNS, kResLdsW, kResLdsTrips>,
                                          &k_residual_lds<kResNS, kResLdsW, 1>, kResLdsFill, kGrpResLds,
                                          (B + kResNS - 1) / kResNS, m, kStagedRes, m->res_lds, g_staged_res, limit, s,
                                          op, nsl, B, rd, rhs, x64, sysi, r64, m->ws.res_spart.p);
    const int64_t nrec = (int64_t)B * nblk;
    k_residual_fold<<<dim3((unsigned)((nrec + kWG - 1) / kWG)), kWG, 0, s>>>(nsl, nblk, B, rd, sysi,
                                                                             m->ws.res_spart.p, part);
}

// r64 = f - A x64 of the batch: from the u64 the fp64 path / recovery
// stored, or with u re-formed from the I rows (two systems per thread).
// Measured and not kept (round 3, profiles/r03_ab/a64_*): the row assembly
// folding a1 in fp64 and storing the fp64 A for a plain fp64 SpMV residual
// -- the residuals went 2 x 5.7 -> 2 x 3.6 ms per 512-system batch, the
// assembly 11.4 -> 15.6 ms (fp64 accumulators: 165 VGPRs, 3 waves, and
// 10.7 GB of A64 stores): C3 3380-3383 vs 3378-3389 timesteps/s.
template <typename... Args>
void launch_residual(mof_mesh *m, int32_t nblk, int32_t B, hipStream_t s, RedArgs rd, Args... args) {
    const OpArgs<double> op = op64(m);
    if (op.u)
        k_residual<<<dim3(xcd_grid(nblk, B, kGrpRes)), kWG, 0, s>>>(op, nblk, B, rd, args...);
    else if (m->res_lds.used)
        launch_residual_lds(m, op, nblk, B, s, rd, args...);
    else {
        g_staged_res.launches[0]++;
        k_residual_rcn<kResNS><<<dim3(xcd_grid(nblk, (B + kResNS - 1) / kResNS, kGrpRes)), kWG, 0, s>>>(
            op, nblk, B, rd, args...);
    }
}

// amg: z and r.z come from m's V-cycle (fp32 only), with the level-0 smoother
// data the init and the update write the pre-smoothing with
template <typename V>
PcgArgs<V> make_args(mof_mesh *m, int32_t B, const MatArgs<V> &mat, const V *dinv, bool amg = false) {
    Workspace &w = m->ws;
    PcgArgs<V> a;
    a.N = m->N;
    a.nblk = w.nblk;
    a.B = B;
    a.sm = sys_all(B);
    a.selfred = 0;
    a.mat = mat;
    a.dinv = dinv;
    a.x = reinterpret_cast<V *>(w.vx.p);
    a.r = reinterpret_cast<V *>(w.vr.p);
    a.z = reinterpret_cast<V *>(w.vz.p);
    a.p = reinterpret_cast<V *>(w.vp.p);
    a.q = reinterpret_cast<V *>(w.vq.p);
    a.part_pq = w.part_pq.p;
    a.part_rzrr = w.part_rzrr.p;
    a.sysd = w.sysd.p;
    a.sysi = w.sysi.p;
    a.red = RedArgs{1, 0, w.nblk, m->N};
    a.ext = 0;
    a.x0 = nullptr;
    a.omega = (V)0;
    a.dA = nullptr;
    a.dA_nb = 0;
    a.dA_off = nullptr;
    a.stall = 0;
    a.sc = w.sc.p;
    a.zh = 0;
    if constexpr (sizeof(V) == 4) {
        if (amg) {
            const AmgFine f = amg_fine(m);
            a.ext = 1;
            a.x0 = f.x0;
            a.omega = f.omega;
            a.dA = static_cast<const uint2 *>(f.A0h);
            a.dA_nb = f.sell_nb;
            a.dA_off = f.sell_off;
        }
    }
    return a;
}

// the workspace's assembled operator and block-Jacobi inverses of the working type
template <typename V>
const V *ws_A(const Workspace &w) {
    if constexpr (sizeof(V) == 4)
        return w.A32.p;
    else
        return w.A64.p;
}
template <typename V>
const V *ws_dinv(const Workspace &w) {
    if constexpr (sizeof(V) == 4)
        return w.dinv32.p;
    else
        return w.dinv64.p;
}

// The local meshes of one solve, run in lockstep on one stream: the mesh of a
// single-domain solve (d == nullptr), or the local parts of a decomposed one
// (mof_dd.h): all P of an in-process handle, one of a rank's. Every stage of
// pcg() and refine() is a loop over `mesh`, followed by halo() / sync() where
// the parts refresh ghost rows or complete the shared partial records; both
// do nothing on a single domain. Ghost rows are computed but never summed,
// and every reduction runs over the [P][B][nmax] records of all parts in one
// order, so all parts take the same decisions bit for bit.
// "Single domain" is d == nullptr, never mesh.size() == 1: a rank with one
// local part takes every host decision its peers take and enters every
// collective.
template <typename V>
struct Parts {
    mof_dd *d;
    int32_t B;
    std::vector<mof_mesh *> mesh;
    mof_mesh *host;  // the mesh whose h_sysi / h_sysd mirror the host reads (all parts hold the same flags)
    // the partial arrays and their record strides: the mesh's own (P = 1), or the handle's shared ones
    double *part_pq, *part_rzrr, *part_rr0, *part_dx;
    int32_t P, nmax, nvmax;
    std::vector<RedArgs> rd, rdx;   // per mesh: the records of the row-block sums, of k_outer_update's maxima
    std::vector<PcgArgs<V>> args;   // per mesh (fill_args)

    Parts(mof_mesh *m, mof_dd *dd, int32_t nb) : d(dd), B(nb) {
        if (d) {
            mesh = d->parts;
            part_pq = d->part_pq.p, part_rzrr = d->part_rzrr.p, part_rr0 = d->part_rr0.p, part_dx = d->part_dx.p;
            P = d->P, nmax = d->nmax, nvmax = d->nvmax;
            for (int32_t id : d->part_ids) {
                rd.push_back(RedArgs{P, id, nmax, d->plan.parts[id].n_own});
                rdx.push_back(RedArgs{P, id, nvmax, d->plan.parts[id].n_own});
            }
        } else {
            Workspace &w = m->ws;
            mesh = {m};
            part_pq = w.part_pq.p, part_rzrr = w.part_rzrr.p, part_rr0 = w.part_rr0.p, part_dx = w.part_dx.p;
            P = 1, nmax = w.nblk, nvmax = (m->N + kWG - 1) / kWG;
            rd = {RedArgs{1, 0, nmax, m->N}};
            rdx = {RedArgs{1, 0, nvmax, m->N}};
        }
        host = mesh[0];
    }
    // once the multigrid's storage and damping of this solve are in place (make_args reads them)
    void fill_args(bool amg, int32_t stall) {
        args.clear();
        for (size_t l = 0; l < mesh.size(); ++l) {
            const Workspace &w = mesh[l]->ws;
            PcgArgs<V> a = make_args<V>(mesh[l], B, make_mat<V>(mesh[l], ws_A<V>(w)), ws_dinv<V>(w), amg);
            a.part_pq = part_pq;
            a.part_rzrr = part_rzrr;
            a.red = rd[l];
            a.stall = stall;
            args.push_back(a);
        }
    }
    // refresh the ghost rows of every part's z (which = 0) or x64 (which = 1)
    void halo(int which, hipStream_t s) const {
        if (d) dd_halo(d, B, which == 0 && sizeof(V) == 4, which, s);
    }
    // every part's records of one partial array, per_part doubles each, complete on every rank
    void sync(double *base, size_t per_part, hipStream_t s) const {
        if (d) dd_sync_partials(d, base, per_part, s);
    }
};

void fetch_flags(mof_mesh *m, int32_t B, hipStream_t s) {
    const auto t0 = std::chrono::steady_clock::now();
    MOF_HIP(hipMemcpyAsync(m->h_sysi, m->ws.sysi.p, sizeof(int32_t) * kSysStride * B,
                           hipMemcpyDeviceToHost, s));
    MOF_HIP(hipMemcpyAsync(m->h_sysd, m->ws.sysd.p, sizeof(double) * kSysStride * B,
                           hipMemcpyDeviceToHost, s));
    MOF_HIP(hipStreamSynchronize(s));
    g_fetch_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    g_fetch_n++;
}

// Longest first chunk of launches queued before the host looks at the flags.
constexpr int32_t kMaxChunk = 256;
// row blocks up to which the SpMV and the update reduce their scalars
// themselves (PcgArgs::selfred): each workgroup then sums at most this many
// records per value instead of reading one pre-reduced double
constexpr int32_t kSelfRedBlk = 32;
// a chunk whose running systems are at most this fraction of the batch
// launches over them alone (pcg, SysMap). One box, round 5
// (profiles/r05_ab/compact/): S1 1134 -> 1162 timesteps/s (its third and
// fourth refinement steps run a few systems each), R3 / C3 / F3 unchanged
// within noise; 0.5, or no first-chunk split, the same
constexpr double kCompactFrac = 0.9;
// pcg's hints: hint[0] the previous batch's slowest convergence, hint[kBulkHint]
// the iteration by which kBulkFrac of its systems had converged -- the first
// chunk stops there, so the tail (the slow few) runs compacted
constexpr int32_t kBulkHint = 48;
constexpr double kBulkFrac = 0.9;

// Iterations of a system in an inner solve that has queued `it` of them:
// SI_CONV (the SpMV launch that saw it converged), f + 1 after a failure at
// update iteration f, all `it` if it is still running or failed at the cap.
inline int32_t sys_iters(const int32_t *si, int32_t it) {
    if (si[SI_CONV] >= 0) return si[SI_CONV];
    return si[SI_FAILED] && si[SI_FAIL_WHY] != FW_MAXITER ? si[SI_FAIL_IT] + 1 : it;
}

// Systems of a chunk [it0, it0 + n) each timed SpMV launch processed: system
// b works in launch it while it < sys_iters(b).
void charge_chunk(const mof_mesh *m, int32_t B, const std::vector<int32_t> &running_at, int32_t it0,
                  int32_t n, uint32_t precision, int32_t solve_systems, const std::vector<float> &ms,
                  SpmvTiming *t) {
    std::vector<int32_t> active(n, 0);
    for (int32_t b = 0; b < B; ++b) {
        if (!running_at[b]) continue;
        const int32_t last = sys_iters(m->h_sysi + b * kSysStride, it0 + n);
        for (int32_t c = 0; c < n && it0 + c < last; ++c) active[c]++;
    }
    for (int32_t c = 0; c < n; ++c) {
        t->ms += ms[c];
        t->launches++;
        t->systems += active[c];
        if (active[c]) t->bytes += spmv_launch_bytes(m, precision, active[c]);
        if (active[c] == solve_systems) {
            t->full_launches++;
            t->ms_full += ms[c];
        }
    }
}

// Inner PCG on all active systems of every local part (rhs: one per part);
// returns iterations summed over systems. One iteration is, over all parts:
// halo(z), the SpMV, sync(p.q), k_red_pq, the update, k_pcg_conv_early, the
// V-cycles, sync(r.z, |r|^2), k_red_rzrr.
template <typename V>
int64_t pcg(Parts<V> &p, const double *const *rhs, double rtol, const SolveParams &sp, hipStream_t s,
            int32_t *max_iters, SpmvTiming *timing, int32_t *hint, bool amg, double outer_rtol = 0.0,
            double etol = 0.0) {
    const int32_t max_iter = sp.max_iter, B = p.B;
    const size_t L = p.mesh.size();
    mof_mesh *mh = p.host;
    std::vector<PcgArgs<V>> &args = p.args;
    // What saves launches, so far on a single domain only (there: one mesh, args[0]):
    const bool single = p.d == nullptr;
    // launches over the running systems alone (SysMap, kCompactFrac)
    const bool compact = single;
    // a mesh of at most kSelfRedBlk row blocks: the SpMV and the update
    // reduce their scalars themselves (same bits as the k_red_* launches)
    const bool selfred = single && args[0].red.P == 1 && args[0].nblk <= kSelfRedBlk;
    // a system converged after the update skips that iteration's V-cycle
    // (k_pcg_conv_early; same bits: its z was never used)
    const bool early = amg && single;
    // bf16 z on regular meshes with the tentative prolongator (C3 +1 %, C2
    // mixed +2 %, same iterations); R3 on the smoothed one: 63 vs 50 its.
    // The halo exchange moves float2 z
    bool zh = false;
    if constexpr (sizeof(V) == 4) zh = amg && single && amg_fine(p.mesh[0]).regular;
    // the first chunk stops where the bulk of the previous batch's systems had converged (hint[kBulkHint])
    const bool bulk_hint = single;
    // the SpMV launches carry events (charge_chunk)
    const bool timed = timing && single;
    // the per-system tolerance of a later refinement step (k_pcg_tol): the parts' stop rule ignores both
    if (!single) outer_rtol = etol = 0.0;
    for (PcgArgs<V> &a : args) {
        a.sm = sys_all(B);
        a.selfred = selfred;
        a.zh = zh;
    }
    const int64_t rec = (int64_t)B * p.nmax;  // records of one part
    const int64_t pqs = p.P * rec, ps = 2 * pqs;  // slot strides of part_pq, part_rzrr
    // z = M^-1 r per part (block Jacobi over the parts, a V-cycle inside
    // each), r.z into slot `slot`
    auto cycles = [&](int32_t slot) {
        if constexpr (sizeof(V) == 4)
            for (size_t l = 0; l < L; ++l)
                amg_vcycle(p.mesh[l], B, args[l].r, args[l].z, p.part_rzrr + slot * ps, args[l].nblk, args[l].red, s,
                           zh, args[l].sm.map, args[l].sm.n);
    };
    auto sync_rzrr = [&](int32_t slot) { p.sync(p.part_rzrr + slot * ps, 2 * rec, s); };
    auto red_rzrr = [&](int32_t slot) {
        if (selfred) return;
        for (size_t l = 0; l < L; ++l) {
            ++g_pcg_launches[kPcRedRzrr];
            k_red_rzrr<V><<<dim3((unsigned)args[l].sm.n), kWG, 0, s>>>(args[l], slot);
        }
    };
    auto red_pq = [&](int32_t slot) {
        if (selfred) return;
        for (size_t l = 0; l < L; ++l) {
            ++g_pcg_launches[kPcRedPq];
            k_red_pq<V><<<dim3((unsigned)args[l].sm.n), kWG, 0, s>>>(args[l], slot);
        }
    };
    // SpMV launch `it_` of every part, its p.q records complete; e0, e1 (timed):
    // events stamped by the kernel's own dispatch packet (start and end of its
    // execution, as rocprof's kernel trace), not separate marker packets around it
    auto spmv = [&](bool first, int32_t it_, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr) {
        p.halo(0, s);
        for (size_t l = 0; l < L; ++l) {
            const PcgArgs<V> &a = args[l];
            if (e0) {
                ++g_pcg_launches[spmv_slot(a, first)];
                hipExtLaunchKernelGGL(spmv_kernel(a, first), spmv_grid(a), dim3(spmv_wg<V>()), 0, s, e0, e1, 0, a, it_, 0);
            } else {
                launch_spmv(a, first, s, it_, 0);
            }
        }
        p.sync(p.part_pq + (it_ & 1) * pqs, rec, s);  // this parity's slot
    };
    // systems active at the start of this solve: the host mirror is current
    // (reset by refine, refreshed by every outer check)
    std::vector<int32_t> was_active(B), running_at(B);
    int32_t solve_systems = 0;
    for (int32_t b = 0; b < B; ++b) {
        was_active[b] = mh->h_sysi[b * kSysStride + SI_ACTIVE];
        solve_systems += was_active[b];
    }
    running_at = was_active;
    // launches over the running systems only when they are at most
    // kCompactFrac of the batch (SysMap): a later refinement step's few
    // systems from the start, a long tail from its chunk boundary (same bits)
    std::vector<int32_t> h_map(B);  // read by the async upload until the next fetch_flags
    auto cover = [&](int32_t n) {   // h_map[0, n) (compact: one mesh)
        int32_t *smap = p.mesh[0]->ws.smap.p;
        MOF_HIP(hipMemcpyAsync(smap, h_map.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, s));
        args[0].sm = SysMap{smap, n};
        ++g_pcg_launches[kPcCompact];
    };
    if (compact && solve_systems <= kCompactFrac * B) {
        int32_t n = 0;
        for (int32_t b = 0; b < B; ++b)
            if (was_active[b]) h_map[n++] = b;
        if (n > 0) cover(n);
    }
    for (size_t l = 0; l < L; ++l)
        k_pcg_init<V><<<dim3((unsigned)args[l].nblk, (unsigned)B), kWG, 0, s>>>(args[l], rhs[l]);
    sync_rzrr(0);
    // the tolerance step resets the convergence word the cycle's kernels
    // check, so it runs before the first cycle
    for (size_t l = 0; l < L; ++l) k_pcg_tol<V><<<dim3((unsigned)B), kWG, 0, s>>>(args[l], rtol, outer_rtol, etol);
    if (amg) {
        cycles(0);
        sync_rzrr(0);
    }
    red_rzrr(0);
    MOF_HIP(hipGetLastError());
    // The first chunk runs as many iterations as the same solve of the
    // previous batch needed (timesteps of one run converge alike), so the
    // host usually synchronises once per inner solve; converged systems
    // retire on the device, so overshooting costs only early-exit launches.
    // With a tail (the previous batch's slowest system 2+ iterations past
    // the bulk of them, kBulkFrac) the first chunk stops at the bulk and the
    // rest runs compacted, straight to the previous slowest.
    int32_t it = 0;
    const int32_t bulk = bulk_hint ? hint[kBulkHint] : 0;
    const bool split = bulk > 0 && *hint >= bulk + 2;
    int32_t chunk = split ? std::min(bulk, kMaxChunk) : (*hint > 0 ? std::min(*hint, kMaxChunk) : 8);
    bool done = false;
    std::vector<hipEvent_t> &ev = mh->spmv_events;
    std::vector<float> ms;
    while (!done && it < max_iter) {
        const int32_t n = std::min(chunk, max_iter - it);
        if (timed && (int32_t)ev.size() < 2 * n) {
            const size_t old = ev.size();
            ev.resize(2 * (size_t)std::max(n, 64));
            for (size_t q = old; q < ev.size(); ++q) MOF_HIP(hipEventCreate(&ev[q]));
        }
        const int32_t it0 = it;
        for (int32_t c = 0; c < n; ++c, ++it) {
            if (timed)
                spmv(it == 0, it, ev[2 * c], ev[2 * c + 1]);
            else
                spmv(it == 0, it);
            red_pq(it & 1);
            for (const PcgArgs<V> &a : args) {
                ++g_pcg_launches[kPcUpdate];
                k_pcg_update<V><<<dim3(upd_blocks(a.nblk), (unsigned)a.sm.n), kWG, 0, s>>>(a, it);
            }
            for (size_t l = 0; early && l < L; ++l) {
                ++g_pcg_launches[kPcConvEarly];
                k_pcg_conv_early<V><<<dim3((unsigned)args[l].sm.n), kWG, 0, s>>>(args[l], it);
            }
            if (amg) cycles((it + 1) & 1);
            sync_rzrr((it + 1) & 1);
            red_rzrr((it + 1) & 1);
        }
        MOF_HIP(hipGetLastError());
        fetch_flags(mh, B, s);
        if (timed) {
            ms.assign(n, 0.f);
            for (int32_t c = 0; c < n; ++c) MOF_HIP(hipEventElapsedTime(&ms[c], ev[2 * c], ev[2 * c + 1]));
            charge_chunk(mh, B, running_at, it0, n, sp.precision, solve_systems, ms, timing);
        }
        done = true;
        int32_t owe_or_run = 0;
        for (int32_t b = 0; b < B; ++b) {
            const int32_t *si = mh->h_sysi + b * kSysStride;
            running_at[b] = si[SI_ACTIVE] && !si[SI_FAILED] && si[SI_CONV] < 0;
            if (running_at[b]) done = false;
            // the next chunk's launches: the running systems and those owed
            // the deferred x update of SpMV launch `it` (marked early by the
            // chunk's last iteration)
            if (was_active[b] && !si[SI_FAILED] && (si[SI_CONV] < 0 || si[SI_CONV] >= it)) h_map[owe_or_run++] = b;
        }
        chunk = split && it == std::min(bulk, kMaxChunk) && *hint > it ? std::min(*hint - it, kMaxChunk) : 8;
        // a tail chunk (at most kCompactFrac of the batch still running)
        // launches over those systems only; same bits (SysMap)
        if (compact && !done && owe_or_run <= kCompactFrac * B) cover(owe_or_run);
    }
    if (!done) {
        // one more check launch so SI_CONV records systems converged at max_iter
        // (it == 0 only with max_iter = 0, the test hook's cap 0: the first instance, which reads
        // no previous iteration's scalars); on parts its p.q is reduced like any SpMV's (no launch reads it)
        spmv(it == 0, it);
        if (!single) red_pq(it & 1);
        if (sp.fail_at_max_iter)
            for (const PcgArgs<V> &a : args)
                k_fail_running<<<dim3((unsigned)((B + 63) / 64)), 64, 0, s>>>(B, it, a.sysi);
        MOF_HIP(hipGetLastError());
        fetch_flags(mh, B, s);
    } else if (early) {
        // systems marked by the last queued iteration (SI_CONV == it) still
        // owe the deferred x += alpha p of SpMV launch `it`: that launch alone
        // (every other system is retired in it)
        bool owe = false;
        for (int32_t b = 0; b < B && !owe; ++b)
            owe = was_active[b] && mh->h_sysi[b * kSysStride + SI_CONV] == it;
        if (owe) spmv(false, it);
        MOF_HIP(hipGetLastError());
    }
    int64_t total = 0;
    int32_t slowest = 0, slowest_conv = 0;
    std::vector<int32_t> convs;
    for (int32_t b = 0; b < B; ++b) {
        if (!was_active[b]) continue;
        const int32_t *si = mh->h_sysi + b * kSysStride;
        const int32_t c = si[SI_CONV], its = sys_iters(si, it);
        total += its;
        slowest = std::max(slowest, its);
        if (c >= 0) {
            slowest_conv = std::max(slowest_conv, c);
            if (bulk_hint) convs.push_back(c);
        }
    }
    if (!convs.empty()) {
        const size_t k = std::min(convs.size() - 1, (size_t)(kBulkFrac * (double)convs.size()));
        std::nth_element(convs.begin(), convs.begin() + k, convs.end());
        hint[kBulkHint] = convs[k];
    }
    *max_iters = std::max(*max_iters, slowest);
    // the next batch's first chunk: +1 because convergence is seen by the
    // launch after (with the early mark, by the iteration itself: the owed
    // SpMV launch above finishes it); only converged systems count (a failed
    // or capped solve must not queue max_iter launches before the next look
    // at the flags)
    if (slowest_conv > 0) *hint = std::min(slowest_conv + (early ? 0 : 1), kMaxChunk);
    return total;
}

// the recovery's damped pass: the meshes' smoother damping for this solve only
struct OmegaScope {
    const std::vector<mof_mesh *> &mesh;
    std::vector<float> old;
    OmegaScope(const std::vector<mof_mesh *> &ms, float om, bool use) : mesh(ms) {
        if (use && om > 0.f)
            for (mof_mesh *m : mesh) old.push_back(amg_set_omega(m, om));
    }
    ~OmegaScope() {
        for (size_t l = 0; l < old.size(); ++l) amg_set_omega(mesh[l], old[l]);
    }
};

// The eager solve of a batch on one mesh (d null) or on d's local parts:
// inner PCG in the working type V, fp64 iterative refinement around it.
template <typename V>
int64_t refine(mof_mesh *m, mof_dd *d, int32_t B, const SolveParams &sp, hipStream_t s, int32_t *outer,
               int32_t *max_iters, SpmvTiming *tm, const uint8_t *only) {
    constexpr bool f32 = sizeof(V) == 4;
    Parts<V> p(m, d, B);
    const size_t L = p.mesh.size();
    mof_mesh *mh = p.host;
    const dim3 gsys((unsigned)((B + 63) / 64));
    // a fresh solve resets every system; with `only`, the selected systems
    // are re-solved from x = 0 and the others stay retired with their
    // solution, residual and flags (the host mirror is the state of the
    // previous solve's last fetch; every part holds the same flags)
    if (!only) {
        for (mof_mesh *q : p.mesh) k_sys_reset<<<gsys, 64, 0, s>>>(B, q->ws.sysi.p, q->ws.sysd.p);
        MOF_HIP(hipGetLastError());
    }
    for (int32_t b = 0; b < B; ++b) {
        if (only && !only[b]) continue;
        int32_t *si = mh->h_sysi + b * kSysStride;
        for (int k = 0; k < kSysStride; ++k) si[k] = 0;
        si[SI_ACTIVE] = 1;
        si[SI_CONV] = -1;
    }
    if (only)
        for (mof_mesh *q : p.mesh)
            MOF_HIP(hipMemcpyAsync(q->ws.sysi.p, mh->h_sysi, sizeof(int32_t) * kSysStride * B, hipMemcpyHostToDevice,
                                   s));
    if (d) {
        // records of workgroups past a part's own count must read as zero, and
        // their positions move with B: clear the shared arrays per batch
        MOF_HIP(hipMemsetAsync(d->part_pq.p, 0, d->part_pq.bytes(), s));
        MOF_HIP(hipMemsetAsync(d->part_rzrr.p, 0, d->part_rzrr.bytes(), s));
        MOF_HIP(hipMemsetAsync(d->part_rr0.p, 0, d->part_rr0.bytes(), s));
        MOF_HIP(hipMemsetAsync(d->part_dx.p, 0, d->part_dx.bytes(), s));
    }
    // the multigrid on every part, or on none
    bool amg = sp.amg && f32;
    for (size_t l = 0; l < L && amg; ++l) amg = amg_build(p.mesh[l]);
    if (amg)
        for (mof_mesh *q : p.mesh) {
            amg_ensure(q, B);
            // a recovery pass (only) re-solves systems of this batch, whose
            // coarse operators are still in place
            if (!only) amg_setup_batch(q, B, s);
        }
    OmegaScope omega_scope(p.mesh, sp.amg_omega, amg);
    p.fill_args(amg, sp.stall);
    // pcg's hints per (precision, preconditioner, refinement step), on a
    // single domain followed by its bulk hints
    std::vector<int32_t> &hints = mh->iter_hint;
    const size_t nhint = d ? 2 * 16 : 2 * kBulkHint;
    if (hints.size() < nhint) hints.assign(nhint, 0);
    const int32_t hint0 = !f32 ? 0 : (d || amg ? 16 : 32);
    std::vector<const double *> rhs(L);
    int64_t iters = 0, iters_before = 0;
    int32_t o = 0;
    // MOF_VERBOSE: per refinement step iterations and residuals on stderr
    static const bool verbose = knob(Knob::Verbose) != nullptr;
    for (; o < sp.max_outer; ++o) {
        for (size_t l = 0; l < L; ++l) rhs[l] = o == 0 ? p.mesh[l]->ws.rhs.p : p.mesh[l]->ws.r64.p;
        // the fp64 solve's first step to 0.5 rtol
        iters += pcg<V>(p, rhs.data(), !f32 && o == 0 ? 0.5 * sp.rtol : sp.inner_rtol, sp, s, max_iters, tm,
                        &hints[hint0 + std::min(o, 15)], amg, o > 0 && sp.adaptive_inner ? sp.rtol : 0.0, sp.etol);
        for (size_t l = 0; l < L; ++l) {
            mof_mesh *q = p.mesh[l];
            Workspace &w = q->ws;
            const dim3 gv((unsigned)((q->N + kWG - 1) / kWG), (unsigned)B);  // one row per thread
            ++g_pcg_launches[kPcOuterUpdate];
            k_outer_update<V><<<gv, kWG, 0, s>>>(q->N, o == 0, p.args[l].x, w.sysi.p, w.x64.p, p.rdx[l], B, p.part_dx);
        }
        p.sync(p.part_dx, 2 * (size_t)B * p.nvmax, s);
        p.halo(1, s);  // the residual reads x64 at the ghosts
        for (size_t l = 0; l < L; ++l) {
            Workspace &w = p.mesh[l]->ws;
            launch_residual(p.mesh[l], w.nblk, B, s, p.rd[l], w.rhs.p, w.x64.p, w.sysi.p, w.r64.p, p.part_rr0);
        }
        p.sync(p.part_rr0, 2 * (size_t)B * p.nmax, s);
        for (size_t l = 0; l < L; ++l) {
            Workspace &w = p.mesh[l]->ws;
            RedArgs rd = p.rd[l], rdx = p.rdx[l];
            if (d) rd.nown = rdx.nown = 0;  // the check sums records, not rows: the parts pass no row count
            ++g_pcg_launches[kPcOuterCheck];
            k_outer_check<<<dim3((unsigned)B), kWG, 0, s>>>(rd, B, p.part_rr0, rdx, p.part_dx, o == 0, sp.rtol,
                                                            sp.etol, w.sysd.p, w.sysi.p);
        }
        MOF_HIP(hipGetLastError());
        fetch_flags(mh, B, s);
        bool any = false;
        for (int32_t b = 0; b < B; ++b) any |= mh->h_sysi[b * kSysStride + SI_ACTIVE] != 0;
        if (verbose) {
            double worst = 0.0, west = 0.0;
            int32_t act = 0;
            for (int32_t b = 0; b < B; ++b) {
                const double *sd = mh->h_sysd + b * kSysStride;
                worst = std::max(worst, sd[SD_REL]);
                if (sd[SD_XMAX] > 0.0) west = std::max(west, sd[SD_EST] / sd[SD_XMAX]);
                act += mh->h_sysi[b * kSysStride + SI_ACTIVE] != 0;
            }
            std::fprintf(stderr,
                         "[mof solve] B=%d outer %d: %lld inner its (sum), max rel residual %.3e, max error est %.3e "
                         "of max|V|, %d still active\n",
                         B, o, (long long)(iters - iters_before), worst, west, act);
            iters_before = iters;
        }
        if (!any) {
            ++o;
            break;
        }
    }
    for (mof_mesh *q : p.mesh) k_mark_unconverged<<<gsys, 64, 0, s>>>(B, sp.rtol, q->ws.sysd.p, q->ws.sysi.p);
    MOF_HIP(hipGetLastError());
    fetch_flags(mh, B, s);
    *outer = o;
    return iters;
}

// ---- the fused small-mesh solve ---------------------------------------------
// On a small mesh every launch of the eager solve is a few microseconds of
// work behind a few microseconds of launch and dependency latency: C1 (642
// vertices, 15 systems) needs ~300 launches per batch and is launch-bound
// (SURVEY.md §7 hard part 4). k_solve_fused runs the whole fp64 block-Jacobi
// solve of one system -- every refinement step's inner PCG (init, tolerance,
// SpMV / p.q / update / r.z iterations, the max_iter check launch), the x64
// update, the fp64 residual and the outer check -- in one workgroup, calling
// the eager kernels' bodies for each of its row blocks in turn with a
// workgroup barrier where the eager path has a launch boundary. Same bodies,
// same row blocks, same partial records and reduction order: V, the flags and
// the iteration counts are bit-identical to the eager path
// (tests/test_gpu_fused.py). One launch and one flag fetch per batch.
struct FusedArgs {
    const double *rhs;  // f of every system
    double *x64, *r64, *part_rr0, *part_dx;
    double rtol, inner_rtol, etol;
    int32_t max_iter, max_outer, adaptive;
};

// flags written by other threads of the workgroup before a barrier: a
// workgroup-scope load (never the scalar cache)
__device__ __forceinline__ int32_t ld_flag(const int32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

template <int NQ>
__global__ __launch_bounds__(NQ * kWG) void k_solve_fused(PcgArgs<double> a, OpArgs<double> op, FusedArgs f) {
    const int32_t b = blockIdx.x;
    int32_t *si = a.sysi + b * kSysStride;
    double *sd = a.sysd + b * kSysStride;
    if (threadIdx.x == 0) {  // k_sys_reset
        for (int k = 0; k < kSysStride; ++k) {
            si[k] = 0;
            sd[k] = 0.0;
        }
        si[SI_ACTIVE] = 1;
        si[SI_CONV] = -1;
    }
    __syncthreads();
    const int32_t nvb = (a.N + kWG - 1) / kWG;              // k_outer_update's blocks
    const int32_t nug = (a.nblk + kUpdRB - 1) / kUpdRB;     // k_pcg_update's row-block groups
    constexpr int NT = NQ * kWG;
    const int32_t q = threadIdx.x / kWG;  // this thread's row block of each group of NQ
    int32_t itsum = 0, itmax = 0, o = 0;
    for (; o < f.max_outer; ++o) {
        // pcg<double>: the first step to 0.5 rtol, later ones to inner_rtol
        const double *rhs = o == 0 ? f.rhs : f.r64;
        for (int32_t rb = 0; rb < a.nblk; rb += NQ) pcg_init_rows<double, NQ>(a, rhs, rb + q, b);
        __syncthreads();
        pcg_tol_sys<double, NT>(a, o == 0 ? 0.5 * f.rtol : f.inner_rtol, o > 0 && f.adaptive ? f.rtol : 0.0, f.etol,
                                b);
        __syncthreads();
        red_rzrr_sys<double, NT>(a, 0, b);
        __syncthreads();
        int32_t it = 0;
        bool fin = false;
        for (; it < f.max_iter; ++it) {
            for (int32_t rb = 0; rb < a.nblk; rb += NQ) {
                if (it == 0)
                    pcg_spmv_rows<double, true, false, NQ>(a, it, 0, rb + q, b);
                else
                    pcg_spmv_rows<double, false, false, NQ>(a, it, 0, rb + q, b);
            }
            __syncthreads();
            if (ld_flag(si + SI_CONV) >= 0 || !ld_flag(si + SI_ACTIVE)) {
                fin = true;
                break;
            }
            red_pq_sys<double, NT>(a, it & 1, b);
            __syncthreads();
            for (int32_t g = 0; g < nug; g += NQ) pcg_update_rows<double, NQ>(a, it, g + q, b);
            __syncthreads();
            if (!ld_flag(si + SI_ACTIVE)) {  // breakdown / divergence / stagnation
                fin = true;
                break;
            }
            red_rzrr_sys<double, NT>(a, (it + 1) & 1, b);
            __syncthreads();
        }
        if (!fin) {  // the check launch after max_iter (SI_CONV of a system converged there)
            for (int32_t rb = 0; rb < a.nblk; rb += NQ) pcg_spmv_rows<double, false, false, NQ>(a, it, 0, rb + q, b);
            __syncthreads();
        }
        // this inner solve's iterations, counted as pcg() counts them
        const int32_t c = ld_flag(si + SI_CONV);
        const int32_t its = c >= 0 ? c
                                   : (ld_flag(si + SI_FAILED) && ld_flag(si + SI_FAIL_WHY) != FW_MAXITER
                                          ? ld_flag(si + SI_FAIL_IT) + 1
                                          : it);
        itsum += its;
        itmax = max(itmax, its);
        const RedArgs rdx{1, 0, nvb, a.N};
        for (int32_t blk = 0; blk < nvb; blk += NQ)
            outer_update_rows<double, NQ>(a.N, o == 0, a.x, a.sysi, f.x64, rdx, a.B, f.part_dx, blk + q, b);
        __syncthreads();
        for (int32_t rb = 0; rb < a.nblk; rb += NQ)
            residual_rows<NQ>(op, a.B, a.red, f.rhs, f.x64, a.sysi, f.r64, f.part_rr0, rb + q, b);
        __syncthreads();
        outer_check_sys<NT>(a.red, a.B, f.part_rr0, rdx, f.part_dx, o == 0, f.rtol, f.etol, a.sysd, a.sysi, b);
        __syncthreads();
        if (!ld_flag(si + SI_ACTIVE)) {
            ++o;
            break;
        }
    }
    if (threadIdx.x == 0) {
        keep_met(si);
        if (si[SI_ACTIVE] && sd[SD_REL] <= f.rtol) {  // k_mark_unconverged
            si[SI_ACTIVE] = 0;
        } else if (si[SI_ACTIVE]) {
            si[SI_FAILED] = 1;
            si[SI_ACTIVE] = 0;
            si[SI_FAIL_WHY] = FW_MAXITER;
        }
        si[SI_ITSUM] = itsum;
        si[SI_ITMAX] = itmax;
        sd[SD_OUTER] = (double)o;
    }
}

}  // namespace

int32_t xcd_batch_cap_host(int64_t nblk, int32_t grp) { return xcd_batch_cap(nblk, grp); }

void mesh_join_prep(mof_mesh *m, bool take_error) {
    if (!m) return;
    std::lock_guard<std::mutex> lk(m->prep_mu);
    if (m->prep.valid()) {
        try {
            m->prep.get();
        } catch (...) {
            m->prep_err = std::current_exception();
        }
    }
    if (take_error && m->prep_err) {
        std::exception_ptr e = m->prep_err;
        m->prep_err = nullptr;
        std::rethrow_exception(e);
    }
}

int32_t grid_batch_cap(const mof_mesh *m) {
    const int64_t per = (m->pat.sell_nb() + kWG - 1) / kWG;  // k_assemble_* / k_tri blocks per system
    return std::min(xcd_batch_cap(per, kGrpAsm), xcd_batch_cap(m->ws.nblk > 0 ? m->ws.nblk : per, kGrpSpmv));
}

double spmv_launch_bytes(const mof_mesh *m, uint32_t precision, int32_t active) {
    // SURVEY.md 8(d)'s algorithmic bytes of a batched CSR SpMV: per system the
    // nnz values, one read of x and one write of y (R = 2N rows); shared by
    // the launch: the nnz column indices and the R + 1 row pointers,
    //   B nnz s_v + 4 nnz + 4 (R + 1) + B R (s_x + s_y),  nnz = 4 nblocks.
    // (The kernel's own traffic differs both ways: it reads only the diagonal
    // and upper blocks with the symmetric reads, and it also updates q, p and
    // x; bench.py reports that figure next to this one.)
    const double nnz = 4.0 * m->pat.nblocks(), R = 2.0 * m->N;
    const double sv = precision == MOF_PREC_MIXED ? 4.0 : 8.0;
    return active * (nnz * sv + R * 2 * sv) + 4.0 * nnz + 4.0 * (R + 1);
}

void ensure_workspace(mof_mesh *m, int32_t B, uint32_t precision) {
    Workspace &w = m->ws;
    const int64_t N = m->N, snb = m->pat.sell_nb();
    const int32_t cap = std::max(B, w.cap);
    // the materialised A of the requested precision (SELL padding stays zero);
    // an A of the other precision is kept only if it already exists
    auto need_A = [&](auto &arr, bool wanted) {
        const size_t n = (size_t)(4 * snb * cap);
        if ((wanted || arr.n > 1) && arr.n < n) {
            arr.alloc(n);
            arr.zero(m->stream);
        }
    };
    need_A(w.A32, precision == MOF_PREC_MIXED);
    need_A(w.A64, precision == MOF_PREC_F64);
    if (w.cap >= B) {
        MOF_HIP(hipStreamSynchronize(m->stream));
        return;
    }
    w.cap = B;
    w.nblk = (int32_t)((N + kRowsPerWG - 1) / kRowsPerWG);
    // the per-triangle term arrays are sized on first use (ensure_tri_terms)
    w.u64.release();
    w.u32.release();
    w.fc.release();
    w.dinv64.alloc(4 * N * B);
    w.dinv32.alloc(4 * N * B);
    w.rhs.alloc(2 * N * B);
    w.x64.alloc(2 * N * B);
    w.r64.alloc(2 * N * B);
    w.vx.alloc(2 * N * B);
    w.vr.alloc(2 * N * B);
    w.vz.alloc(2 * N * B);
    w.vp.alloc(2 * N * B);
    w.vq.alloc(2 * N * B);
    w.part_pq.alloc(2 * (size_t)w.nblk * B);  // by iteration parity
    w.part_rzrr.alloc((size_t)4 * w.nblk * B);
    w.sc.alloc((size_t)6 * B);
    w.sc.zero(m->stream);
    w.part_rr0.alloc((size_t)2 * w.nblk * B);
    if (m->res_lds.used) w.res_spart.alloc((size_t)2 * m->pat.nslices * B);
    w.part_dx.alloc((size_t)2 * ((N + kWG - 1) / kWG) * B);
    w.sysd.alloc((size_t)kSysStride * B);
    w.sysi.alloc((size_t)kSysStride * B);
    w.smap.alloc((size_t)B);
    w.dt.alloc(B);
    w.Ibuf.alloc(2 * N * B);
    w.Iint.alloc(2 * N * B);
    w.Vbuf.alloc(2 * N * B);
    if (m->h_cap < B) {
        if (m->h_sysi) (void)hipHostFree(m->h_sysi);
        if (m->h_sysd) (void)hipHostFree(m->h_sysd);
        m->h_sysi = nullptr;
        m->h_sysd = nullptr;
        MOF_HIP(hipHostMalloc((void **)&m->h_sysi, sizeof(int32_t) * kSysStride * B, 0));
        MOF_HIP(hipHostMalloc((void **)&m->h_sysd, sizeof(double) * kSysStride * B, 0));
        m->h_cap = B;
    }
    MOF_HIP(hipStreamSynchronize(m->stream));
}

// The fused solve covers the fp64 solve of a whole batch from x = 0 with a
// stored u64 (the fp64 path's residual); auto (sp.fused < 0) on meshes of at
// most kFusedMaxBlk row blocks (4096 vertices), where the eager path is
// launch-bound.
constexpr int32_t kFusedMaxBlk = 16;
bool fused_eligible(const mof_mesh *m, const SolveParams &sp, const uint8_t *only) {
    if (sp.fused == 0 || only || sp.precision != MOF_PREC_F64 || sp.amg || sp.fail_at_max_iter) return false;
    if (m->ws.u64_stale || !m->ws.u64.p || m->n_own != m->N) return false;
    if (sp.fused > 0) return true;
    return m->ws.nblk <= kFusedMaxBlk;
}

// Row blocks the fused solve's workgroup runs side by side (groups of 256
// threads)
int fused_quarters(int32_t nblk) {
    return nblk >= 4 ? 4 : (nblk >= 2 ? 2 : 1);
}

int64_t solve_batch(mof_mesh *m, int32_t B, const SolveParams &sp, hipStream_t s, int32_t *outer,
                    int32_t *max_iters, SpmvTiming *timing, const uint8_t *only) {
    SpmvTiming *tm = sp.time_spmv ? timing : nullptr;
    Workspace &w = m->ws;
    if (fused_eligible(m, sp, only)) {
        // the whole solve in one launch (k_solve_fused), bit-identical to the
        // eager loop (refine)
        PcgArgs<double> a = make_args<double>(m, B, make_mat<double>(m, w.A64.p), w.dinv64.p);
        a.stall = sp.stall;
        const FusedArgs fa{w.rhs.p, w.x64.p,   w.r64.p,     w.part_rr0.p, w.part_dx.p,
                           sp.rtol, sp.inner_rtol, sp.etol,     sp.max_iter, sp.max_outer,
                           sp.adaptive_inner ? 1 : 0};
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (tm) {
            if (m->spmv_events.size() < 2) {
                const size_t old_n = m->spmv_events.size();
                m->spmv_events.resize(64);
                for (size_t q = old_n; q < m->spmv_events.size(); ++q) MOF_HIP(hipEventCreate(&m->spmv_events[q]));
            }
            e0 = m->spmv_events[0];
            e1 = m->spmv_events[1];
        }
        // row blocks side by side: NQ groups of 256 threads per workgroup
        const int nq = fused_quarters(m->ws.nblk);
        auto kf = nq >= 4 ? k_solve_fused<4> : (nq == 2 ? k_solve_fused<2> : k_solve_fused<1>);
        if (tm)
            hipExtLaunchKernelGGL(kf, dim3((unsigned)B), dim3(nq * kWG), 0, s, e0, e1, 0, a, op64(m), fa);
        else
            hipLaunchKernelGGL(kf, dim3((unsigned)B), dim3(nq * kWG), 0, s, a, op64(m), fa);
        MOF_HIP(hipGetLastError());
        fetch_flags(m, B, s);
        int64_t iters = 0;
        int32_t o = 0;
        for (int32_t b = 0; b < B; ++b) {
            const int32_t *si = m->h_sysi + b * kSysStride;
            iters += si[SI_ITSUM];
            *max_iters = std::max(*max_iters, si[SI_ITMAX]);
            o = std::max(o, (int32_t)m->h_sysd[b * kSysStride + SD_OUTER]);
        }
        *outer = o;
        if (tm) {
            float ms = 0.f;
            MOF_HIP(hipEventElapsedTime(&ms, e0, e1));
            tm->fused_launches++;
            tm->ms_fused += ms;
        }
        return iters;
    }
    return sp.precision == MOF_PREC_MIXED ? refine<float>(m, nullptr, B, sp, s, outer, max_iters, tm, only)
                                          : refine<double>(m, nullptr, B, sp, s, outer, max_iters, tm, only);
}

// The domain-decomposed solve (mof_dd.h): the same loop over d's local parts.
int64_t solve_batch_dd(mof_dd *d, int32_t B, const SolveParams &sp, hipStream_t s, int32_t *outer,
                       int32_t *max_iters, const uint8_t *only) {
    return sp.precision == MOF_PREC_MIXED ? refine<float>(nullptr, d, B, sp, s, outer, max_iters, nullptr, only)
                                          : refine<double>(nullptr, d, B, sp, s, outer, max_iters, nullptr, only);
}

double bench_spmv(mof_mesh *m, uint32_t precision, int32_t B, int32_t reps, hipStream_t s,
                  double *bytes) {
    Workspace &w = m->ws;
    MOF_REQUIRE(B >= 1 && B <= w.cap, "bench batch exceeds the workspace of the last solve");
    hipEvent_t e0, e1;
    MOF_HIP(hipEventCreate(&e0));
    MOF_HIP(hipEventCreate(&e1));
    *bytes = spmv_launch_bytes(m, precision, B);
    const dim3 gx(xcd_grid(w.nblk, B, kGrpSpmv));
    auto launch = [&]() {
        if (precision == MOF_PREC_MIXED) {
            PcgArgs<float> a = make_args<float>(m, B, make_mat<float>(m, w.A32.p), w.dinv32.p);
            spmv_kernel(a, false)<<<spmv_grid(a), spmv_wg<float>(), 0, s>>>(a, 1, kForce);
        } else {
            PcgArgs<double> a = make_args<double>(m, B, make_mat<double>(m, w.A64.p), w.dinv64.p);
            k_pcg_spmv<double, false><<<gx, spmv_wg<double>(), 0, s>>>(a, 1, kForce);
        }
    };
    for (int r = 0; r < 3; ++r) launch();
    MOF_HIP(hipEventRecord(e0, s));
    for (int r = 0; r < reps; ++r) launch();
    MOF_HIP(hipEventRecord(e1, s));
    MOF_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    MOF_HIP(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return ms / reps;
}


// Host check of the XCD order (tests, via mof_xcd_map_check): every
// (row block, system) pair is visited by exactly one workgroup of the grid.
bool xcd_map_covers(int32_t nblk, int32_t B, int32_t grp) {
    if (nblk < 1 || B < 1) return false;
    std::vector<uint8_t> hit((size_t)nblk * B, 0);
    const int64_t W = xcd_grid(nblk, B, grp);
    for (int64_t w = 0; w < W; ++w) {
        int32_t rb, b;
        if (!xcd_map_w((int32_t)w, nblk, B, rb, b, grp)) continue;
        if (rb < 0 || b < 0 || hit[(size_t)b * nblk + rb]++) return false;
    }
    for (uint8_t h : hit)
        if (h != 1) return false;
    return true;
}

namespace {

struct PcgDeviceGuard {
    int prev = 0;
    explicit PcgDeviceGuard(int d) {
        (void)hipGetDevice(&prev);
        MOF_HIP(hipSetDevice(d));
    }
    ~PcgDeviceGuard() { (void)hipSetDevice(prev); }
};

// the handle's per-system flags and scalars (device and host mirror) replaced
// for one test solve and put back
struct SysSwap {
    mof_mesh *m;
    int32_t B;
    std::vector<int32_t> si;
    std::vector<double> sd;
    std::vector<int32_t> hsi;
    std::vector<double> hsd;
    SysSwap(mof_mesh *mm, int32_t b, const uint8_t *active)
        : m(mm), B(b), si((size_t)b * kSysStride), sd((size_t)b * kSysStride) {
        Workspace &w = m->ws;
        MOF_HIP(hipMemcpy(si.data(), w.sysi.p, si.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        MOF_HIP(hipMemcpy(sd.data(), w.sysd.p, sd.size() * sizeof(double), hipMemcpyDeviceToHost));
        hsi.assign(m->h_sysi, m->h_sysi + si.size());
        hsd.assign(m->h_sysd, m->h_sysd + sd.size());
        std::vector<int32_t> now(si.size(), 0);
        for (int32_t k = 0; k < B; ++k) {
            now[(size_t)k * kSysStride + SI_CONV] = -1;
            now[(size_t)k * kSysStride + SI_ACTIVE] = !active || active[k];
        }
        std::copy(now.begin(), now.end(), m->h_sysi);  // pcg() reads the mirror for the systems to run
        MOF_HIP(hipMemcpy(w.sysi.p, now.data(), now.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    ~SysSwap() {
        Workspace &w = m->ws;
        (void)hipMemcpy(w.sysi.p, si.data(), si.size() * sizeof(int32_t), hipMemcpyHostToDevice);
        (void)hipMemcpy(w.sysd.p, sd.data(), sd.size() * sizeof(double), hipMemcpyHostToDevice);
        std::copy(hsi.begin(), hsi.end(), m->h_sysi);
        std::copy(hsd.begin(), hsd.end(), m->h_sysd);
    }
};

// ---- what mof_test_pcg_inner and mof_dd_test_pcg_inner share ----

// a mesh of the hook holds the last solve's operator of V for B systems (and a built multigrid)
template <typename V>
void hook_require(const mof_mesh *m, int32_t B, bool amg) {
    const Workspace &w = m->ws;
    const size_t need = 4 * (size_t)m->pat.sell_nb() * B;
    MOF_REQUIRE(B >= 1 && B <= w.cap && w.nblk > 0, "the handle's (a part's) last batch had fewer systems");
    if constexpr (sizeof(V) == 4)
        MOF_REQUIRE(w.A32.n >= need, "no fp32 operator: the last solve was not mixed-precision");
    else
        MOF_REQUIRE(w.A64.n >= need, "no fp64 operator: the last solve was not an fp64 one");
    if (amg) {
        MOF_REQUIRE(m->amg && amg_levels(m) >= 2, "the handle (a part) has no built multigrid");
        MOF_REQUIRE(B <= amg_capacity(m), "the multigrid's storage holds fewer systems");
    }
}

// the SolveParams of a hook's one inner solve
template <typename V>
SolveParams hook_params(bool amg, int32_t max_iter, double rtol, double etol) {
    SolveParams sp{};
    sp.precision = sizeof(V) == 4 ? MOF_PREC_MIXED : MOF_PREC_F64;
    sp.block_jacobi = true;
    sp.time_spmv = false;
    sp.amg = amg;
    sp.max_iter = max_iter;
    sp.max_outer = 1;
    sp.rtol = rtol;
    sp.inner_rtol = rtol;
    sp.etol = etol;
    sp.stall = amg ? kPcgStall : 0;
    sp.fail_at_max_iter = false;
    return sp;
}

// before the solve: the sentinel word in every mesh's five vectors and
// smoother x0; partial records of systems that never run, and of workgroups
// past a part's own count, read as zero
template <typename V>
void hook_prepare(const Parts<V> &p, bool amg, const uint32_t *sentinel, hipStream_t s) {
    for (mof_mesh *m : p.mesh) {
        Workspace &w = m->ws;
        const size_t nv = (size_t)m->N * p.B;
        if (sentinel) {
            for (DevArray<double> *a : {&w.vx, &w.vr, &w.vz, &w.vp, &w.vq})
                MOF_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(a->p), (int)*sentinel,
                                          2 * nv * sizeof(V) / 4, s));
            if (amg) MOF_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(amg_fine(m).x0), (int)*sentinel, nv, s));
        }
        MOF_HIP(hipMemsetAsync(w.sc.p, 0, sizeof(double) * 6 * p.B, s));
    }
    const size_t rec = (size_t)p.P * p.B * p.nmax;
    MOF_HIP(hipMemsetAsync(p.part_pq, 0, sizeof(double) * 2 * rec, s));
    MOF_HIP(hipMemsetAsync(p.part_rzrr, 0, sizeof(double) * 4 * rec, s));
}

void hook_get(void *dst, size_t at, const void *src, size_t bytes) {
    if (dst) MOF_HIP(hipMemcpy(static_cast<char *>(dst) + at, src, bytes, hipMemcpyDeviceToHost));
}

// after the solve: both slots' scalars as the kernels form them, k_red_rzrr's
// and k_red_pq's reduction (reduce_sys) of the partial records the solve left
// (all parts'), for every system, by the first mesh; scal[slot][b] = {r.z, |r|^2, p.q}
template <typename V>
void hook_scalars(PcgArgs<V> a, int32_t B, hipStream_t s, double *scal) {
    a.sm = sys_all(B);
    for (int32_t slot = 0; slot < 2; ++slot) {
        k_red_rzrr<V><<<dim3((unsigned)B), kWG, 0, s>>>(a, slot);
        k_red_pq<V><<<dim3((unsigned)B), kWG, 0, s>>>(a, slot);
    }
    MOF_HIP(hipGetLastError());
    MOF_HIP(hipStreamSynchronize(s));
    if (!scal) return;
    std::vector<double> sc((size_t)6 * B);
    hook_get(sc.data(), 0, a.sc, sizeof(double) * 6 * B);
    for (int32_t slot = 0; slot < 2; ++slot)
        for (int32_t b = 0; b < B; ++b) {
            double *o = scal + 3 * ((size_t)slot * B + b);
            o[0] = sc[2 * ((size_t)slot * B + b)];
            o[1] = sc[2 * ((size_t)slot * B + b) + 1];
            o[2] = sc[(size_t)4 * B + (size_t)slot * B + b];
        }
}

// where a hook copies the meshes' state to (null: skipped), one mesh after the other
struct HookOut {
    void *x, *r, *z, *p, *q;
    int32_t *sysi;
    double *sysd;
    void *dinv, *A;
    size_t ov = 0, os = 0, od = 0, oa = 0;  // bytes of vectors, rows of sysi / sysd, bytes of dinv, of A so far
};
// zh: z holds a bf16 pair per vertex
template <typename V>
void hook_read(mof_mesh *m, int32_t B, bool amg, bool zh, int32_t a_system, HookOut &o) {
    const Workspace &w = m->ws;
    const size_t nv = (size_t)m->N * B, snb = (size_t)m->pat.sell_nb(), vb = sizeof(V) * 2 * nv;
    hook_get(o.x, o.ov, w.vx.p, vb);
    hook_get(o.r, o.ov, w.vr.p, vb);
    hook_get(o.z, o.ov, w.vz.p, zh ? sizeof(uint32_t) * nv : vb);
    hook_get(o.p, o.ov, w.vp.p, vb);
    hook_get(o.q, o.ov, w.vq.p, vb);
    o.ov += vb;
    hook_get(o.sysi, o.os * sizeof(int32_t), w.sysi.p, sizeof(int32_t) * kSysStride * B);
    hook_get(o.sysd, o.os * sizeof(double), w.sysd.p, sizeof(double) * kSysStride * B);
    o.os += (size_t)kSysStride * B;
    if (!amg) hook_get(o.dinv, o.od, ws_dinv<V>(w), sizeof(V) * 4 * nv);
    o.od += sizeof(V) * 4 * nv;
    if (a_system >= 0) hook_get(o.A, o.oa, ws_A<V>(w) + 4 * snb * (size_t)a_system, sizeof(V) * 4 * snb);
    o.oa += sizeof(V) * 4 * snb;
}

// mof_test_pcg_inner for one working type
template <typename V>
void test_pcg_inner(mof_mesh *m, int32_t B, const double *rhs, double rtol, double outer_rtol, double etol, bool amg,
                    int32_t max_iter, const uint8_t *active, int32_t *hint2, const uint32_t *sentinel, void *x,
                    void *r, void *z, void *p, void *q, uint32_t *x0, double *scal, int32_t *sysi, double *sysd,
                    void *dinv, int32_t a_system, void *A, int32_t *meta) {
    constexpr bool f32 = sizeof(V) == 4;
    Workspace &w = m->ws;
    const size_t nv = (size_t)m->N * B;
    hook_require<V>(m, B, amg);
    MOF_REQUIRE(m->n_own == m->N, "a decomposed part's handle");
    MOF_REQUIRE(max_iter >= 0, "negative iteration cap");
    MOF_REQUIRE(!amg || f32, "the multigrid preconditions the fp32 inner solve only");
    MOF_REQUIRE(a_system < B, "bad system to read back");
    hipStream_t s = m->stream;
    MOF_HIP(hipStreamSynchronize(s));
    DevArray<double> drhs;
    drhs.alloc(2 * nv);
    MOF_HIP(hipMemcpy(drhs.p, rhs, sizeof(double) * 2 * nv, hipMemcpyHostToDevice));
    SysSwap swap(m, B, active);
    Parts<V> parts(m, nullptr, B);
    hook_prepare(parts, amg, sentinel, s);
    const SolveParams sp = hook_params<V>(amg, max_iter, rtol, etol);
    parts.fill_args(amg, sp.stall);
    std::vector<int32_t> hint(2 * kBulkHint, 0);
    if (hint2) {
        hint[0] = hint2[0];
        hint[kBulkHint] = hint2[1];
    }
    int32_t max_iters = 0;
    const double *drhs_p = drhs.p;
    const int64_t total = pcg<V>(parts, &drhs_p, rtol, sp, s, &max_iters, nullptr, hint.data(), amg, outer_rtol, etol);
    hook_scalars(parts.args[0], B, s, scal);
    const bool zh = f32 && amg && amg_fine(m).regular;
    HookOut out{x, r, z, p, q, sysi, sysd, dinv, A};
    hook_read<V>(m, B, amg, zh, a_system, out);
    if (amg) hook_get(x0, 0, amg_fine(m).x0, sizeof(uint32_t) * nv);
    if (hint2) {
        hint2[0] = hint[0];
        hint2[1] = hint[kBulkHint];
    }
    if (meta) {
        const int32_t v[8] = {zh,
                              m->sym_reads,
                              parts.args[0].mat.sell_idx != nullptr,
                              w.nblk <= kSelfRedBlk,
                              w.nblk,
                              (int32_t)std::min<int64_t>(total, INT32_MAX),
                              max_iters,
                              kSysStride};
        std::copy(v, v + 8, meta);
    }
}

// mof_dd_test_pcg_inner for one working type
template <typename V>
void test_pcg_dd_inner(mof_dd *d, int32_t B, const double *rhs, double rtol, bool amg, int32_t max_iter,
                       const uint32_t *sentinel, void *x, void *r, void *z, void *p, void *q, int32_t *sysi,
                       double *sysd, void *dinv, int32_t a_system, void *A, double *part_rzrr, double *part_pq,
                       double *scal, int32_t *meta) {
    constexpr bool f32 = sizeof(V) == 4;
    MOF_REQUIRE(d->rank < 0, "an in-process handle only");
    MOF_REQUIRE(B >= 1 && B <= d->cap && d->nmax > 0, "the handle's last batch had fewer systems");
    MOF_REQUIRE(max_iter >= 0, "negative iteration cap");
    MOF_REQUIRE(!amg || f32, "the multigrid preconditions the fp32 inner solve only");
    MOF_REQUIRE(a_system < B, "bad system to read back");
    for (const mof_mesh *m : d->parts) hook_require<V>(m, B, amg);
    hipStream_t s = d->stream;
    MOF_HIP(hipStreamSynchronize(s));
    std::vector<std::unique_ptr<DevKeep>> keep;
    std::vector<std::unique_ptr<SysSwap>> swap;
    std::vector<const double *> drhs;
    size_t off = 0;
    for (mof_mesh *m : d->parts) {
        Workspace &w = m->ws;
        const size_t nv = (size_t)m->N * B;
        keep.emplace_back(new DevKeep(w.rhs.p, sizeof(double) * 2 * nv));
        MOF_HIP(hipMemcpy(w.rhs.p, rhs + off, sizeof(double) * 2 * nv, hipMemcpyHostToDevice));
        drhs.push_back(w.rhs.p);
        off += 2 * nv;
        swap.emplace_back(new SysSwap(m, B, nullptr));
    }
    Parts<V> parts(nullptr, d, B);
    hook_prepare(parts, amg, sentinel, s);
    const SolveParams sp = hook_params<V>(amg, max_iter, rtol, 0.0);
    parts.fill_args(amg, sp.stall);
    int32_t max_iters = 0, hint = 0;
    const int64_t total = pcg<V>(parts, drhs.data(), rtol, sp, s, &max_iters, nullptr, &hint, amg);
    hook_scalars(parts.args[0], B, s, scal);
    HookOut out{x, r, z, p, q, sysi, sysd, dinv, A};
    for (mof_mesh *m : d->parts) hook_read<V>(m, B, amg, false, a_system, out);
    const size_t rec = (size_t)d->P * B * d->nmax;
    hook_get(part_rzrr, 0, d->part_rzrr.p, sizeof(double) * 4 * rec);
    hook_get(part_pq, 0, d->part_pq.p, sizeof(double) * 2 * rec);
    if (meta) {
        const int32_t v[6] = {d->nmax, d->P, (int32_t)std::min<int64_t>(total, INT32_MAX), max_iters, kSysStride,
                              (int32_t)d->parts.size()};
        std::copy(v, v + 6, meta);
    }
}

}  // namespace

}  // namespace mof

// ---- test hooks (include/mof.h) ------------------------------------------------

int mof_io_guard(const std::function<void()> &f);  // mof_abi.cpp: status + mof_last_error

extern "C" {

int mof_test_pcg_inner(mof_mesh *m, int32_t B, const double *rhs, double rtol, double outer_rtol, double etol,
                       int32_t amg, uint32_t precision, int32_t max_iter, const uint8_t *active, int32_t *hint,
                       const uint32_t *sentinel, void *x, void *r, void *z, void *p, void *q, uint32_t *x0,
                       double *scal, int32_t *sysi, double *sysd, void *dinv, int32_t a_system, void *A,
                       int32_t *meta) {
    return mof_io_guard([&] {
        MOF_REQUIRE(m && rhs, "NULL argument");
        MOF_REQUIRE(precision == MOF_PREC_MIXED || precision == MOF_PREC_F64, "bad precision");
        mof::mesh_join_prep(m);
        mof::PcgDeviceGuard dg(m->device);
        if (precision == MOF_PREC_MIXED)
            mof::test_pcg_inner<float>(m, B, rhs, rtol, outer_rtol, etol, amg != 0, max_iter, active, hint, sentinel, x,
                                       r, z, p, q, x0, scal, sysi, sysd, dinv, a_system, A, meta);
        else
            mof::test_pcg_inner<double>(m, B, rhs, rtol, outer_rtol, etol, amg != 0, max_iter, active, hint, sentinel,
                                        x, r, z, p, q, x0, scal, sysi, sysd, dinv, a_system, A, meta);
    });
}

int mof_dd_test_pcg_inner(mof_dd *d, int32_t B, const double *rhs, double rtol, int32_t amg, uint32_t precision,
                          int32_t max_iter, const uint32_t *sentinel, void *x, void *r, void *z, void *p, void *q,
                          int32_t *sysi, double *sysd, void *dinv, int32_t a_system, void *A, double *part_rzrr,
                          double *part_pq, double *scal, int32_t *meta) {
    return mof_io_guard([&] {
        MOF_REQUIRE(d && rhs, "NULL argument");
        MOF_REQUIRE(precision == MOF_PREC_MIXED || precision == MOF_PREC_F64, "bad precision");
        mof::PcgDeviceGuard dg(d->device);
        if (precision == MOF_PREC_MIXED)
            mof::test_pcg_dd_inner<float>(d, B, rhs, rtol, amg != 0, max_iter, sentinel, x, r, z, p, q, sysi, sysd,
                                          dinv, a_system, A, part_rzrr, part_pq, scal, meta);
        else
            mof::test_pcg_dd_inner<double>(d, B, rhs, rtol, amg != 0, max_iter, sentinel, x, r, z, p, q, sysi, sysd,
                                           dinv, a_system, A, part_rzrr, part_pq, scal, meta);
    });
}

int mof_test_pcg_launches(int64_t *counts) {
    return mof_io_guard([&] {
        MOF_REQUIRE(counts, "NULL argument");
        for (int k = 0; k < mof::kPcKernels; ++k) counts[k] = mof::g_pcg_launches[k].load();
    });
}

int mof_test_outer_readback(mof_mesh *m, int32_t B, double *x64, double *r64, void *xin, int32_t xin_bytes,
                            int32_t *sysi, double *sysd) {
    return mof_io_guard([&] {
        MOF_REQUIRE(m, "mesh is NULL");
        mof::mesh_join_prep(m);
        mof::Workspace &w = m->ws;
        MOF_REQUIRE(B >= 1 && B <= w.cap, "the handle's last batch had fewer systems");
        MOF_REQUIRE(!xin || xin_bytes == 4 || xin_bytes == 8, "the inner x holds floats or doubles");
        mof::PcgDeviceGuard dg(m->device);
        MOF_HIP(hipStreamSynchronize(m->stream));
        const size_t nv = (size_t)m->N * B;
        auto get = [&](void *dst, const void *src, size_t bytes) {
            if (dst) MOF_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
        };
        get(x64, w.x64.p, sizeof(double) * 2 * nv);
        get(r64, w.r64.p, sizeof(double) * 2 * nv);
        get(xin, w.vx.p, (size_t)xin_bytes * 2 * nv);
        get(sysi, w.sysi.p, sizeof(int32_t) * mof::kSysStride * B);
        get(sysd, w.sysd.p, sizeof(double) * mof::kSysStride * B);
    });
}

}  // extern "C"
