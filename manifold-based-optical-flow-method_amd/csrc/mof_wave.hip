// mof_wave.hip -- wave speed on the mesh (mof_wave_speed, include/mof.h):
// the reference's S5_compute_wave_v.py, speed = (dX/dt) / |grad_M X| per vertex
// and frame, from phases (S5:60-123, 225-233) or amplitudes (S5:14-58).
//
// The spatial half (S5:136-191: per-triangle gradient, area-weighted vertex
// mean, projection on the tangent plane, components on e_i) is linear in X,
// so for a fixed mesh it is one sparse operator on the vertex adjacency the
// handle already holds in SELL-64:
//     (alpha, beta)_i = sum_j c_ij X_j,
//     c_ij^a = (sum_T area_T grad_w[T][b] . p_i^a) / sum_T area_T,
//     p_i^a  = (e_i^a - (e_i^a . n) n / (n . n)) / (e_i^a . e_i^a),  n = e_i^0 x e_i^1
// with T over the triangles holding i (corner a) and j (corner b), in the
// caller's triangle order (the block's cptr / clist terms). One double2 per
// SELL position, built once per handle (k_wave_coef).
//
// Per pass of frames [t0, t1): k_wave_gather brings the rows the pass needs
// into the internal vertex order, F frames interleaved per vertex (one 8F-byte
// gather serves the F frames of a thread); k_wave does the row product for F
// frames, the norm, the temporal stencil and the divide, and writes the
// requested outputs in the same interleaved internal order; k_wave_scatter
// takes them back to the caller's (T, N) rows. Both permutation kernels run
// over the caller's vertices, so their row-major side is coalesced and their
// permuted side moves whole 8F-byte pieces.
//
// Compiled without fp contraction: dX/dt follows numpy's rounding step by step.
#include <algorithm>
#include <cmath>

#include "mof_internal.h"
#include "mof_rowkern.h"

namespace mof {

// -D overrides for A/B builds (tools/build_variant.sh; profiles/wave/)
#ifndef MOF_WAVE_F
#define MOF_WAVE_F 4
#endif
#ifndef MOF_WAVE_U
#define MOF_WAVE_U 4
#endif
constexpr int kWaveF = MOF_WAVE_F;  // frames per thread of the hot kernel (even)
constexpr int kWaveU = MOF_WAVE_U;  // SELL slots per load batch
constexpr int32_t kGrpWave = 8;  // frame groups walked back to back per row block (xcd_map)
// auto frames_per_pass: at most this many (frame, vertex) values per pass --
// 88 MiB for the pass's rows in internal order and for each output, whatever
// T is, so that what one kernel of a pass writes is still in the memory-side
// cache when the next reads it (C3, T = 256: 0.737 ms per call in passes of
// 64 frames, 0.753 at 96, 0.78-0.79 at 128 and 204, 0.775 at 48)
constexpr int64_t kWavePassElems = (int64_t)11 << 20;

struct WaveState {
    DevArray<double2> coef;   // [sell_nb] (alpha, beta) coefficients, padding 0
    DevArray<double> Xint;    // [groups][N][F]: the pass's rows, internal order
    DevArray<double> oint[4]; // [groups][N][F] (grad_ab: [2]): the pass's outputs, internal order
    DevArray<double> Xin;     // host-pointer calls: the pass's rows of X, caller's order
    DevArray<double> out[4];  // host-pointer calls: speed, grad_norm, dXdt, grad_ab of a pass
    bool built = false;
};

namespace {

// One thread per vertex row: folds the row's blocks' terms into its SELL slots.
__global__ __launch_bounds__(kWG) void k_wave_coef(int32_t N, const int32_t *__restrict__ sell_off,
                                                   const int32_t *__restrict__ sell_blk,
                                                   const int32_t *__restrict__ cptr,
                                                   const int32_t *__restrict__ clist, const double *__restrict__ gw,
                                                   const double *__restrict__ area, const double *__restrict__ e,
                                                   double2 *__restrict__ coef) {
    const int32_t i = blockIdx.x * kWG + threadIdx.x;
    if (i >= N) return;
    const int32_t s = i >> 6, l = i & 63;
    const int32_t o = sell_off[s];
    const int32_t w = (sell_off[s + 1] - o) >> 6;
    // S5:173-191 as two vectors: alpha = v . p0, beta = v . p1
    const double *e0 = e + 6 * (int64_t)i, *e1 = e0 + 3;
    const double n[3] = {e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]};
    const double nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    const double n0 = (e0[0] * n[0] + e0[1] * n[1]) + e0[2] * n[2];
    const double n1 = (e1[0] * n[0] + e1[1] * n[1]) + e1[2] * n[2];
    const double q0 = (e0[0] * e0[0] + e0[1] * e0[1]) + e0[2] * e0[2];
    const double q1 = (e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2];
    double p0[3], p1[3];
    for (int d = 0; d < 3; ++d) {
        p0[d] = (e0[d] - n0 * n[d] / nn) / q0;
        p1[d] = (e1[d] - n1 * n[d] / nn) / q1;
    }
    // the vertex's area: its incident triangles are the diagonal block's terms (slot 0)
    double asum = 0.0;
    {
        const int32_t bd = sell_blk[o + l];
        for (int32_t q = cptr[bd]; q < cptr[bd + 1]; ++q) asum += area[clist[q] / 9];
    }
    for (int32_t t = 0; t < w; ++t) {
        const int64_t pos = (int64_t)o + t * kSlice + l;
        const int32_t blk = sell_blk[pos];
        if (blk < 0) continue;  // padding keeps the zero it was cleared to
        double ca = 0.0, cb = 0.0;
        for (int32_t q = cptr[blk]; q < cptr[blk + 1]; ++q) {
            const int32_t code = clist[q];
            const int32_t T = code / 9, b = code % 3;
            const double *g = gw + 9 * (int64_t)T + 3 * b;
            ca += area[T] * ((g[0] * p0[0] + g[1] * p0[1]) + g[2] * p0[2]);
            cb += area[T] * ((g[0] * p1[0] + g[1] * p1[1]) + g[2] * p1[2]);
        }
        coef[pos] = make_double2(ca / asum, cb / asum);
    }
}

// The pass's rows in internal order: group q holds frames t0 + (q - 1) F + f,
// f < F, so group 0 is the F frames before the pass and the last group the F
// after it (the temporal stencil's halo). Frames outside [lo, hi) -- not in X,
// or not needed -- are written as 0. Xsrc is frame lo's row. One thread per
// caller's vertex c: the reads of a frame's row are coalesced, the write is
// one 8F-byte piece at the vertex's internal place perm[c].
template <int F>
__global__ __launch_bounds__(kWG) void k_wave_gather(int32_t N, int32_t ngroups, int64_t t0, int64_t lo, int64_t hi,
                                                     const double *__restrict__ Xsrc,
                                                     const int32_t *__restrict__ perm, double *__restrict__ Xint) {
    const int32_t c = blockIdx.x * kWG + threadIdx.x;
    const int32_t q = blockIdx.y;
    if (c >= N || q >= ngroups) return;
    double v[F];
#pragma unroll
    for (int f = 0; f < F; ++f) {
        const int64_t t = t0 + ((int64_t)q - 1) * F + f;
        v[f] = (t >= lo && t < hi) ? Xsrc[(t - lo) * N + c] : 0.0;
    }
    double2 *dst = reinterpret_cast<double2 *>(Xint + ((int64_t)q * N + perm[c]) * F);
#pragma unroll
    for (int f = 0; f < F; f += 2) dst[f / 2] = make_double2(v[f], v[f + 1]);
}

// The pass's outputs back to the caller's rows: one thread per caller's
// vertex and group of F frames reads the vertex's 8F-byte pieces and writes
// frame by frame, coalesced. out*: frame t0's row of each output, or null.
struct WaveOut {
    const double *ispeed, *ignorm, *idxdt, *igab;  // [ng][N][F] ([2] for grad_ab), internal order
    double *speed, *gnorm, *dxdt;
    double2 *gab;
};
template <int F>
__global__ __launch_bounds__(kWG) void k_wave_scatter(int32_t N, int32_t ng, int64_t nframes,
                                                      const int32_t *__restrict__ perm, const WaveOut o) {
    const int32_t c = blockIdx.x * kWG + threadIdx.x;
    const int32_t g = blockIdx.y;
    if (c >= N || g >= ng) return;
    const int64_t src = ((int64_t)g * N + perm[c]) * F;
    const int64_t r0 = (int64_t)g * F;  // the group's first frame, counted from t0
    auto rows = [&](const double *in, double *out) {
        double v[F];
#pragma unroll
        for (int f = 0; f < F; f += 2) {
            const double2 w = *reinterpret_cast<const double2 *>(in + src + f);
            v[f] = w.x;
            v[f + 1] = w.y;
        }
#pragma unroll
        for (int f = 0; f < F; ++f)
            if (r0 + f < nframes) out[(r0 + f) * N + c] = v[f];
    };
    if (o.speed) rows(o.ispeed, o.speed);
    if (o.gnorm) rows(o.ignorm, o.gnorm);
    if (o.dxdt) rows(o.idxdt, o.dxdt);
    if (o.gab) {
        double2 v[F];
#pragma unroll
        for (int f = 0; f < F; ++f) v[f] = *reinterpret_cast<const double2 *>(o.igab + 2 * (src + f));
#pragma unroll
        for (int f = 0; f < F; ++f)
            if (r0 + f < nframes) o.gab[(r0 + f) * N + c] = v[f];
    }
}

struct WaveArgs {
    int32_t N, nblk, ng;  // vertices, 256-row blocks, frame groups of the pass
    int64_t T, t0;        // frames of the sequence, first frame of the pass
    double dt;
    const int32_t *sell_off, *sell_col;
    const double2 *coef;
    const double *Xint;
    // the pass's outputs [ng][N][F] in internal order (grad_ab: [2]), or null
    double *speed, *gnorm, *dxdt, *gab;
};

// np.mod(x + pi, 2 pi) - pi (S5:230) with numpy's float mod: C fmod, then
// + 2 pi when the remainder is non-zero and negative, +0 when it is zero
__device__ __forceinline__ double wrap_pi(double x) {
    const double pi = 3.141592653589793, two_pi = 6.283185307179586;
    double m = fmod(x + pi, two_pi);
    if (m != 0.0) {
        if (m < 0.0) m += two_pi;
    } else {
        m = 0.0;
    }
    return m - pi;
}

// One wave per SELL slice, one thread per (vertex row, group of F frames).
template <int F, bool PHASE>
__global__ __launch_bounds__(kWG) void k_wave(const WaveArgs a) {
    int32_t rb, g;
    if (!xcd_map(a.nblk, a.ng, rb, g, kGrpWave)) return;
    const int32_t i0 = rb * kWG + (int32_t)threadIdx.x;
    if ((i0 & ~63) >= a.N) return;  // the whole wave lies past the last slice
    const int32_t i = min(i0, a.N - 1);  // lanes past N repeat row N - 1 (same slice), unstored
    const int64_t N = a.N;
    const int32_t s = wave_slice(i), l = i & 63;
    const int32_t o = a.sell_off[s];
    const int32_t w = (a.sell_off[s + 1] - o) >> 6;
    const double *Xg = a.Xint + (int64_t)(g + 1) * N * F;   // the group's frames

    // Every slot of the slice, padding included: a padding position holds a
    // zero coefficient and the row's own column, so it adds 0 (or the NaN the
    // diagonal term gives anyway where X is not finite) and no lane needs a
    // mask. Whole batches of U slots first, all loads of a batch issued before
    // its first use; fma: the sums carry a tolerance, not numpy's rounding.
    double al[F], be[F];
#pragma unroll
    for (int f = 0; f < F; ++f) al[f] = be[f] = 0.0;
    auto slots = [&](int32_t ts, auto nu) {
        constexpr int U = decltype(nu)::value;
        double2 c[U];
        int32_t j[U];
        double x[U][F];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t pos = (int64_t)o + (ts + u) * kSlice + l;
            c[u] = a.coef[pos];
            j[u] = a.sell_col[pos];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const double *xp = Xg + (int64_t)j[u] * F;
#pragma unroll
            for (int f = 0; f < F; f += 2) {
                const double2 v = *reinterpret_cast<const double2 *>(xp + f);
                x[u][f] = v.x;
                x[u][f + 1] = v.y;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int f = 0; f < F; ++f) {
                al[f] = fma(c[u].x, x[u][f], al[f]);
                be[f] = fma(c[u].y, x[u][f], be[f]);
            }
    };
    int32_t ts = 0;
    for (; ts + kWaveU <= w; ts += kWaveU) slots(ts, std::integral_constant<int, kWaveU>{});
    for (; ts < w; ++ts) slots(ts, std::integral_constant<int, 1>{});

    // own-row values of frames tb - 1 .. tb + F (the neighbouring groups hold the ends)
    const int64_t tb = a.t0 + (int64_t)g * F;
    double xo[F + 2];
    xo[0] = a.Xint[((int64_t)g * N + i) * F + (F - 1)];
#pragma unroll
    for (int f = 0; f < F; ++f) xo[f + 1] = Xg[(int64_t)i * F + f];
    xo[F + 1] = a.Xint[((int64_t)(g + 2) * N + i) * F];
    // any frame t0 - F <= t < t0 + (ng + 1) F of the pass's rows
    auto xat = [&](int64_t t) {
        const int64_t r = t - a.t0 + F;
        return a.Xint[((r / F) * N + i) * F + (r % F)];
    };

    if (i0 >= a.N) return;
    double d[F], gn[F], sp[F];
#pragma unroll
    for (int f = 0; f < F; ++f) {
        // frames past the pass's end (the last group's tail) are computed from
        // the zero rows and never leave the workspace
        const int64_t t = tb + f;
        if constexpr (PHASE) {  // S5:60-77
            if (t == 0)
                d[f] = wrap_pi(xo[f + 2] - xo[f + 1]) / a.dt;
            else if (t == a.T - 1)
                d[f] = wrap_pi(xo[f + 1] - xo[f]) / a.dt;
            else
                d[f] = wrap_pi(xo[f + 2] - xo[f]) / (2.0 * a.dt);
        } else {  // np.gradient(X, axis=0, edge_order=2) / dt (S5:24)
            if (t == 0)
                d[f] = ((-1.5 * xo[f + 1] + 2.0 * xo[f + 2]) + -0.5 * xat(2)) / a.dt;
            else if (t == a.T - 1)
                d[f] = ((0.5 * xat(t - 2) + -2.0 * xo[f]) + 1.5 * xo[f + 1]) / a.dt;
            else
                d[f] = ((xo[f + 2] - xo[f]) / 2.0) / a.dt;
        }
        gn[f] = sqrt(al[f] * al[f] + be[f] * be[f]);
        sp[f] = d[f] / gn[f];
    }
    const int64_t q = ((int64_t)g * N + i) * F;
    auto put = [&](double *out, const double (&v)[F]) {
#pragma unroll
        for (int f = 0; f < F; f += 2) *reinterpret_cast<double2 *>(out + q + f) = make_double2(v[f], v[f + 1]);
    };
    if (a.speed) put(a.speed, sp);
    if (a.gnorm) put(a.gnorm, gn);
    if (a.dxdt) put(a.dxdt, d);
    if (a.gab) {
#pragma unroll
        for (int f = 0; f < F; ++f) *reinterpret_cast<double2 *>(a.gab + 2 * (q + f)) = make_double2(al[f], be[f]);
    }
}

}  // namespace

void wave_destroy(WaveState *w) { delete w; }

// The coefficient table of the handle (first use), on its own stream.
static WaveState *wave_state(mof_mesh *m) {
    if (!m->wave) m->wave = new WaveState();
    WaveState *W = m->wave;
    if (W->built) return W;
    const int64_t snb = m->pat.sell_nb();
    hipStream_t s = m->stream;
    MOF_REQUIRE(m->perm_d.n >= (size_t)m->N && m->sell_blk.n >= (size_t)snb && m->gw.n >= 9 * (size_t)m->M &&
                    m->e.n >= 6 * (size_t)m->N && m->area.n >= (size_t)m->M,
                "mesh handle holds no geometry");
    W->coef.alloc((size_t)snb);
    W->coef.zero(s);
    k_wave_coef<<<dim3((unsigned)((m->N + kWG - 1) / kWG)), kWG, 0, s>>>(
        m->N, m->sell_off.p, m->sell_blk.p, m->cptr.p, m->clist.p, m->gw.p, m->area.p, m->e.p, W->coef.p);
    MOF_HIP(hipGetLastError());
    MOF_HIP(hipStreamSynchronize(s));
    W->built = true;
    return W;
}

int32_t wave_auto_frames(int32_t N, int32_t T) {
    // whole sets of kGrpWave frame groups (the hot kernel's grid is padded to
    // them: 68 frames per pass measured 0.75 ms where 64 take 0.72), at least one group
    const int64_t set = (int64_t)kWaveF * kGrpWave;
    int64_t fpp = kWavePassElems / std::max(N, 1);
    fpp = fpp >= set ? fpp / set * set : std::max<int64_t>(kWaveF, fpp / kWaveF * kWaveF);
    return (int32_t)std::min<int64_t>(fpp, std::max(T, 1));
}

// X (T, N) and the outputs in the caller's order: device pointers (dev_io) or
// host pointers staged pass by pass. fpp > 0 frames per pass.
void wave_speed(mof_mesh *m, const double *X, int32_t T, double dt, bool phase, int32_t fpp, bool dev_io,
                hipStream_t s, double *speed, double *gnorm, double *dxdt, double *gab) {
    constexpr int F = kWaveF;
    WaveState *W = wave_state(m);
    const int64_t N = m->N;
    fpp = std::min(fpp, T);
    const int32_t ngmax = (fpp + F - 1) / F;
    const size_t need = (size_t)(ngmax + 2) * F * N;
    if (W->Xint.n < need) W->Xint.alloc(need);
    double *outs[4] = {speed, gnorm, dxdt, gab};
    const int64_t ow[4] = {1, 1, 1, 2};
    for (int k = 0; k < 4; ++k)
        if (outs[k] && W->oint[k].n < (size_t)ngmax * F * N * ow[k]) W->oint[k].alloc((size_t)ngmax * F * N * ow[k]);
    if (!dev_io) {
        const size_t rows = (size_t)std::min<int64_t>(T, (int64_t)fpp + 4);
        if (W->Xin.n < rows * N) W->Xin.alloc(rows * N);
        for (int k = 0; k < 4; ++k)
            if (outs[k] && W->out[k].n < (size_t)fpp * N * ow[k]) W->out[k].alloc((size_t)fpp * N * ow[k]);
    }
    const int32_t nblk = (int32_t)((N + kWG - 1) / kWG);
    for (int64_t t0 = 0; t0 < T; t0 += fpp) {
        const int64_t t1 = std::min<int64_t>(T, t0 + fpp);
        // the rows the pass reads: one before and after it for the centred
        // differences, two where it holds an end of the sequence (edge_order 2)
        const int64_t lo = std::max<int64_t>(0, t0 - 2), hi = std::min<int64_t>(T, t1 + 2);
        const int32_t ng = (int32_t)((t1 - t0 + F - 1) / F);
        const double *Xsrc = X + lo * N;
        if (!dev_io) {
            MOF_HIP(hipMemcpyAsync(W->Xin.p, X + lo * N, sizeof(double) * (size_t)((hi - lo) * N),
                                   hipMemcpyHostToDevice, s));
            Xsrc = W->Xin.p;
        }
        k_wave_gather<F><<<dim3((unsigned)nblk, (unsigned)(ng + 2)), kWG, 0, s>>>((int32_t)N, ng + 2, t0, lo, hi, Xsrc,
                                                                                 m->perm_d.p, W->Xint.p);
        MOF_HIP(hipGetLastError());
        WaveArgs a;
        a.N = (int32_t)N;
        a.nblk = nblk;
        a.ng = ng;
        a.T = T;
        a.t0 = t0;
        a.dt = dt;
        a.sell_off = m->sell_off.p;
        a.sell_col = m->sell_col.p;
        a.coef = W->coef.p;
        a.Xint = W->Xint.p;
        double *po[4];
        for (int k = 0; k < 4; ++k) po[k] = !outs[k] ? nullptr : (dev_io ? outs[k] + t0 * N * ow[k] : W->out[k].p);
        a.speed = outs[0] ? W->oint[0].p : nullptr;
        a.gnorm = outs[1] ? W->oint[1].p : nullptr;
        a.dxdt = outs[2] ? W->oint[2].p : nullptr;
        a.gab = outs[3] ? W->oint[3].p : nullptr;
        const unsigned grid = xcd_grid(nblk, ng, kGrpWave);
        if (phase)
            k_wave<F, true><<<dim3(grid), kWG, 0, s>>>(a);
        else
            k_wave<F, false><<<dim3(grid), kWG, 0, s>>>(a);
        MOF_HIP(hipGetLastError());
        WaveOut wo;
        wo.ispeed = a.speed;
        wo.ignorm = a.gnorm;
        wo.idxdt = a.dxdt;
        wo.igab = a.gab;
        wo.speed = po[0];
        wo.gnorm = po[1];
        wo.dxdt = po[2];
        wo.gab = reinterpret_cast<double2 *>(po[3]);
        k_wave_scatter<F><<<dim3((unsigned)nblk, (unsigned)ng), kWG, 0, s>>>((int32_t)N, ng, t1 - t0, m->perm_d.p, wo);
        MOF_HIP(hipGetLastError());
        if (!dev_io) {
            for (int k = 0; k < 4; ++k)
                if (outs[k])
                    MOF_HIP(hipMemcpyAsync(outs[k] + t0 * N * ow[k], po[k],
                                           sizeof(double) * (size_t)((t1 - t0) * N * ow[k]), hipMemcpyDeviceToHost,
                                           s));
            // the staging buffers are reused by the next pass
            MOF_HIP(hipStreamSynchronize(s));
        }
    }
    MOF_HIP(hipStreamSynchronize(s));
}

}  // namespace mof
