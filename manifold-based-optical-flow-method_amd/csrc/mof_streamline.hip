// mof_streamline.hip -- streamlines on the mesh (mof_streamline_map,
// mof_streamlines, include/mof.h): the reference's S6_streamline.py.
//
// The reference starts a greedy vertex walk from every vertex of every frame
// (S6:17-37) and rescans the whole path at each step (S6:39-49). Its choice of
// the next vertex at vertex i depends on (field, i) alone, so the walks are
//   1. a successor map next[k][i] per field (k_stream_next), and
//   2. from each seed, s, next[s], next[next[s]], ... up to the first vertex
//      that is terminal or already on the path. Its length is 1 + the length
//      from next[s] off the cycles of next and the cycle's length on them:
//      pointer jumping over all vertices of a field at once (k_jump_*), or,
//      kept for comparison (-DMOF_STREAM_WALK=0), one walk per seed by
//      Brent's cycle finding (k_stream_walk). O(1) state per thread in both,
//      no visited set and no path rescanned.
//
// Successor (S6:63-77): with e1, e2 = e_i, n = e1 x e2 and, per neighbour j,
//   u_j = normalize(w - (w . n) n / (n . n)),  w = p_j - p_i,
//   d_j = (u_j0 V_i0 + u_j1 V_i1) + u_j2 V_i2,
// j* = argmax d_j, the smallest caller's id on equal maxima; i is terminal
// (next = -1) unless d_j* > 0. The u_j do not depend on the field: three
// doubles per SELL-64 slot, built once per handle (k_stream_dir) together with
// the slot's neighbour in the caller's ids and, where the boundary-edge test
// applies (i has fewer than 6 triangles and shares exactly one with j), that
// triangle. The test itself (S6:100-133) is restated as written: the
// reference passes vertex *indices* to position_diff_on_basis_with_origin, so
// its 2-D triangle has collinear corners up to rounding.
//
// Fields go through in passes of bounded size. The list-shaped result
// (mof_streamlines) is compacted per pass: block sums of the kept lines and
// their vertices (k_stream_count), their running offsets formed on the host
// (a few KB), and a second walk that writes the ids (k_stream_emit).
//
// Compiled without fp contraction: every product and sum rounds as numpy's.
#include <algorithm>
#include <climits>
#include <cmath>

#include "mof_internal.h"
#include "mof_rowkern.h"

namespace mof {

// -D override for A/B builds (tools/build_variant.sh; profiles/streamline/)
#ifndef MOF_STREAM_F
#define MOF_STREAM_F 4
#endif
#ifndef MOF_STREAM_WALK
#define MOF_STREAM_WALK 1
#endif
// the lengths: 1 pointer jumping over all vertices of a field at once, 0 one
// walk per seed (Brent's cycle finding); profiles/streamline/ has both
constexpr int kStreamWalk = MOF_STREAM_WALK;
constexpr int kStreamF = MOF_STREAM_F;  // fields per thread of k_stream_next: one read of a row's slots serves F fields
// auto fields per pass: at most this many (field, vertex) pairs -- 48 MiB of
// staged V and 8 MiB each of next, length and the five pointer-jumping arrays
// whatever K is, and still four resident waves per SIMD for the pointer chase
constexpr int64_t kStreamPassElems = (int64_t)2 << 20;
std::atomic<int> g_stream_pass_fields{0};  // tests only (mof_test_streamline_pass): fields per pass, 0 = auto

struct StreamState {
    DevArray<double> udir;    // [sell_nb][3] unit directions u_j, padding / diagonal 0
    DevArray<int32_t> nbr;    // [sell_nb] the slot's neighbour, caller's id; -1 padding / diagonal
    DevArray<int32_t> btri;   // [sell_nb] internal triangle of the slot's boundary-edge test, or -1
    DevArray<int32_t> inv;    // [N] internal vertex -> caller's id
    DevArray<double> Vin;     // host-pointer calls: the pass's fields
    DevArray<int32_t> nxt, len;  // [pass][N] the pass's map and lengths, caller's order
    DevArray<int32_t> jw[4];  // [pass][N] pointer jumping: the ping-pong (vertex, steps) arrays
    DevArray<int32_t> clen;   // [pass][N] pointer jumping: cycle length, 0 off the cycles
    DevArray<int64_t> bsum;   // [pass][blocks][2] kept lines / their vertices per block, then their offsets
    DevArray<int64_t> loff;   // the pass's line offsets
    DevArray<int32_t> lvtx;   // the pass's line vertices
    bool built = false;
};

namespace {

__device__ __forceinline__ double dot3(const double *a, const double *b) {
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

// One thread per vertex row: the row's unit directions, neighbours and
// boundary-edge triangles into its SELL slots.
template <bool F32P>
__global__ __launch_bounds__(kWG) void k_stream_dir(int32_t N, const int32_t *__restrict__ sell_off,
                                                    const int32_t *__restrict__ sell_col,
                                                    const int32_t *__restrict__ sell_blk,
                                                    const int32_t *__restrict__ cptr,
                                                    const int32_t *__restrict__ clist, const double *__restrict__ e,
                                                    const double *__restrict__ xyz, const int32_t *__restrict__ inv,
                                                    double *__restrict__ udir, int32_t *__restrict__ nbr,
                                                    int32_t *__restrict__ btri) {
    const int32_t i = blockIdx.x * kWG + threadIdx.x;
    if (i >= N) return;
    const int32_t s = i >> 6, l = i & 63;
    const int32_t o = sell_off[s];
    const int32_t w = (sell_off[s + 1] - o) >> 6;
    const double *e0 = e + 6 * (int64_t)i, *e1 = e0 + 3;
    const double n[3] = {e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]};
    const double nn = dot3(n, n);
    const double *pi = xyz + 3 * (int64_t)i;
    // the vertex's triangles are the diagonal block's terms (slot 0)
    const int32_t bd = sell_blk[o + l];
    const int32_t ncell = cptr[bd + 1] - cptr[bd];
    for (int32_t t = 1; t < w; ++t) {
        const int64_t pos = (int64_t)o + t * kSlice + l;
        const int32_t blk = sell_blk[pos];
        if (blk < 0) continue;  // padding keeps what it was cleared to
        const int32_t j = sell_col[pos];
        const double *pj = xyz + 3 * (int64_t)j;
        double v[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) v[d] = F32P ? (double)((float)pj[d] - (float)pi[d]) : pj[d] - pi[d];
        const double vn = dot3(v, n);
        double vt[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) vt[d] = v[d] - vn * n[d] / nn;
        const double len = sqrt(dot3(vt, vt));
#pragma unroll
        for (int d = 0; d < 3; ++d) udir[3 * pos + d] = vt[d] / len;
        nbr[pos] = inv[j];
        // the triangles holding i and j are the block's terms
        const int32_t q0 = cptr[blk], shared = cptr[blk + 1] - q0;
        btri[pos] = (ncell < 6 && shared == 1) ? clist[q0] / 9 : -1;
    }
}

// S6:100-129 for the triangle (A, B, C: caller's ids, the triangle's own
// corner order) that vertex ci shares with its chosen neighbour: true when
// inTri == 1. The positions are formed from differences of vertex ids, as
// the reference forms them.
__device__ bool boundary_edge_test(int32_t A, int32_t B, int32_t C, int32_t ci, const double *e0, const double *e1,
                                   const double *V) {
    if (A == ci) {
    } else if (B == ci) {
        B = A;
        A = ci;
    } else if (C == ci) {
        C = A;
        A = ci;
    }
    const double n[3] = {e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]};
    const double nn = dot3(n, n);
    auto posdiff = [&](int32_t from, int32_t to, double &u, double &v) {  // S6:173-182
        const double rel = (double)((int64_t)to - (int64_t)from);
        double p[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) p[d] = rel - rel * n[d] * n[d] / nn;
        u = dot3(p, e0);
        v = dot3(p, e1);
    };
    double bx, by, cx, cy;
    posdiff(A, B, bx, by);
    posdiff(C, A, cx, cy);
    const double cross = bx * cy - by * cx;  // clockwise (S6:204-219), a = (0, 0)
    if (cross < 0) {
        double t = bx;
        bx = cx;
        cx = t;
        t = by;
        by = cy;
        cy = t;
    } else if (!(cross > 0)) {
        return false;
    }
    const double px = dot3(V, e0) / dot3(e0, e0), py = dot3(V, e1) / dot3(e1, e1);  // express_vector_on_basis
    // inTri (S6:184-202): ab x ap, bc x bp, ca x cp all positive
    const double c0 = (bx - 0.0) * (py - 0.0) - (by - 0.0) * (px - 0.0);
    const double c1 = (cx - bx) * (py - by) - (cy - by) * (px - bx);
    const double c2 = (0.0 - cx) * (py - cy) - (0.0 - cy) * (px - cx);
    return c0 > 0 && c1 > 0 && c2 > 0;
}

struct NextArgs {
    int32_t N, K;  // vertices, fields of the pass
    const int32_t *sell_off, *nbr, *btri, *inv, *tri;
    const double *udir, *e;
    const double *V;   // [K][N][3] caller's order
    int32_t *next;     // [K][N] caller's order
    int32_t *len;      // [K][N] or null: 0 where the seed is skipped (V . V == 0), else 1
};

// One wave per SELL slice, one thread per (vertex row, group of F fields).
template <int F>
__global__ __launch_bounds__(kWG) void k_stream_next(const NextArgs a) {
    const int32_t i0 = blockIdx.x * kWG + (int32_t)threadIdx.x;
    if ((i0 & ~63) >= a.N) return;       // the whole wave lies past the last slice
    const int32_t i = min(i0, a.N - 1);  // lanes past N repeat row N - 1 (same slice), unstored
    const int32_t k0 = (int32_t)blockIdx.y * F;
    const int64_t N = a.N;
    const int32_t s = wave_slice(i), l = i & 63;
    const int32_t o = a.sell_off[s];
    const int32_t w = (a.sell_off[s + 1] - o) >> 6;
    const int32_t ci = a.inv[i];

    double V[F][3], best[F];
    int32_t bid[F], bpos[F];
    bool nan[F];
#pragma unroll
    for (int f = 0; f < F; ++f) {
        const bool on = k0 + f < a.K;
        const double *v = a.V + (((int64_t)(on ? k0 + f : k0)) * N + ci) * 3;
#pragma unroll
        for (int d = 0; d < 3; ++d) V[f][d] = v[d];
        best[f] = -INFINITY;
        bid[f] = INT_MAX;
        bpos[f] = -1;
        nan[f] = false;
    }
    // slot 0 is the row itself
    for (int32_t t = 1; t < w; ++t) {
        const int32_t pos = o + t * kSlice + l;
        const int32_t id = a.nbr[pos];
        const double *u = a.udir + 3 * (int64_t)pos;
        const double u0 = u[0], u1 = u[1], u2 = u[2];
        if (id < 0) continue;
#pragma unroll
        for (int f = 0; f < F; ++f) {
            const double d = (u0 * V[f][0] + u1 * V[f][1]) + u2 * V[f][2];
            // np.argmax stops at a NaN, and a NaN is not > 0: terminal
            nan[f] = nan[f] || d != d;
            if (d > best[f] || (d == best[f] && id < bid[f])) {
                best[f] = d;
                bid[f] = id;
                bpos[f] = pos;
            }
        }
    }
    if (i0 >= a.N) return;
    const double *e0 = a.e + 6 * (int64_t)i;
#pragma unroll
    for (int f = 0; f < F; ++f) {
        if (k0 + f >= a.K) break;
        bool ok = bpos[f] >= 0 && !nan[f] && best[f] > 0;
        if (ok) {
            const int32_t T = a.btri[bpos[f]];
            if (T >= 0) {
                const int32_t *tv = a.tri + 3 * (int64_t)T;
                ok = boundary_edge_test(a.inv[tv[0]], a.inv[tv[1]], a.inv[tv[2]], ci, e0, e0 + 3, V[f]);
            }
        }
        const int64_t q = (int64_t)(k0 + f) * N + ci;
        a.next[q] = ok ? bid[f] : -1;
        if (a.len) a.len[q] = ((V[f][0] * V[f][0] + V[f][1] * V[f][1]) + V[f][2] * V[f][2]) == 0.0 ? 0 : 1;
    }
}

// The vertices of the walk from s along nx (entries in [-1, N)): up to the
// first terminal exit, or tail + cycle by Brent's algorithm.
__device__ __forceinline__ int32_t walk_length(const int32_t *__restrict__ nx, int32_t s) {
    int32_t tort = s, hare = nx[s];
    uint32_t power = 1, lam = 1;
    int32_t cnt = 1;
    while (hare >= 0 && hare != tort) {
        if (power == lam) {
            tort = hare;
            power <<= 1;
            lam = 0;
        }
        hare = nx[hare];
        ++lam;
        ++cnt;
    }
    if (hare < 0) return cnt;
    tort = hare = s;
    for (uint32_t q = 0; q < lam; ++q) hare = nx[hare];
    int32_t mu = 0;
    while (tort != hare) {
        tort = nx[tort];
        hare = nx[hare];
        ++mu;
    }
    return mu + (int32_t)lam;
}

// One thread per (seed, field); len holds k_stream_next's 0 / 1.
__global__ __launch_bounds__(kWG) void k_stream_walk(int32_t N, const int32_t *__restrict__ next,
                                                     int32_t *__restrict__ len) {
    const int32_t c = blockIdx.x * kWG + threadIdx.x;
    if (c >= N) return;
    const int64_t row = (int64_t)blockIdx.y * N;
    if (len[row + c] == 0) return;
    len[row + c] = walk_length(next + row, c);
}

// ---- the lengths by pointer jumping (MOF_STREAM_WALK 1) --------------------
// length(i) = 1 + length(next(i)) off the cycles, the cycle's length on them:
// every vertex of a field at once, O(N log N) pointer steps per field where
// the walks from every seed take O(N x mean length).
//  1. R = ceil(log2 N) doublings of next: p = next^(2^R)(i) is -1 where the
//     walk ends at a terminal vertex, else a vertex on a cycle, and every
//     cycle vertex is such a p (next permutes a cycle);
//  2. those vertices are marked, and each walks its cycle until it meets a
//     smaller id (it gives up) or itself (it is the smallest: it walks once
//     more and writes the length to the whole cycle);
//  3. R doublings of (q, t) = (vertex reached, steps taken) that stop at the
//     roots -- cycle and terminal vertices -- give the tail, and the length
//     is t + the root's (a cycle's length, or 1).
// One thread per (vertex, field) everywhere, O(1) state, no path rescanned.

__global__ __launch_bounds__(kWG) void k_jump_double(int32_t N, const int32_t *__restrict__ src,
                                                     int32_t *__restrict__ dst) {
    const int32_t c = blockIdx.x * kWG + threadIdx.x;
    if (c >= N) return;
    const int64_t row = (int64_t)blockIdx.y * N;
    const int32_t j = src[row + c];
    dst[row + c] = j < 0 ? -1 : src[row + j];
}

__global__ __launch_bounds__(kWG) void k_jump_mark(int32_t N, const int32_t *__restrict__ p,
                                                   int32_t *__restrict__ clen) {
    const int32_t c = blockIdx.x * kWG + threadIdx.x;
    if (c >= N) return;
    const int64_t row = (int64_t)blockIdx.y * N;
    const int32_t j = p[row + c];
    if (j >= 0) clen[row + j] = -1;  // every writer writes the same mark
}

// clen: 0 off the cycles, non-zero (the mark, then the length) on them
__global__ __launch_bounds__(kWG) void k_jump_cycle(int32_t N, const int32_t *__restrict__ next, int32_t *clen) {
    const int32_t c = blockIdx.x * kWG + threadIdx.x;
    if (c >= N) return;
    const int64_t row = (int64_t)blockIdx.y * N;
    if (clen[row + c] == 0) return;
    const int32_t *nx = next + row;
    int32_t v = nx[c], n = 1;
    while (v > c && n <= N) {  // a cycle vertex's successors are cycle vertices: never -1, back within N steps
        v = nx[v];
        ++n;
    }
    if (v != c) return;  // a smaller id on the cycle: that vertex writes
    v = c;
    do {
        clen[row + v] = n;
        v = nx[v];
    } while (v != c);
}

__global__ __launch_bounds__(kWG) void k_jump_tail_init(int32_t N, const int32_t *__restrict__ next,
                                                        const int32_t *__restrict__ clen, int32_t *__restrict__ q,
                                                        int32_t *__restrict__ t) {
    const int32_t c = blockIdx.x * kWG + threadIdx.x;
    if (c >= N) return;
    const int64_t x = (int64_t)blockIdx.y * N + c;
    const int32_t j = next[x];
    const bool root = j < 0 || clen[x] != 0;
    q[x] = root ? c : j;
    t[x] = root ? 0 : 1;
}

__global__ __launch_bounds__(kWG) void k_jump_tail(int32_t N, const int32_t *__restrict__ q0,
                                                   const int32_t *__restrict__ t0, int32_t *__restrict__ q1,
                                                   int32_t *__restrict__ t1) {
    const int32_t c = blockIdx.x * kWG + threadIdx.x;
    if (c >= N) return;
    const int64_t row = (int64_t)blockIdx.y * N;
    const int32_t j = q0[row + c];
    q1[row + c] = q0[row + j];
    t1[row + c] = t0[row + c] + t0[row + j];
}

// len holds k_stream_next's 0 / 1
__global__ __launch_bounds__(kWG) void k_jump_final(int32_t N, const int32_t *__restrict__ q,
                                                    const int32_t *__restrict__ t, const int32_t *__restrict__ clen,
                                                    int32_t *__restrict__ len) {
    const int32_t c = blockIdx.x * kWG + threadIdx.x;
    if (c >= N) return;
    const int64_t row = (int64_t)blockIdx.y * N;
    if (len[row + c] == 0) return;
    const int32_t r = clen[row + q[row + c]];
    len[row + c] = t[row + c] + (r != 0 ? r : 1);
}

// Kept lines and their vertices per block of 256 seeds of a field.
__global__ __launch_bounds__(kWG) void k_stream_count(int32_t N, int32_t min_len, const int32_t *__restrict__ len,
                                                      int64_t *__restrict__ bsum) {
    __shared__ int64_t sc[kWG], sv[kWG];
    const int32_t c = blockIdx.x * kWG + threadIdx.x;
    const int32_t L = c < N ? len[(int64_t)blockIdx.y * N + c] : 0;
    const bool keep = L > 0 && L >= min_len;
    sc[threadIdx.x] = keep ? 1 : 0;
    sv[threadIdx.x] = keep ? L : 0;
    __syncthreads();
    for (int d = kWG / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) {
            sc[threadIdx.x] += sc[threadIdx.x + d];
            sv[threadIdx.x] += sv[threadIdx.x + d];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int64_t b = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
        bsum[2 * b] = sc[0];
        bsum[2 * b + 1] = sv[0];
    }
}

// The second walk: boff holds each block's first line and first vertex within
// the pass; a kept seed's line goes to loff[line] (offset + vbase) and its
// vertex ids to lvtx, nlines / nverts entries.
__global__ __launch_bounds__(kWG) void k_stream_emit(int32_t N, int32_t min_len, const int32_t *__restrict__ next,
                                                     const int32_t *__restrict__ len,
                                                     const int64_t *__restrict__ boff, int64_t vbase, int64_t nlines,
                                                     int64_t nverts, int64_t *__restrict__ loff,
                                                     int32_t *__restrict__ lvtx) {
    __shared__ int64_t sc[kWG], sv[kWG];
    const int32_t c = blockIdx.x * kWG + threadIdx.x;
    const int64_t row = (int64_t)blockIdx.y * N;
    const int32_t L = c < N ? len[row + c] : 0;
    const bool keep = L > 0 && L >= min_len;
    sc[threadIdx.x] = keep ? 1 : 0;
    sv[threadIdx.x] = keep ? L : 0;
    __syncthreads();
    for (int d = 1; d < kWG; d <<= 1) {  // inclusive scan
        int64_t ac = 0, av = 0;
        if ((int)threadIdx.x >= d) {
            ac = sc[threadIdx.x - d];
            av = sv[threadIdx.x - d];
        }
        __syncthreads();
        sc[threadIdx.x] += ac;
        sv[threadIdx.x] += av;
        __syncthreads();
    }
    if (!keep) return;
    const int64_t b = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    const int64_t line = boff[2 * b] + sc[threadIdx.x] - 1;
    const int64_t v0 = boff[2 * b + 1] + sv[threadIdx.x] - L;
    if (line >= nlines) return;
    loff[line] = vbase + v0;
    const int32_t *nx = next + row;
    int32_t v = c;
    for (int32_t q = 0; q < L && v >= 0 && v0 + q < nverts; ++q) {
        lvtx[v0 + q] = v;
        v = nx[v];
    }
}

}  // namespace

void stream_destroy(StreamState *st) { delete st; }

// The direction table of the handle (first use), on its own stream.
static StreamState *stream_state(mof_mesh *m) {
    if (!m->sline) m->sline = new StreamState();
    StreamState *S = m->sline;
    if (S->built) return S;
    const int64_t snb = m->pat.sell_nb();
    const size_t N = (size_t)m->N;
    hipStream_t s = m->stream;
    MOF_REQUIRE(m->shared && m->shared->xyz_new.size() >= 3 * N && m->inv.size() >= N &&
                    m->sell_blk.n >= (size_t)snb && m->sell_col.n >= (size_t)snb && m->e.n >= 6 * N &&
                    m->tri.n >= 3 * (size_t)m->M,
                "mesh handle holds no geometry");
    MOF_REQUIRE(snb < ((int64_t)1 << 31), "mesh too large for the streamline tables");
    S->udir.alloc(3 * (size_t)snb);
    S->udir.zero(s);
    S->nbr.alloc((size_t)snb);
    S->btri.alloc((size_t)snb);
    MOF_HIP(hipMemsetAsync(S->nbr.p, 0xFF, S->nbr.bytes(), s));
    MOF_HIP(hipMemsetAsync(S->btri.p, 0xFF, S->btri.bytes(), s));
    S->inv.alloc(N);
    S->inv.upload(m->inv.data(), N, s);
    DevArray<double> xyz;
    xyz.alloc(3 * N);
    xyz.upload(m->shared->xyz_new.data(), 3 * N, s);
    const dim3 grid((unsigned)((m->N + kWG - 1) / kWG));
    if (m->flags & MOF_GEOM_F32_POINTS)
        k_stream_dir<true><<<grid, kWG, 0, s>>>(m->N, m->sell_off.p, m->sell_col.p, m->sell_blk.p, m->cptr.p,
                                                m->clist.p, m->e.p, xyz.p, S->inv.p, S->udir.p, S->nbr.p, S->btri.p);
    else
        k_stream_dir<false><<<grid, kWG, 0, s>>>(m->N, m->sell_off.p, m->sell_col.p, m->sell_blk.p, m->cptr.p,
                                                 m->clist.p, m->e.p, xyz.p, S->inv.p, S->udir.p, S->nbr.p, S->btri.p);
    MOF_HIP(hipGetLastError());
    MOF_HIP(hipStreamSynchronize(s));  // xyz is freed on return
    S->built = true;
    return S;
}

// fields per pass for N vertices: bounds the pass workspace whatever K is
static int32_t stream_pass_fields(int32_t N, int32_t K) {
    int64_t kp = g_stream_pass_fields.load();
    if (kp <= 0) {
        kp = std::max<int64_t>(1, kStreamPassElems / std::max(N, 1));
        if (kp > kStreamF) kp = kp / kStreamF * kStreamF;
    }
    // the kernels' grids: one y index per field (walk) or group of F fields
    return (int32_t)std::min<int64_t>({kp, (int64_t)K, (int64_t)65535});
}

// next (and, with len, the walk lengths) of the Kp fields at V: device pointers
static void stream_pass(mof_mesh *m, StreamState *S, const double *V, int32_t Kp, int32_t *next, int32_t *len,
                        hipStream_t s) {
    constexpr int F = kStreamF;
    NextArgs a;
    a.N = m->N;
    a.K = Kp;
    a.sell_off = m->sell_off.p;
    a.nbr = S->nbr.p;
    a.btri = S->btri.p;
    a.inv = S->inv.p;
    a.tri = m->tri.p;
    a.udir = S->udir.p;
    a.e = m->e.p;
    a.V = V;
    a.next = next;
    a.len = len;
    const unsigned nblk = (unsigned)((m->N + kWG - 1) / kWG);
    k_stream_next<F><<<dim3(nblk, (unsigned)((Kp + F - 1) / F)), kWG, 0, s>>>(a);
    MOF_HIP(hipGetLastError());
    if (!len) return;
    const dim3 grid(nblk, (unsigned)Kp);
    if (!kStreamWalk) {
        k_stream_walk<<<grid, kWG, 0, s>>>(m->N, next, len);
        MOF_HIP(hipGetLastError());
        return;
    }
    const size_t pn = (size_t)Kp * m->N;
    for (auto &w : S->jw)
        if (w.n < pn) w.alloc(pn);
    if (S->clen.n < pn) S->clen.alloc(pn);
    int R = 1;
    while (((int64_t)1 << R) < m->N) ++R;  // 2^R steps pass any tail
    const int32_t *src = next;
    for (int r = 0; r < R; ++r) {
        int32_t *dst = S->jw[r & 1].p;
        k_jump_double<<<grid, kWG, 0, s>>>(m->N, src, dst);
        src = dst;
    }
    MOF_HIP(hipMemsetAsync(S->clen.p, 0, sizeof(int32_t) * pn, s));
    k_jump_mark<<<grid, kWG, 0, s>>>(m->N, src, S->clen.p);
    k_jump_cycle<<<grid, kWG, 0, s>>>(m->N, next, S->clen.p);
    int32_t *q = S->jw[0].p, *t = S->jw[1].p, *q1 = S->jw[2].p, *t1 = S->jw[3].p;
    k_jump_tail_init<<<grid, kWG, 0, s>>>(m->N, next, S->clen.p, q, t);
    for (int r = 0; r < R; ++r) {
        k_jump_tail<<<grid, kWG, 0, s>>>(m->N, q, t, q1, t1);
        std::swap(q, q1);
        std::swap(t, t1);
    }
    k_jump_final<<<grid, kWG, 0, s>>>(m->N, q, t, S->clen.p, len);
    MOF_HIP(hipGetLastError());
}

void stream_map(mof_mesh *m, const double *V, int32_t K, bool dev_io, hipStream_t s, int32_t *next, int32_t *length) {
    StreamState *S = stream_state(m);
    const int64_t N = m->N;
    const int32_t kp = stream_pass_fields(m->N, K);
    const size_t pn = (size_t)kp * N;
    if (!dev_io && S->Vin.n < 3 * pn) S->Vin.alloc(3 * pn);
    if ((!dev_io || !next) && S->nxt.n < pn) S->nxt.alloc(pn);
    if (!dev_io && length && S->len.n < pn) S->len.alloc(pn);
    for (int32_t k0 = 0; k0 < K; k0 += kp) {
        const int32_t k1 = std::min(K, k0 + kp);
        const size_t n = (size_t)(k1 - k0) * N;
        const double *Vd = V + (int64_t)k0 * N * 3;
        if (!dev_io) {
            MOF_HIP(hipMemcpyAsync(S->Vin.p, Vd, sizeof(double) * 3 * n, hipMemcpyHostToDevice, s));
            Vd = S->Vin.p;
        }
        int32_t *nx = dev_io && next ? next + (int64_t)k0 * N : S->nxt.p;
        int32_t *ln = !length ? nullptr : (dev_io ? length + (int64_t)k0 * N : S->len.p);
        stream_pass(m, S, Vd, k1 - k0, nx, ln, s);
        if (!dev_io) {
            if (next) MOF_HIP(hipMemcpyAsync(next + (int64_t)k0 * N, nx, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s));
            if (length)
                MOF_HIP(hipMemcpyAsync(length + (int64_t)k0 * N, ln, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s));
            MOF_HIP(hipStreamSynchronize(s));  // the staging buffers are reused by the next pass
        }
    }
    MOF_HIP(hipStreamSynchronize(s));
}

bool stream_lists(mof_mesh *m, const double *V, int32_t K, int32_t min_len, bool dev_io, hipStream_t s,
                  int64_t cap_lines, int64_t cap_vertices, int64_t *totals, int64_t *n_lines, int64_t *line_off,
                  int32_t *line_vtx) {
    StreamState *S = stream_state(m);
    const int64_t N = m->N;
    const int32_t kp = stream_pass_fields(m->N, K);
    const size_t pn = (size_t)kp * N;
    const int64_t nbx = (N + kWG - 1) / kWG;
    if (!dev_io && S->Vin.n < 3 * pn) S->Vin.alloc(3 * pn);
    if (S->nxt.n < pn) S->nxt.alloc(pn);
    if (S->len.n < pn) S->len.alloc(pn);
    if (S->bsum.n < (size_t)(2 * kp * nbx)) S->bsum.alloc((size_t)(2 * kp * nbx));
    std::vector<int64_t> hb((size_t)(2 * kp * nbx));
    int64_t tl = 0, tv = 0;
    bool over = false;
    for (int32_t k0 = 0; k0 < K; k0 += kp) {
        const int32_t k1 = std::min(K, k0 + kp), Kp = k1 - k0;
        const double *Vd = V + (int64_t)k0 * N * 3;
        if (!dev_io) {
            MOF_HIP(hipMemcpyAsync(S->Vin.p, Vd, sizeof(double) * 3 * (size_t)Kp * N, hipMemcpyHostToDevice, s));
            Vd = S->Vin.p;
        }
        stream_pass(m, S, Vd, Kp, S->nxt.p, S->len.p, s);
        const dim3 grid((unsigned)nbx, (unsigned)Kp);
        k_stream_count<<<grid, kWG, 0, s>>>(m->N, min_len, S->len.p, S->bsum.p);
        MOF_HIP(hipGetLastError());
        const size_t nb = (size_t)(Kp * nbx);
        MOF_HIP(hipMemcpyAsync(hb.data(), S->bsum.p, sizeof(int64_t) * 2 * nb, hipMemcpyDeviceToHost, s));
        MOF_HIP(hipStreamSynchronize(s));
        // block sums -> each block's first line / vertex within the pass
        int64_t pl = 0, pv = 0;
        for (int32_t k = 0; k < Kp; ++k) {
            const int64_t l0 = pl;
            for (int64_t b = (int64_t)k * nbx; b < (int64_t)(k + 1) * nbx; ++b) {
                const int64_t c = hb[2 * b], v = hb[2 * b + 1];
                hb[2 * b] = pl;
                hb[2 * b + 1] = pv;
                pl += c;
                pv += v;
            }
            if (n_lines) n_lines[k0 + k] = pl - l0;
        }
        over = over || tl + pl > cap_lines || tv + pv > cap_vertices;
        if (!over && pl > 0) {
            if (S->loff.n < (size_t)pl) S->loff.alloc((size_t)pl);
            if (S->lvtx.n < (size_t)pv) S->lvtx.alloc((size_t)pv);
            MOF_HIP(hipMemcpyAsync(S->bsum.p, hb.data(), sizeof(int64_t) * 2 * nb, hipMemcpyHostToDevice, s));
            k_stream_emit<<<grid, kWG, 0, s>>>(m->N, min_len, S->nxt.p, S->len.p, S->bsum.p, tv, pl, pv, S->loff.p,
                                               S->lvtx.p);
            MOF_HIP(hipGetLastError());
            MOF_HIP(hipMemcpyAsync(line_off + tl, S->loff.p, sizeof(int64_t) * (size_t)pl, hipMemcpyDeviceToHost, s));
            MOF_HIP(hipMemcpyAsync(line_vtx + tv, S->lvtx.p, sizeof(int32_t) * (size_t)pv, hipMemcpyDeviceToHost, s));
            MOF_HIP(hipStreamSynchronize(s));
        }
        tl += pl;
        tv += pv;
    }
    totals[0] = tl;
    totals[1] = tv;
    if (!over && line_off) line_off[tl] = tv;
    return !over;
}

}  // namespace mof
