// mof_winding.hip -- winding numbers on the mesh (mof_winding_rings,
// mof_winding_levels, mof_winding_map, mof_closest_vertices, include/mof.h):
// the reference's S7_winding_line.py.
//
// The reference, per singular point and level (S7:120-165): the ring of
// vertices at edge distance level + 1 from the nearest vertex c, their
// positions in c's tangent basis, their polar order, and the sum of the
// signed angles between consecutive ring vectors of the field. Everything up
// to the polar order depends on c alone, not on the frame, so it is
//   1. a ring table per distinct centre, built once and shared by all frames:
//      membership by breadth-first search on the host (mof_winding_host.cpp),
//      keys and order on the device (k_wind_sort, one workgroup per ring);
//   2. per (frame, centre) one wave that walks the centre's rings outwards
//      until a check fails (k_wind_levels, wave-uniform exit).
// Level 0 is the Poincare index of the one-ring. At every vertex of every
// field (mof_winding_map) it is a dense pass of the successor map's shape:
// k_wind_map reads each vertex's neighbours in polar order from a per-slot
// table built once per handle (k_wind_rank), as k_stream_dir builds u_j.
//
// Both kernels take the ring's angles from the same device functions
// (wind_unit, wind_angle) and add them in ring order, one after the other,
// starting from 0: wn0[k, c] of the map equals wn[., 0] of the levels bit for
// bit, and nothing depends on the handle's internal vertex order (the table
// and the rings hold the caller's ids, ties go to the smaller of them).
//
// Compiled without fp contraction: every product and sum rounds as numpy's.
#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>

#include "mof_internal.h"

int mof_io_guard(const std::function<void()> &f);  // mof_abi.cpp: status + mof_last_error

namespace mof {

#ifndef MOF_WIND_F
#define MOF_WIND_F 4
#endif
constexpr int kWindF = MOF_WIND_F;  // fields per thread of k_wind_map: one read of a row's table serves F fields
// auto fields per pass of the map: at most this many (field, vertex) pairs --
// 48 MiB of staged V and 18 MiB of staged results whatever K is
constexpr int64_t kWindPassElems = (int64_t)2 << 20;
constexpr int kSortLds = 2048;  // ring vertices k_wind_sort ranks out of LDS; larger rings out of global memory
std::atomic<int> g_wind_pass_fields{0};  // tests only (mof_test_winding_pass): fields per pass, 0 = auto
static double g_wind_ms[3] = {0.0, 0.0, 0.0};  // mof_winding_timing: host search, sort, evaluation of the last call

struct WindState {
    DevArray<double> xyz;    // [N][3] positions, internal order
    DevArray<int32_t> inv;   // [N] internal vertex -> caller's id
    DevArray<int32_t> pnbr;  // [sell_nb] slot r + 1 of a row: its neighbour of polar rank r, caller's id; else -1
    bool geom = false, ranked = false;
    // the ring table of the last call
    DevArray<int32_t> t_cen;   // [C] centres, internal ids
    DevArray<int64_t> t_off;   // [C][L + 1]
    DevArray<int32_t> t_in;    // ring members, internal ids, search order
    DevArray<int32_t> t_cid;   // the same in the caller's ids
    DevArray<double> t_key;    // their polar keys
    DevArray<int32_t> t_ring;  // the sorted rings, caller's ids
    // staging
    DevArray<double> Vin, wn;
    DevArray<int8_t> idx, typ;
    DevArray<int32_t> qf, qr, cnt, cv;
    DevArray<double> pts;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    ~WindState() {
        for (auto e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

namespace {

struct Basis {
    double e1[3], e2[3], n[3], nn, e11, e22;
};

__device__ __forceinline__ double dot3(const double *a, const double *b) {
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

__device__ __forceinline__ Basis wind_basis(const double *__restrict__ e6) {
    Basis B;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        B.e1[d] = e6[d];
        B.e2[d] = e6[3 + d];
    }
    B.n[0] = B.e1[1] * B.e2[2] - B.e1[2] * B.e2[1];
    B.n[1] = B.e1[2] * B.e2[0] - B.e1[0] * B.e2[2];
    B.n[2] = B.e1[0] * B.e2[1] - B.e1[1] * B.e2[0];
    B.nn = dot3(B.n, B.n);
    B.e11 = dot3(B.e1, B.e1);
    B.e22 = dot3(B.e2, B.e2);
    return B;
}

// position_diff_on_basis_with_origin (S7:36-45) and the polar key
template <bool F32P>
__device__ __forceinline__ double wind_key(const Basis &B, const double *__restrict__ pc,
                                           const double *__restrict__ pj) {
    double w[3], p[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) w[d] = F32P ? (double)((float)pj[d] - (float)pc[d]) : pj[d] - pc[d];
    const double wn = dot3(w, B.n);
#pragma unroll
    for (int d = 0; d < 3; ++d) p[d] = w[d] - wn * B.n[d] / B.nn;
    return atan2(dot3(p, B.e2), dot3(p, B.e1));
}

__device__ __forceinline__ bool key_less(double ka, int32_t ia, double kb, int32_t ib) {
    return ka < kb || (ka == kb && ia < ib);
}

// project_vector_to_plane, express_vector_on_basis and the normalisation of
// angle_between_vectors (S7:26-33, 48-57, 63-64)
__device__ __forceinline__ void wind_unit(const Basis &B, const double *__restrict__ V, double &ux, double &uy) {
    const double v[3] = {V[0], V[1], V[2]};
    const double vn = dot3(v, B.n);
    double vt[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) vt[d] = v[d] - vn * B.n[d] / B.nn;
    const double a = dot3(vt, B.e1) / B.e11, b = dot3(vt, B.e2) / B.e22;
    const double r = sqrt(a * a + b * b);
    ux = a / r;
    uy = b / r;
}

// angle_between_vectors (S7:65-74) of two unit vectors
__device__ __forceinline__ double wind_angle(double ux, double uy, double vx, double vy) {
    double d = ux * vx + uy * vy;
    if (d > 1)
        d = 1;
    else if (d < -1)
        d = -1;
    const double ang = acos(d);
    return (ux * vy - uy * vx < 0) ? -ang : ang;
}

constexpr double kTwoPi = 6.283185307179586;  // 2 * np.pi

__device__ __forceinline__ int wind_type0(double wn) {  // S7:150-158
    if (-1.01 <= wn && wn <= -0.99) return -1;
    if (0.99 <= wn && wn <= 1.01) return 1;
    return 0;
}

__device__ __forceinline__ bool wind_check(double wn, int flag) {  // check_property (S7:104-118)
    if (flag == 1) return wn >= 0.999 && wn <= 1.001;
    if (flag == -1) return wn >= -1.001 && wn <= -0.999;
    return false;
}

// One thread per vertex row: the polar keys of its neighbours into key (per
// SELL slot), then each neighbour to the slot of its rank.
template <bool F32P>
__global__ __launch_bounds__(kWG) void k_wind_rank(int32_t N, const int32_t *__restrict__ sell_off,
                                                   const int32_t *__restrict__ sell_col,
                                                   const int32_t *__restrict__ sell_blk, const double *__restrict__ e,
                                                   const double *__restrict__ xyz, const int32_t *__restrict__ inv,
                                                   double *__restrict__ key, int32_t *__restrict__ pnbr) {
    const int32_t i = blockIdx.x * kWG + threadIdx.x;
    if (i >= N) return;
    const int32_t s = i >> 6, l = i & 63;
    const int32_t o = sell_off[s];
    const int32_t w = (sell_off[s + 1] - o) >> 6;
    const Basis B = wind_basis(e + 6 * (int64_t)i);
    const double *pc = xyz + 3 * (int64_t)i;
    for (int32_t t = 1; t < w; ++t) {  // slot 0 is the row itself
        const int64_t pos = (int64_t)o + t * kSlice + l;
        if (sell_blk[pos] < 0) continue;
        key[pos] = wind_key<F32P>(B, pc, xyz + 3 * (int64_t)sell_col[pos]);
    }
    for (int32_t t = 1; t < w; ++t) {
        const int64_t pos = (int64_t)o + t * kSlice + l;
        if (sell_blk[pos] < 0) continue;
        const double kt = key[pos];
        const int32_t it = inv[sell_col[pos]];
        int32_t rank = 0;
        for (int32_t u = 1; u < w; ++u) {
            const int64_t pu = (int64_t)o + u * kSlice + l;
            if (u == t || sell_blk[pu] < 0) continue;
            rank += key_less(key[pu], inv[sell_col[pu]], kt, it) ? 1 : 0;
        }
        pnbr[(int64_t)o + (rank + 1) * kSlice + l] = it;  // rank < the row's neighbours <= w - 1
    }
}

struct MapArgs {
    int32_t N, K;  // vertices, fields of the pass
    const int32_t *sell_off, *pnbr, *inv;
    const double *e;
    const double *V;  // [K][N][3] caller's order
    double *wn0;      // [K][N] caller's order, or null
    int8_t *index;    // [K][N] or null
};

// One wave per SELL slice, one thread per (vertex row, group of F fields).
template <int F>
__global__ __launch_bounds__(kWG) void k_wind_map(const MapArgs a) {
    const int32_t i = blockIdx.x * kWG + (int32_t)threadIdx.x;
    if (i >= a.N) return;
    const int32_t k0 = (int32_t)blockIdx.y * F;
    const int64_t N = a.N;
    const int32_t s = i >> 6, l = i & 63;
    const int32_t o = a.sell_off[s];
    const int32_t w = (a.sell_off[s + 1] - o) >> 6;
    const Basis B = wind_basis(a.e + 6 * (int64_t)i);
    double fx[F], fy[F], px[F], py[F], acc[F];
    int32_t n = 0;
    for (int32_t t = 1; t < w; ++t) {
        const int32_t id = a.pnbr[o + t * kSlice + l];
        if (id < 0) break;  // the ranks fill the slots from 1 without gaps
#pragma unroll
        for (int f = 0; f < F; ++f) {
            const int32_t k = k0 + f < a.K ? k0 + f : k0;
            double ux, uy;
            wind_unit(B, a.V + ((int64_t)k * N + id) * 3, ux, uy);
            if (n == 0) {
                fx[f] = ux;
                fy[f] = uy;
                acc[f] = 0.0;
            } else {
                acc[f] += wind_angle(px[f], py[f], ux, uy);
            }
            px[f] = ux;
            py[f] = uy;
        }
        ++n;
    }
    const int32_t ci = a.inv[i];
#pragma unroll
    for (int f = 0; f < F; ++f) {
        if (k0 + f >= a.K) break;
        double wn = NAN;  // no neighbour: an empty ring
        if (n > 0) {
            acc[f] += wind_angle(px[f], py[f], fx[f], fy[f]);
            wn = acc[f] / kTwoPi;
        }
        const int64_t q = (int64_t)(k0 + f) * N + ci;
        if (a.wn0) a.wn0[q] = wn;
        if (a.index) a.index[q] = (int8_t)wind_type0(wn);
    }
}

// One workgroup per (centre, ring): the keys, then every member to the place
// of its rank among (key, caller's id). Rings up to kSortLds vertices are
// ranked out of LDS, larger ones out of the key array in global memory.
template <bool F32P>
__global__ __launch_bounds__(kWG) void k_wind_sort(int32_t L, const int32_t *__restrict__ cen,
                                                   const int64_t *__restrict__ off, const int32_t *__restrict__ rin,
                                                   const double *__restrict__ e, const double *__restrict__ xyz,
                                                   const int32_t *__restrict__ inv, double *__restrict__ key,
                                                   int32_t *__restrict__ cid, int32_t *__restrict__ ring) {
    __shared__ double skey[kSortLds];
    __shared__ int32_t scid[kSortLds];
    const int64_t r = blockIdx.x;
    const int64_t c = r / L, l = r % L;
    const int64_t o0 = off[c * (L + 1) + l];
    const int64_t n = off[c * (L + 1) + l + 1] - o0;
    if (n <= 0) return;  // the whole workgroup
    const int32_t ci = cen[c];
    const Basis B = wind_basis(e + 6 * (int64_t)ci);
    const double *pc = xyz + 3 * (int64_t)ci;
    const bool lds = n <= kSortLds;
    for (int64_t p = threadIdx.x; p < n; p += kWG) {
        const int32_t j = rin[o0 + p];
        const double k = wind_key<F32P>(B, pc, xyz + 3 * (int64_t)j);
        const int32_t id = inv[j];
        key[o0 + p] = k;
        cid[o0 + p] = id;
        if (lds) {
            skey[p] = k;
            scid[p] = id;
        }
    }
    __syncthreads();  // the keys, in LDS and (workgroup scope) in global memory
    for (int64_t p = threadIdx.x; p < n; p += kWG) {
        int64_t rank = 0;
        if (lds) {
            const double kp = skey[p];
            const int32_t ip = scid[p];
            for (int32_t u = 0; u < (int32_t)n; ++u) rank += key_less(skey[u], scid[u], kp, ip) ? 1 : 0;
            ring[o0 + rank] = ip;
        } else {
            const double kp = key[o0 + p];
            const int32_t ip = cid[o0 + p];
            for (int64_t u = 0; u < n; ++u) rank += key_less(key[o0 + u], cid[o0 + u], kp, ip) ? 1 : 0;
            ring[o0 + rank] = ip;
        }
    }
}

struct LevelArgs {
    int32_t Q, L, N, all;
    const int32_t *qframe, *qrow;  // [Q] field of V and row of the ring table
    const int32_t *cen;            // [C] centres, internal ids
    const int64_t *off;            // [C][L + 1]
    const int32_t *ring;           // sorted rings, caller's ids
    const double *e, *V;
    double *wn;      // [Q][L] or null
    int32_t *count;  // [Q] or null
    int8_t *type;    // [Q] or null
};

// One wave per query. Per ring, 64 angles at a time: each lane forms the angle
// from its ring vertex to the next, then every lane adds the 64 in ring order
// (the same additions in the same order as k_wind_map's thread).
__global__ __launch_bounds__(kWG) void k_wind_levels(const LevelArgs a) {
    const int32_t lane = threadIdx.x & 63;
    const int32_t q = blockIdx.x * (kWG / 64) + ((int32_t)threadIdx.x >> 6);
    if (q >= a.Q) return;  // the whole wave
    const int32_t L = a.L;
    const int64_t row = a.qrow[q];
    const Basis B = wind_basis(a.e + 6 * (int64_t)a.cen[row]);
    const double *V = a.V + (int64_t)a.qframe[q] * a.N * 3;
    const int64_t *off = a.off + row * (L + 1);
    int32_t count = 0, flag = 0, l = 0;
    bool live = true;
    for (; l < L; ++l) {
        const int64_t o0 = off[l], n = off[l + 1] - o0;
        if (n == 0) break;  // the mesh is exhausted: as a failed check
        if (!live && !a.all) break;
        double acc = 0.0;
        for (int64_t base = 0; base < n; base += 64) {
            const int64_t p = base + lane;
            double ang = 0.0;
            if (p < n) {
                const int32_t j0 = a.ring[o0 + p], j1 = a.ring[o0 + (p + 1 == n ? 0 : p + 1)];
                double ux, uy, vx, vy;
                wind_unit(B, V + 3 * (int64_t)j0, ux, uy);
                wind_unit(B, V + 3 * (int64_t)j1, vx, vy);
                ang = wind_angle(ux, uy, vx, vy);
            }
            const int32_t m = (int32_t)(n - base < 64 ? n - base : 64);
            for (int32_t t = 0; t < m; ++t) acc += __shfl(ang, t);
        }
        const double wn = acc / kTwoPi;
        if (a.wn && lane == 0) a.wn[(int64_t)q * L + l] = wn;
        if (!live) continue;
        if (l == 0) {
            flag = wind_type0(wn);
            count = flag ? 1 : 0;  // and on to level 1 whatever the flag (S7:150-158 has no break)
        } else if (wind_check(wn, flag)) {
            ++count;
        } else {
            live = false;
        }
    }
    if (a.wn)
        for (int32_t r = l + lane; r < L; r += 64) a.wn[(int64_t)q * L + r] = NAN;
    if (lane == 0) {
        if (a.count) a.count[q] = count;
        if (a.type) a.type[q] = (int8_t)flag;
    }
}

// One workgroup per query point: the nearest vertex, the lowest caller's id
// among equally near ones.
__global__ __launch_bounds__(kWG) void k_wind_closest(int32_t N, const double *__restrict__ xyz,
                                                      const int32_t *__restrict__ inv,
                                                      const double *__restrict__ pts, int32_t *__restrict__ out) {
    __shared__ double sd[kWG];
    __shared__ int32_t si[kWG];
    const double *x = pts + 3 * (int64_t)blockIdx.x;
    const double x0 = x[0], x1 = x[1], x2 = x[2];
    double bd = INFINITY;
    int32_t bi = INT_MAX;
    for (int32_t i = threadIdx.x; i < N; i += kWG) {
        const double *p = xyz + 3 * (int64_t)i;
        const double d0 = p[0] - x0, d1 = p[1] - x1, d2 = p[2] - x2;
        const double d = (d0 * d0 + d1 * d1) + d2 * d2;
        const int32_t id = inv[i];
        if (d < bd || (d == bd && id < bi)) {
            bd = d;
            bi = id;
        }
    }
    sd[threadIdx.x] = bd;
    si[threadIdx.x] = bi;
    __syncthreads();
    for (int s = kWG / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const double d = sd[threadIdx.x + s];
            const int32_t id = si[threadIdx.x + s];
            if (d < sd[threadIdx.x] || (d == sd[threadIdx.x] && id < si[threadIdx.x])) {
                sd[threadIdx.x] = d;
                si[threadIdx.x] = id;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = si[0] == INT_MAX ? -1 : si[0];  // -1: every distance is NaN
}

struct DeviceGuard {
    int prev = 0;
    explicit DeviceGuard(int d) {
        (void)hipGetDevice(&prev);
        MOF_HIP(hipSetDevice(d));
    }
    ~DeviceGuard() { (void)hipSetDevice(prev); }
};

template <typename T>
void grow(DevArray<T> &a, size_t n) {
    if (a.n < n) a.alloc(n);
}

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

void wind_destroy(WindState *st) { delete st; }

// The handle's positions and id map on the device (first use).
static WindState *wind_state(mof_mesh *m, hipStream_t s) {
    if (!m->wind) m->wind = new WindState();
    WindState *S = m->wind;
    if (S->geom) return S;
    const size_t N = (size_t)m->N;
    MOF_REQUIRE(m->shared && m->shared->xyz_new.size() >= 3 * N && m->inv.size() >= N && m->perm.size() >= N &&
                    m->e.n >= 6 * N,
                "mesh handle holds no geometry");
    S->xyz.alloc(3 * N);
    S->xyz.upload(m->shared->xyz_new.data(), 3 * N, s);
    S->inv.alloc(N);
    S->inv.upload(m->inv.data(), N, s);
    for (auto &e : S->ev) MOF_HIP(hipEventCreate(&e));
    MOF_HIP(hipStreamSynchronize(s));
    S->geom = true;
    return S;
}

// The polar-ordered neighbour table of the handle (first mof_winding_map).
static void wind_rank(mof_mesh *m, WindState *S, hipStream_t s) {
    if (S->ranked) return;
    const int64_t snb = m->pat.sell_nb();
    MOF_REQUIRE(m->sell_blk.n >= (size_t)snb && m->sell_col.n >= (size_t)snb, "mesh handle holds no geometry");
    MOF_REQUIRE(snb < ((int64_t)1 << 31), "mesh too large for the winding table");
    S->pnbr.alloc((size_t)snb);
    MOF_HIP(hipMemsetAsync(S->pnbr.p, 0xFF, S->pnbr.bytes(), s));
    DevArray<double> key;
    key.alloc((size_t)snb);
    const dim3 grid((unsigned)((m->N + kWG - 1) / kWG));
    if (m->flags & MOF_GEOM_F32_POINTS)
        k_wind_rank<true><<<grid, kWG, 0, s>>>(m->N, m->sell_off.p, m->sell_col.p, m->sell_blk.p, m->e.p, S->xyz.p,
                                               S->inv.p, key.p, S->pnbr.p);
    else
        k_wind_rank<false><<<grid, kWG, 0, s>>>(m->N, m->sell_off.p, m->sell_col.p, m->sell_blk.p, m->e.p, S->xyz.p,
                                                S->inv.p, key.p, S->pnbr.p);
    MOF_HIP(hipGetLastError());
    MOF_HIP(hipStreamSynchronize(s));  // key is freed on return
    S->ranked = true;
}

static int32_t wind_pass_fields(int32_t N, int32_t K) {
    int64_t kp = g_wind_pass_fields.load();
    if (kp <= 0) {
        kp = std::max<int64_t>(1, kWindPassElems / std::max(N, 1));
        if (kp > kWindF) kp = kp / kWindF * kWindF;
    }
    return (int32_t)std::min<int64_t>({kp, (int64_t)K, (int64_t)65535 * kWindF});
}

static void wind_map(mof_mesh *m, const double *V, int32_t K, bool dev_io, hipStream_t s, double *wn0, int8_t *index) {
    WindState *S = wind_state(m, s);
    wind_rank(m, S, s);
    const int64_t N = m->N;
    const int32_t kp = wind_pass_fields(m->N, K);
    const size_t pn = (size_t)kp * N;
    if (!dev_io) {
        grow(S->Vin, 3 * pn);
        if (wn0) grow(S->wn, pn);
        if (index) grow(S->idx, pn);
    }
    for (int32_t k0 = 0; k0 < K; k0 += kp) {
        const int32_t k1 = std::min(K, k0 + kp), Kp = k1 - k0;
        const size_t n = (size_t)Kp * N;
        const double *Vd = V + (int64_t)k0 * N * 3;
        if (!dev_io) {
            MOF_HIP(hipMemcpyAsync(S->Vin.p, Vd, sizeof(double) * 3 * n, hipMemcpyHostToDevice, s));
            Vd = S->Vin.p;
        }
        MapArgs a;
        a.N = m->N;
        a.K = Kp;
        a.sell_off = m->sell_off.p;
        a.pnbr = S->pnbr.p;
        a.inv = S->inv.p;
        a.e = m->e.p;
        a.V = Vd;
        a.wn0 = !wn0 ? nullptr : (dev_io ? wn0 + (int64_t)k0 * N : S->wn.p);
        a.index = !index ? nullptr : (dev_io ? index + (int64_t)k0 * N : S->idx.p);
        const dim3 grid((unsigned)((m->N + kWG - 1) / kWG), (unsigned)((Kp + kWindF - 1) / kWindF));
        k_wind_map<kWindF><<<grid, kWG, 0, s>>>(a);
        MOF_HIP(hipGetLastError());
        if (!dev_io) {
            if (wn0) MOF_HIP(hipMemcpyAsync(wn0 + (int64_t)k0 * N, a.wn0, sizeof(double) * n, hipMemcpyDeviceToHost, s));
            if (index) MOF_HIP(hipMemcpyAsync(index + (int64_t)k0 * N, a.index, n, hipMemcpyDeviceToHost, s));
            MOF_HIP(hipStreamSynchronize(s));  // the staging buffers are reused by the next pass
        }
    }
    MOF_HIP(hipStreamSynchronize(s));
}

// The sorted ring table of C centres (host, caller's ids) into S->t_*; the
// host copy of its offsets in off. Returns the entries.
static int64_t wind_table(mof_mesh *m, WindState *S, const int32_t *centres, int32_t C, int32_t L, hipStream_t s,
                          std::vector<int64_t> &off) {
    std::vector<int32_t> cen((size_t)C), members;
    for (int32_t q = 0; q < C; ++q) {
        MOF_REQUIRE(centres[q] >= 0 && centres[q] < m->N, "centre " + std::to_string(centres[q]) + " is no vertex");
        cen[q] = m->perm[centres[q]];
    }
    auto t0 = std::chrono::steady_clock::now();
    wind_bfs(m->pat, cen.data(), C, L, off, members);
    g_wind_ms[0] = ms_since(t0);
    const int64_t total = (int64_t)members.size();
    const int64_t nrings = (int64_t)C * L;
    MOF_REQUIRE(nrings < ((int64_t)1 << 31), "centres x max_level exceeds 2^31 rings");
    grow(S->t_cen, (size_t)C);
    grow(S->t_off, off.size());
    grow(S->t_in, (size_t)total);
    grow(S->t_cid, (size_t)total);
    grow(S->t_key, (size_t)total);
    grow(S->t_ring, (size_t)total);
    S->t_cen.upload(cen.data(), (size_t)C, s);
    S->t_off.upload(off.data(), off.size(), s);
    if (total) S->t_in.upload(members.data(), (size_t)total, s);
    S->t_ring.zero(s);  // NaN keys (a NaN position or basis) share ranks: the places they skip stay vertex 0
    MOF_HIP(hipEventRecord(S->ev[0], s));
    if (total) {
        if (m->flags & MOF_GEOM_F32_POINTS)
            k_wind_sort<true><<<(unsigned)nrings, kWG, 0, s>>>(L, S->t_cen.p, S->t_off.p, S->t_in.p, m->e.p, S->xyz.p,
                                                               S->inv.p, S->t_key.p, S->t_cid.p, S->t_ring.p);
        else
            k_wind_sort<false><<<(unsigned)nrings, kWG, 0, s>>>(L, S->t_cen.p, S->t_off.p, S->t_in.p, m->e.p, S->xyz.p,
                                                                S->inv.p, S->t_key.p, S->t_cid.p, S->t_ring.p);
        MOF_HIP(hipGetLastError());
    }
    MOF_HIP(hipEventRecord(S->ev[1], s));
    MOF_HIP(hipStreamSynchronize(s));  // cen, off and members leave scope
    float ms = 0.f;
    MOF_HIP(hipEventElapsedTime(&ms, S->ev[0], S->ev[1]));
    g_wind_ms[1] = ms;
    g_wind_ms[2] = 0.0;
    return total;
}

static void wind_levels(mof_mesh *m, const double *V, int32_t K, const int32_t *frame, const int32_t *centre, int32_t Q,
                        int32_t L, bool all, bool dev_io, hipStream_t s, double *wn, int32_t *count, int8_t *type) {
    WindState *S = wind_state(m, s);
    const int64_t N = m->N;
    std::vector<int32_t> hf((size_t)Q), hc((size_t)Q);
    if (dev_io) {
        MOF_HIP(hipMemcpyAsync(hf.data(), frame, sizeof(int32_t) * Q, hipMemcpyDeviceToHost, s));
        MOF_HIP(hipMemcpyAsync(hc.data(), centre, sizeof(int32_t) * Q, hipMemcpyDeviceToHost, s));
        MOF_HIP(hipStreamSynchronize(s));
    } else {
        std::copy(frame, frame + Q, hf.begin());
        std::copy(centre, centre + Q, hc.begin());
    }
    for (int32_t q = 0; q < Q; ++q)
        MOF_REQUIRE(hf[q] >= 0 && hf[q] < K, "frame " + std::to_string(hf[q]) + " outside the K fields");
    // the distinct centres, ascending, and each query's row among them
    std::vector<int32_t> uc(hc);
    std::sort(uc.begin(), uc.end());
    uc.erase(std::unique(uc.begin(), uc.end()), uc.end());
    std::vector<int64_t> off;
    wind_table(m, S, uc.data(), (int32_t)uc.size(), L, s, off);
    std::vector<int32_t> qrow((size_t)Q);
    for (int32_t q = 0; q < Q; ++q) qrow[q] = (int32_t)(std::lower_bound(uc.begin(), uc.end(), hc[q]) - uc.begin());
    // host pointers: only the fields the queries name are staged
    const double *Vd = V;
    if (!dev_io) {
        std::vector<int32_t> uf(hf);
        std::sort(uf.begin(), uf.end());
        uf.erase(std::unique(uf.begin(), uf.end()), uf.end());
        grow(S->Vin, 3 * uf.size() * (size_t)N);
        for (size_t u = 0; u < uf.size(); ++u)
            MOF_HIP(hipMemcpyAsync(S->Vin.p + 3 * u * (size_t)N, V + 3 * (int64_t)uf[u] * N, sizeof(double) * 3 * N,
                                   hipMemcpyHostToDevice, s));
        for (int32_t q = 0; q < Q; ++q) hf[q] = (int32_t)(std::lower_bound(uf.begin(), uf.end(), hf[q]) - uf.begin());
        Vd = S->Vin.p;
        if (wn) grow(S->wn, (size_t)Q * L);
        if (count) grow(S->cnt, (size_t)Q);
        if (type) grow(S->typ, (size_t)Q);
    }
    grow(S->qf, (size_t)Q);
    grow(S->qr, (size_t)Q);
    S->qf.upload(hf.data(), (size_t)Q, s);
    S->qr.upload(qrow.data(), (size_t)Q, s);
    LevelArgs a;
    a.Q = Q;
    a.L = L;
    a.N = m->N;
    a.all = all ? 1 : 0;
    a.qframe = S->qf.p;
    a.qrow = S->qr.p;
    a.cen = S->t_cen.p;
    a.off = S->t_off.p;
    a.ring = S->t_ring.p;
    a.e = m->e.p;
    a.V = Vd;
    a.wn = !wn ? nullptr : (dev_io ? wn : S->wn.p);
    a.count = !count ? nullptr : (dev_io ? count : S->cnt.p);
    a.type = !type ? nullptr : (dev_io ? type : S->typ.p);
    MOF_HIP(hipEventRecord(S->ev[2], s));
    k_wind_levels<<<(unsigned)((Q + kWG / 64 - 1) / (kWG / 64)), kWG, 0, s>>>(a);
    MOF_HIP(hipGetLastError());
    MOF_HIP(hipEventRecord(S->ev[3], s));
    if (!dev_io) {
        if (wn) MOF_HIP(hipMemcpyAsync(wn, a.wn, sizeof(double) * (size_t)Q * L, hipMemcpyDeviceToHost, s));
        if (count) MOF_HIP(hipMemcpyAsync(count, a.count, sizeof(int32_t) * (size_t)Q, hipMemcpyDeviceToHost, s));
        if (type) MOF_HIP(hipMemcpyAsync(type, a.type, (size_t)Q, hipMemcpyDeviceToHost, s));
    }
    MOF_HIP(hipStreamSynchronize(s));  // hf and qrow leave scope
    float ms = 0.f;
    MOF_HIP(hipEventElapsedTime(&ms, S->ev[2], S->ev[3]));
    g_wind_ms[2] = ms;
}

static void wind_closest(mof_mesh *m, const double *points, int32_t Q, bool dev_io, hipStream_t s, int32_t *vertex) {
    WindState *S = wind_state(m, s);
    const double *pd = points;
    int32_t *vd = vertex;
    if (!dev_io) {
        grow(S->pts, 3 * (size_t)Q);
        grow(S->cv, (size_t)Q);
        S->pts.upload(points, 3 * (size_t)Q, s);
        pd = S->pts.p;
        vd = S->cv.p;
    }
    k_wind_closest<<<(unsigned)Q, kWG, 0, s>>>(m->N, S->xyz.p, S->inv.p, pd, vd);
    MOF_HIP(hipGetLastError());
    if (!dev_io) MOF_HIP(hipMemcpyAsync(vertex, vd, sizeof(int32_t) * (size_t)Q, hipMemcpyDeviceToHost, s));
    MOF_HIP(hipStreamSynchronize(s));
}

}  // namespace mof

using mof::DeviceGuard;

extern "C" {

int mof_winding_rings(mof_mesh *m, const int32_t *centres, int32_t C, int32_t max_level, int64_t cap, int64_t *total,
                      int64_t *level_off, int32_t *ring_vtx) {
    return mof_io_guard([&] {
        MOF_REQUIRE(m, "mesh is NULL");
        MOF_REQUIRE(centres && total, "centres or total is NULL");
        MOF_REQUIRE(C >= 1 && max_level >= 1, "C < 1 centres or max_level < 1");
        MOF_REQUIRE(cap >= 0 && (cap == 0 || (level_off && ring_vtx)), "NULL table with a capacity");
        mof::mesh_join_prep(m);
        DeviceGuard dg(m->device);
        hipStream_t s = m->stream;
        mof::WindState *S = mof::wind_state(m, s);
        std::vector<int64_t> off;
        *total = mof::wind_table(m, S, centres, C, max_level, s, off);
        MOF_REQUIRE(*total <= cap && level_off && ring_vtx,
                    "ring table exceeds cap: " + std::to_string(*total) + " entries (total)");
        std::copy(off.begin(), off.end(), level_off);
        if (*total) {
            MOF_HIP(hipMemcpyAsync(ring_vtx, S->t_ring.p, sizeof(int32_t) * (size_t)*total, hipMemcpyDeviceToHost, s));
            MOF_HIP(hipStreamSynchronize(s));
        }
    });
}

int mof_winding_levels(mof_mesh *m, const double *V_coord, int32_t K, const int32_t *frame, const int32_t *centre,
                       int32_t Q, int32_t max_level, uint32_t flags, void *stream, double *wn, int32_t *count,
                       int8_t *type) {
    return mof_io_guard([&] {
        MOF_REQUIRE(m, "mesh is NULL");
        MOF_REQUIRE(V_coord && frame && centre, "V_coord, frame or centre is NULL");
        MOF_REQUIRE(K >= 1 && Q >= 1 && max_level >= 1, "K < 1 fields, Q < 1 queries or max_level < 1");
        MOF_REQUIRE(wn || count || type, "every output is NULL");
        mof::mesh_join_prep(m);
        DeviceGuard dg(m->device);
        hipStream_t s = stream ? (hipStream_t)stream : m->stream;
        mof::wind_levels(m, V_coord, K, frame, centre, Q, max_level, (flags & MOF_WIND_ALL_LEVELS) != 0,
                         (flags & MOF_IO_DEVICE) != 0, s, wn, count, type);
    });
}

int mof_winding_map(mof_mesh *m, const double *V_coord, int32_t K, uint32_t flags, void *stream, double *wn0,
                    int8_t *index) {
    return mof_io_guard([&] {
        MOF_REQUIRE(m, "mesh is NULL");
        MOF_REQUIRE(V_coord, "V_coord is NULL");
        MOF_REQUIRE(K >= 1, "K < 1 fields");
        MOF_REQUIRE(wn0 || index, "every output is NULL");
        mof::mesh_join_prep(m);
        DeviceGuard dg(m->device);
        hipStream_t s = stream ? (hipStream_t)stream : m->stream;
        mof::wind_map(m, V_coord, K, (flags & MOF_IO_DEVICE) != 0, s, wn0, index);
    });
}

int mof_test_winding_pass(int32_t fields) {
    mof::g_wind_pass_fields.store(fields > 0 ? fields : 0);
    return MOF_OK;
}

int mof_winding_timing(double *ms) {
    return mof_io_guard([&] {
        MOF_REQUIRE(ms, "ms is NULL");
        for (int i = 0; i < 3; ++i) ms[i] = mof::g_wind_ms[i];
    });
}

int mof_closest_vertices(mof_mesh *m, const double *points, int32_t Q, uint32_t flags, void *stream, int32_t *vertex) {
    return mof_io_guard([&] {
        MOF_REQUIRE(m, "mesh is NULL");
        MOF_REQUIRE(points && vertex, "points or vertex is NULL");
        MOF_REQUIRE(Q >= 1, "Q < 1 points");
        mof::mesh_join_prep(m);
        DeviceGuard dg(m->device);
        hipStream_t s = stream ? (hipStream_t)stream : m->stream;
        mof::wind_closest(m, points, Q, (flags & MOF_IO_DEVICE) != 0, s, vertex);
    });
}

}  // extern "C"
