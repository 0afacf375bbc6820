// mof_rbf.hip -- potentials on the mesh from the electrodes (mof_rbf_eval,
// include/mof.h): the device half of the reference's S2_interpolate.py and
// S2_interpolate_phases.py.
//
// The scripts build scipy.interpolate.Rbf(x, y, z, d) per frame with all
// defaults (multiquadric, euclidean, smooth 0) and evaluate it at the surface's
// vertices. The E x E matrix does not depend on the frame, so the weights of
// all frames are one host solve (mofhip/interp.py: numpy; the library links no
// LAPACK) and the evaluation is the (T x E) (E x N) product
//   out[t][i] = sum_e W[t][e] phi(i, e),
//   r = sqrt((dx dx + dy dy) + dz dz), q = (1 / epsilon) r, phi = sqrt(q q + 1)
// -- scipy's cdist and _h_multiquadric statement by statement in fp64 without
// contraction (this file is built with -ffp-contract=off; sqrt is correctly
// rounded), so phi is scipy's bit for bit.
//
// k_rbf_eval, on v_mfma_f64_16x16x4_f64: frames on the rows of the D tile,
// vertices on its columns, electrodes on K, four per product. A wave owns NT
// tiles of 16 consecutive vertices and keeps their phi in registers in the B
// operand's layout -- lane l holds phi(vertex l & 15, electrode 4 c + (l >> 4))
// for every K-chunk c: NT * KC = 64 values, KC = 16, 32 or 64 chunks for E up
// to 64, 128 or 256 -- generated once and used for every frame tile the
// workgroup walks. phi never reaches memory. The A operand, W[frame l & 15]
// [electrode 4 c + (l >> 4)], is read from a zero-padded copy of the pass's
// weights in operand order (k_rbf_pack: [frame tile][chunk][lane], so a wave's
// load is 512 contiguous bytes), a few hundred KB that the caches serve, one
// group of 8 or 16 chunks ahead of the products. A padding column multiplies the phi of
// electrode 0, a padding vertex reads vertex N - 1: 0 * finite, nothing out of
// bounds, and rows >= the pass's frames and columns >= N are not stored. The
// result map col = l & 15, row = (l >> 4) + 4 reg makes each store of a wave
// 128 contiguous bytes along a row of out, NT of them side by side.
//
// One entry of out is one chain of products over the chunks c = 0, 1, ... in
// ascending order in one accumulator: no atomics, no partial sums through
// memory, and no dependence on the tile row a frame lands in -- so none on the
// pass size, nor on how the frame tiles are spread over the grid.
#include <algorithm>
#include <cmath>

#include "mof_internal.h"

int mof_io_guard(const std::function<void()> &f);  // mof_abi.cpp: status + mof_last_error

namespace mof {

constexpr int kRbfMaxE = 256;         // electrodes: 64 K-chunks of one vertex tile fill a wave's phi registers
constexpr int kRbfPhiRegs = 64;       // phi values per lane: NT vertex tiles x KC K-chunks
// K-chunks whose operands are loaded ahead together: the largest group that
// leaves the real-data kernel two waves per SIMD (16 at NT = 4 took 266 registers)
constexpr int rbf_group(int nt) { return nt == 4 ? 8 : 16; }
constexpr int kRbfPassFrames = 4096;  // frames per pass at most: the padded weights stay within 16 MiB
constexpr int kRbfTilesPerWG = 8;     // frame tiles a workgroup walks at least (when the pass has them): phi's cost is spread over them
constexpr int kRbfGridTarget = 1024;  // workgroups wanted before the frame tiles stop being split over grid.y
// automatic passes from host memory: at most this many bytes of staged output
constexpr int64_t kRbfStageBytes = (int64_t)256 << 20;
std::atomic<int> g_rbf_pass{0};  // tests only (mof_test_rbf_pass): frames per pass, 0 = auto

typedef double f64x4 __attribute__((ext_vector_type(4)));

// Wp[plane][tile][c][lane], c < nkp: the A operand of frame tile `tile` and
// K-chunk c as lane l reads it, W[16 tile + (l & 15)][4 c + (l >> 4)] of the
// pass's rows [0, rows) x E columns, zeros elsewhere
__global__ __launch_bounds__(kWG) void k_rbf_pack(const double *__restrict__ W_re, const double *__restrict__ W_im,
                                                  int32_t rows, int32_t E, int32_t ntile, int32_t nkp,
                                                  double *__restrict__ Wp) {
    const int64_t per = (int64_t)ntile * nkp * 64;
    const int64_t idx = (int64_t)blockIdx.x * kWG + threadIdx.x;
    if (idx >= per) return;
    const int lane = (int)(idx & 63);
    const int32_t c = (int32_t)((idx >> 6) % nkp), tile = (int32_t)((idx >> 6) / nkp);
    const int32_t t = tile * 16 + (lane & 15), e = 4 * c + (lane >> 4);
    const bool live = t < rows && e < E;
    Wp[idx] = live ? W_re[(int64_t)t * E + e] : 0.0;
    if (W_im) Wp[per + idx] = live ? W_im[(int64_t)t * E + e] : 0.0;
}

// the A operands of G chunks from p (this lane's column of the packed weights)
template <bool CPLX, int G>
__device__ __forceinline__ void rbf_load(const double *__restrict__ p, int64_t plane, double (&a)[G], double (&b)[G]) {
#pragma unroll
    for (int cc = 0; cc < G; ++cc) {
        a[cc] = p[cc * 64];
        if (CPLX) b[cc] = p[plane + cc * 64];
    }
}

// Workgroup (x, y): the 64 NT vertices from 64 NT x (16 NT per wave) and the
// frame tiles y, y + gridDim.y, ... of the pass. MODE 0: real weights; 1: two
// planes into out and out_im; 2: out = atan2(im, re). The operands of the next
// group of chunks -- of this frame tile or of the next -- are loaded while
// the products of the current one run: at most two waves share a SIMD (phi
// takes half of a wave's registers), too few to hide the loads otherwise.
template <int NT, int MODE>
__global__ __launch_bounds__(kWG) void k_rbf_eval(const double *__restrict__ pts, int32_t N,
                                                  const double *__restrict__ el, int32_t E, int32_t nk,
                                                  double inv_eps, const double *__restrict__ Wp, int32_t ntile,
                                                  int32_t frames, double *__restrict__ out,
                                                  double *__restrict__ out_im) {
    constexpr int KC = kRbfPhiRegs / NT, G = rbf_group(NT), NG = KC / G;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fr = lane & 15, fk = lane >> 4;
    const int64_t vb = ((int64_t)blockIdx.x * (kWG / 64) + wave) * (16 * NT);
    if (vb >= N) return;  // the whole wave: no barrier follows

    double px[NT], py[NT], pz[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        int64_t v = vb + 16 * j + fr;
        if (v >= N) v = (int64_t)N - 1;  // a padding column: read in bounds, never stored
        px[j] = pts[3 * v];
        py[j] = pts[3 * v + 1];
        pz[j] = pts[3 * v + 2];
    }
    double phi[NT][KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) {
#pragma unroll
        for (int j = 0; j < NT; ++j) phi[j][c] = 0.0;
        if (c < nk) {
            int32_t e = 4 * c + fk;
            if (e >= E) e = 0;  // a padding column: its weights are zeros, its phi stays finite
            const double ex = el[3 * e], ey = el[3 * e + 1], ez = el[3 * e + 2];
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const double dx = px[j] - ex, dy = py[j] - ey, dz = pz[j] - ez;
                const double r = __dsqrt_rn((dx * dx + dy * dy) + dz * dz);
                const double q = inv_eps * r;
                phi[j][c] = __dsqrt_rn(q * q + 1.0);
            }
        }
    }

    const int32_t ng = (nk + G - 1) / G, nkp = ng * G;
    const int64_t plane = (int64_t)ntile * nkp * 64;
    const int32_t step = (int32_t)gridDim.y;
    double a[G], b[G], na[G], nb[G];
#pragma unroll
    for (int cc = 0; cc < G; ++cc) a[cc] = b[cc] = na[cc] = nb[cc] = 0.0;
    int32_t tile = (int32_t)blockIdx.y;
    if (tile < ntile) rbf_load<MODE != 0, G>(Wp + (int64_t)tile * nkp * 64 + lane, plane, a, b);
    for (; tile < ntile; tile += step) {
        f64x4 re[NT], im[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            re[j] = (f64x4){0.0, 0.0, 0.0, 0.0};
            im[j] = (f64x4){0.0, 0.0, 0.0, 0.0};
        }
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            if (g < ng) {
                if (g + 1 < NG && g + 1 < ng)
                    rbf_load<MODE != 0, G>(Wp + ((int64_t)tile * nkp + (g + 1) * G) * 64 + lane, plane, na, nb);
                else if (tile + step < ntile)
                    rbf_load<MODE != 0, G>(Wp + (int64_t)(tile + step) * nkp * 64 + lane, plane, na, nb);
#pragma unroll
                for (int cc = 0; cc < G; ++cc) {
                    const int c = g * G + cc;
                    if (c < nk) {
#pragma unroll
                        for (int j = 0; j < NT; ++j) {
                            re[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[cc], phi[j][c], re[j], 0, 0, 0);
                            if (MODE) im[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(b[cc], phi[j][c], im[j], 0, 0, 0);
                        }
                    }
                }
#pragma unroll
                for (int cc = 0; cc < G; ++cc) {
                    a[cc] = na[cc];
                    b[cc] = nb[cc];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int64_t v = vb + 16 * j + fr;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int32_t t = tile * 16 + fk + 4 * g;
                if (t < frames && v < N) {
                    const int64_t o = (int64_t)t * N + v;
                    if (MODE == 2) {
                        out[o] = atan2(im[j][g], re[j][g]);
                    } else {
                        out[o] = re[j][g];
                        if (MODE == 1) out_im[o] = im[j][g];
                    }
                }
            }
        }
    }
}

namespace {

struct DeviceGuard {
    int prev = 0;
    explicit DeviceGuard(int d) {
        (void)hipGetDevice(&prev);
        MOF_HIP(hipSetDevice(d));
    }
    ~DeviceGuard() { (void)hipSetDevice(prev); }
};

void check_device(int32_t device) {
    int ndev = 0;
    MOF_HIP(hipGetDeviceCount(&ndev));
    MOF_REQUIRE(device >= 0 && device < ndev, "device ordinal out of range");
}

template <int NT>
void launch_eval(int mode, dim3 grid, hipStream_t s, const double *pts, int32_t N, const double *el, int32_t E,
                 int32_t nk, double inv_eps, const double *Wp, int32_t ntile, int32_t frames, double *out,
                 double *out_im) {
    if (mode == 0)
        k_rbf_eval<NT, 0><<<grid, kWG, 0, s>>>(pts, N, el, E, nk, inv_eps, Wp, ntile, frames, out, out_im);
    else if (mode == 1)
        k_rbf_eval<NT, 1><<<grid, kWG, 0, s>>>(pts, N, el, E, nk, inv_eps, Wp, ntile, frames, out, out_im);
    else
        k_rbf_eval<NT, 2><<<grid, kWG, 0, s>>>(pts, N, el, E, nk, inv_eps, Wp, ntile, frames, out, out_im);
    MOF_HIP(hipGetLastError());
}

// mode 0: real; 1: complex planes; 2: angle
void rbf_eval(const double *points, int32_t N, const double *electrodes, int32_t E, double epsilon,
              const double *W_re, const double *W_im, int32_t T, int mode, bool dev_io, hipStream_t s, double *out,
              double *out_im) {
    const int32_t nk = (E + 3) / 4;
    const int nt = nk <= 16 ? 4 : nk <= 32 ? 2 : 1;  // vertex tiles per wave: nt * nk <= 64 phi registers
    const int32_t grp = rbf_group(nt), nkp = (nk + grp - 1) / grp * grp;  // whole groups: the loads ahead need no guard
    const int planes_in = mode ? 2 : 1, planes_out = mode == 1 ? 2 : 1;
    const double inv_eps = 1.0 / epsilon;

    int64_t pass = kRbfPassFrames;
    const int32_t hook = g_rbf_pass.load();
    if (hook > 0)
        pass = hook;
    else if (!dev_io)
        pass = std::max<int64_t>(1, std::min<int64_t>(pass, kRbfStageBytes / ((int64_t)N * 8 * planes_out)));
    pass = std::min<int64_t>(pass, T);
    const int32_t ntile_max = (int32_t)((pass + 15) / 16);

    DevArray<double> Wp, dpts, del, dW, dout;
    Wp.alloc((size_t)planes_in * ntile_max * nkp * 64);
    const double *pd = points, *ed = electrodes;
    if (!dev_io) {
        dpts.alloc((size_t)N * 3);
        dpts.upload(points, (size_t)N * 3, s);
        pd = dpts.p;
        del.alloc((size_t)E * 3);
        del.upload(electrodes, (size_t)E * 3, s);
        ed = del.p;
        dW.alloc((size_t)planes_in * pass * E);
        dout.alloc((size_t)planes_out * pass * N);
    }
    const unsigned nvb = (unsigned)(((int64_t)N + 64 * nt - 1) / (64 * nt));
    for (int32_t t0 = 0; t0 < T; t0 += (int32_t)pass) {
        const int32_t frames = (int32_t)std::min<int64_t>(pass, T - t0);
        const int32_t ntile = (frames + 15) / 16;
        const double *wr = W_re + (int64_t)t0 * E, *wi = mode ? W_im + (int64_t)t0 * E : nullptr;
        double *o = out + (int64_t)t0 * N, *oi = mode == 1 ? out_im + (int64_t)t0 * N : nullptr;
        if (!dev_io) {
            dW.upload(wr, (size_t)frames * E, s);
            wr = dW.p;
            if (mode) {
                MOF_HIP(hipMemcpyAsync(dW.p + (size_t)pass * E, wi, (size_t)frames * E * 8, hipMemcpyHostToDevice, s));
                wi = dW.p + (size_t)pass * E;
            }
            o = dout.p;
            oi = mode == 1 ? dout.p + (size_t)pass * N : nullptr;
        }
        const int64_t per = (int64_t)ntile * nkp * 64;
        k_rbf_pack<<<(unsigned)((per + kWG - 1) / kWG), kWG, 0, s>>>(wr, wi, frames, E, ntile, nkp, Wp.p);
        MOF_HIP(hipGetLastError());
        // the frame tiles over grid.y only as far as the vertex blocks leave the device idle
        int64_t gy = std::max<int64_t>(1, kRbfGridTarget / nvb);
        gy = std::min<int64_t>(gy, std::max<int32_t>(1, ntile / kRbfTilesPerWG));
        const dim3 grid(nvb, (unsigned)gy);
        if (nt == 4)
            launch_eval<4>(mode, grid, s, pd, N, ed, E, nk, inv_eps, Wp.p, ntile, frames, o, oi);
        else if (nt == 2)
            launch_eval<2>(mode, grid, s, pd, N, ed, E, nk, inv_eps, Wp.p, ntile, frames, o, oi);
        else
            launch_eval<1>(mode, grid, s, pd, N, ed, E, nk, inv_eps, Wp.p, ntile, frames, o, oi);
        if (!dev_io) {
            MOF_HIP(hipMemcpyAsync(out + (int64_t)t0 * N, o, (size_t)frames * N * 8, hipMemcpyDeviceToHost, s));
            if (mode == 1)
                MOF_HIP(hipMemcpyAsync(out_im + (int64_t)t0 * N, oi, (size_t)frames * N * 8, hipMemcpyDeviceToHost,
                                       s));
        }
    }
    MOF_HIP(hipStreamSynchronize(s));  // the workspace leaves scope
}

}  // namespace
}  // namespace mof

extern "C" {

int mof_rbf_eval(int32_t device, const double *points, int32_t N, const double *electrodes, int32_t E,
                 double epsilon, const double *W_re, const double *W_im, int32_t T, uint32_t flags, void *stream,
                 double *out, double *out_im) {
    return mof_io_guard([&] {
        MOF_REQUIRE(N >= 1 && E >= 1 && T >= 1, "N < 1 points, E < 1 electrodes or T < 1 frames");
        MOF_REQUIRE(E <= mof::kRbfMaxE, "E exceeds " + std::to_string(mof::kRbfMaxE) + " electrodes");
        MOF_REQUIRE(std::isfinite(epsilon) && epsilon > 0.0, "epsilon is not a finite positive number");
        MOF_REQUIRE(points && electrodes && W_re && out, "points, electrodes, W_re or out is NULL");
        const bool angle = (flags & MOF_RBF_ANGLE) != 0;
        MOF_REQUIRE(!angle || W_im, "W_im is NULL with MOF_RBF_ANGLE");
        MOF_REQUIRE(!W_im || angle || out_im, "out_im is NULL with W_im and without MOF_RBF_ANGLE");
        mof::check_device(device);
        mof::DeviceGuard dg(device);
        mof::rbf_eval(points, N, electrodes, E, epsilon, W_re, W_im, T, angle ? 2 : W_im ? 1 : 0,
                      (flags & MOF_IO_DEVICE) != 0, (hipStream_t)stream, out, out_im);
    });
}

int mof_test_rbf_pass(int32_t frames) {
    mof::g_rbf_pass.store(frames > 0 ? frames : 0);
    return MOF_OK;
}

}  // extern "C"
