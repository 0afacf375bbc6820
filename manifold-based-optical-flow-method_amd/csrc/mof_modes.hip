// mof_modes.hip -- spatiotemporal modes of the velocity fields (mof_modes_gram,
// mof_modes_project, include/mof.h): the device half of the reference's two
// S4_spatiotemporal_decomposition_* scripts by the method of snapshots.
//
// The scripts take np.linalg.svd of the K x N complex matrix X = V1 + i V2
// (ComplexMatrices) or of the real K x 2N matrix [V1 | V2] (ConcatMatrices),
// V = [V1 | V2] the planar (K, 2N) fields. With K << N the left vectors and the
// singular values are those of the K x K Gram matrix, X X^H = S + i A or S:
//   1. k_modes_gram: S = V V^T over all 2N columns and A = V2 V1^T - V1 V2^T on
//      v_mfma_f64_16x16x4_f64. One workgroup accumulates one (64 x 64 block pair
//      bi <= bj, chunk of kModesChunk columns) into a workspace slot;
//      k_modes_reduce adds the chunks to the running sums in ascending order and
//      mirrors: S exactly symmetric, A exactly antisymmetric, no atomics.
//   2. the K x K eigenproblem is the caller's (mofhip/modes.py: numpy eigh).
//   3. k_modes_project: Y = W^H X for the first r eigenvectors W = P + i Q, in
//      V's planar layout (r, 2N): one thread owns a column and walks the K rows
//      in ascending order, so Y does not depend on how the rows are split into
//      passes. k_modes_norm2 / k_modes_norm: sigma_r[j] = |Y_j| in a fixed order.
// The chunk length is the only thing that fixes the summation order of pass 1:
// it is a library constant, independent of K, of the device and of the pass.
#include <algorithm>
#include <cmath>

#include "mof_internal.h"

int mof_io_guard(const std::function<void()> &f);  // mof_abi.cpp: status + mof_last_error

namespace mof {

constexpr int kModesChunk = 2048;    // columns of N per workspace slot: fixes the summation order
constexpr int kModesMaxK = 8192;     // fields: 128 row blocks, 8256 block pairs, S and A 512 MiB each
constexpr int kModesMaxN = 1 << 29;  // vertices: the 2N column indices stay within int32
constexpr int kMB = 64;              // rows of a block: 4 tiles of 16, one tile row per wave
constexpr int kMW = 16;              // columns staged per step: 4 k-steps of the 16x16x4 product
constexpr int kMLd = kMW + 2;        // LDS row stride in doubles: 18 r + c is distinct mod 32 over 16 rows x 2 columns
constexpr int kProjR = 4;            // modes per projection launch (the scripts' nmodeplot)
constexpr int kProjRows = 256;       // rows of coefficients in LDS at a time
constexpr int kNormSeg = 4096;       // columns per partial sum of a row norm
// automatic passes: at most this many bytes of Gram workspace / of staged V
constexpr int64_t kModesWsBytes = (int64_t)256 << 20;
constexpr int64_t kModesStageBytes = (int64_t)256 << 20;
std::atomic<int> g_modes_chunk{0};      // tests only (mof_test_modes_chunk): columns per chunk, 0 = kModesChunk
std::atomic<int> g_modes_pass_rows{0};  // tests only (mof_test_modes_pass): rows of V per pass, 0 = auto

typedef double f64x4 __attribute__((ext_vector_type(4)));

// One (block pair, chunk): rows [64 bi, +64) x rows [64 bj, +64) over the
// columns [c0, c1) of V1 and V2 (row stride ld). Wave w owns the tile row w of
// the block: four 16 x 16 tiles of S and, with CPLX, of A -- independent
// accumulators. A diagonal block computes all 16 tiles although only those
// with t >= w are read (6 of 16 tiles of nB of the nB (nB + 1) / 2 blocks, 3 %
// at K = 1536): skipping them per wave put a branch round every product and
// took the kernel from 148 to 360 registers and from 37 to 128 ms on C3.
// Operands: lane l holds A[l & 15][k = l >> 4] and B[k = l >> 4][l & 15],
// both read from the LDS image [row][column]; the f64 result map is
// col = l & 15, row = (l >> 4) + 4 reg. Rows >= K and columns >= c1 are staged
// as zeros. VEC: 16-byte loads (both halves 16-byte aligned).
template <bool CPLX, bool VEC>
__global__ __launch_bounds__(kWG) void k_modes_gram(const double *__restrict__ V1, const double *__restrict__ V2,
                                                    int64_t ld, int32_t K, int32_t ncols, int32_t chunk, int32_t nB,
                                                    double *__restrict__ ws) {
    __shared__ double sm[2][2][kMB][kMLd];  // [block i / j][half][row][column]
    int32_t bi = 0, rem = (int32_t)blockIdx.x;
    while (rem >= nB - bi) {
        rem -= nB - bi;
        ++bi;
    }
    const int32_t bj = bi + rem;
    const bool diag = bi == bj;
    const int32_t c0 = (int32_t)blockIdx.y * chunk;
    const int32_t c1 = min(c0 + chunk, ncols);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fk = lane >> 4;

    f64x4 accS[4], accA[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        accS[t] = (f64x4){0.0, 0.0, 0.0, 0.0};
        accA[t] = (f64x4){0.0, 0.0, 0.0, 0.0};
    }
    for (int32_t c = c0; c < c1; c += kMW) {
        // stage: 2 blocks x 2 halves x 64 rows x 16 columns
        if (VEC) {
            // 8 double2 per row and half: 2 x 2 x 64 x 8 = 2048 loads, 8 per thread
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const int q = tid + it * kWG;
                const int cc = (q & 7) * 2, row = (q >> 3) & 63, half = (q >> 9) & 1, blk = q >> 10;
                if (blk == 1 && diag) continue;
                const int32_t gr = (blk ? bj : bi) * kMB + row, gc = c + cc;
                double2 v = make_double2(0.0, 0.0);
                if (gr < K) {
                    const double *src = (half ? V2 : V1) + (int64_t)gr * ld + gc;
                    if (gc + 1 < c1)
                        v = *reinterpret_cast<const double2 *>(src);
                    else if (gc < c1)
                        v.x = src[0];
                }
                sm[blk][half][row][cc] = v.x;
                sm[blk][half][row][cc + 1] = v.y;
            }
        } else {
#pragma unroll
            for (int it = 0; it < 16; ++it) {
                const int q = tid + it * kWG;
                const int cc = q & 15, row = (q >> 4) & 63, half = (q >> 10) & 1, blk = q >> 11;
                if (blk == 1 && diag) continue;
                const int32_t gr = (blk ? bj : bi) * kMB + row, gc = c + cc;
                double v = 0.0;
                if (gr < K && gc < c1) v = (half ? V2 : V1)[(int64_t)gr * ld + gc];
                sm[blk][half][row][cc] = v;
            }
        }
        __syncthreads();
        const int jb = diag ? 0 : 1;
#pragma unroll
        for (int kk = 0; kk < kMW; kk += 4) {
            const double a1 = sm[0][0][wave * 16 + fr][kk + fk];
            const double a2 = sm[0][1][wave * 16 + fr][kk + fk];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const double b1 = sm[jb][0][t * 16 + fr][kk + fk];
                const double b2 = sm[jb][1][t * 16 + fr][kk + fk];
                accS[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, accS[t], 0, 0, 0);
                accS[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, b2, accS[t], 0, 0, 0);
                if (CPLX) {
                    accA[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, b1, accA[t], 0, 0, 0);
                    accA[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(-a1, b2, accA[t], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }
    // slot [pair][chunk of the pass][S, A][64][64]
    const int nmat = CPLX ? 2 : 1;
    double *slot = ws + ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * (int64_t)(nmat * kMB * kMB);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int row = wave * 16 + fk + 4 * g, col = t * 16 + fr;
            slot[row * kMB + col] = accS[t][g];
            if (CPLX) slot[kMB * kMB + row * kMB + col] = accA[t][g];
        }
}

// The running sums over the chunks so far, one thread per (i, j) with i <= j:
// S[i][j] (+)= slot 0 + slot 1 + ... of this pass, one after the other, and the
// mirror image. `first`: the sums start at 0 (a pass boundary changes nothing:
// the running value goes through memory unrounded).
template <bool CPLX>
__global__ __launch_bounds__(kWG) void k_modes_reduce(int32_t K, int32_t nB, int32_t nchunk, int32_t first,
                                                      const double *__restrict__ ws, double *__restrict__ S,
                                                      double *__restrict__ A) {
    const int64_t idx = (int64_t)blockIdx.x * kWG + threadIdx.x;
    if (idx >= (int64_t)K * K) return;
    const int32_t i = (int32_t)(idx / K), j = (int32_t)(idx % K);
    if (i > j) return;
    const int32_t bi = i / kMB, bj = j / kMB;
    // pair index of (bi, bj): the rows before bi hold nB, nB - 1, ... pairs
    const int64_t p = (int64_t)bi * nB - (int64_t)bi * (bi - 1) / 2 + (bj - bi);
    const int nmat = CPLX ? 2 : 1;
    const double *src = ws + p * nchunk * (int64_t)(nmat * kMB * kMB) + (i % kMB) * kMB + (j % kMB);
    double s = first ? 0.0 : S[(int64_t)i * K + j];
    double a = (!CPLX || first) ? 0.0 : A[(int64_t)i * K + j];
    for (int32_t c = 0; c < nchunk; ++c) {
        s += src[(int64_t)c * (nmat * kMB * kMB)];
        if (CPLX) a += src[(int64_t)c * (nmat * kMB * kMB) + kMB * kMB];
    }
    S[(int64_t)i * K + j] = s;
    S[(int64_t)j * K + i] = s;
    if (CPLX) {
        if (i == j) a = 0.0;
        A[(int64_t)i * K + j] = a;
        A[(int64_t)j * K + i] = 0.0 - a;
    }
}

// Y[j0 + m] (+)= sum over the rows [k0, k1) of this pass, ascending, for the
// modes m < R of one launch. CPLX: thread = column n < N,
//   Y[j][n] += P[k][j] V1[k][n] + Q[k][j] V2[k][n], Y[j][N + n] += P[k][j] V2[k][n] - Q[k][j] V1[k][n];
// else thread = column c < 2N, Y[j][c] += P[k][j] V[k][c]. V holds the rows of
// the pass (row stride 2N); P, Q (K, r) row-major. The coefficients of 256
// rows at a time sit in LDS and are read at a wave-uniform address.
template <bool CPLX>
__global__ __launch_bounds__(kWG) void k_modes_project(const double *__restrict__ V, int32_t N, int32_t k0,
                                                       int32_t k1, const double *__restrict__ P,
                                                       const double *__restrict__ Q, int32_t r, int32_t j0,
                                                       int32_t first, double *__restrict__ Y) {
    __shared__ double cf[kProjRows][2 * kProjR];
    const int32_t ncol = CPLX ? N : 2 * N;
    const int64_t ld = 2 * (int64_t)N;
    const int32_t n = (int32_t)(blockIdx.x * kWG + threadIdx.x);
    const bool live = n < ncol;
    const int R = min(kProjR, r - j0);
    double re[kProjR], im[kProjR];
#pragma unroll
    for (int m = 0; m < kProjR; ++m) {
        re[m] = im[m] = 0.0;
        if (!first && live && m < R) {
            re[m] = Y[(int64_t)(j0 + m) * ld + n];
            if (CPLX) im[m] = Y[(int64_t)(j0 + m) * ld + N + n];
        }
    }
    for (int32_t kb = k0; kb < k1; kb += kProjRows) {
        const int32_t rows = min(kProjRows, k1 - kb);
        __syncthreads();
        for (int q = threadIdx.x; q < rows * 2 * kProjR; q += kWG) {
            const int row = q / (2 * kProjR), m = q % (2 * kProjR);
            double v = 0.0;
            if ((m & 3) < R) {
                const double *src = m < kProjR ? P : Q;
                if (src) v = src[(int64_t)(kb + row) * r + j0 + (m & 3)];
            }
            cf[row][m] = v;
        }
        __syncthreads();
        if (!live) continue;
        const double *v1p = V + (int64_t)(kb - k0) * ld + n;
#pragma unroll 4
        for (int32_t k = 0; k < rows; ++k) {
            const double v1 = v1p[(int64_t)k * ld];
            if (CPLX) {
                const double v2 = v1p[(int64_t)k * ld + N];
#pragma unroll
                for (int m = 0; m < kProjR; ++m) {
                    const double p = cf[k][m], q = cf[k][kProjR + m];
                    re[m] = fma(q, v2, fma(p, v1, re[m]));
                    im[m] = fma(-q, v1, fma(p, v2, im[m]));
                }
            } else {
#pragma unroll
                for (int m = 0; m < kProjR; ++m) re[m] = fma(cf[k][m], v1, re[m]);
            }
        }
    }
    if (!live) return;
#pragma unroll
    for (int m = 0; m < kProjR; ++m)
        if (m < R) {
            Y[(int64_t)(j0 + m) * ld + n] = re[m];
            if (CPLX) Y[(int64_t)(j0 + m) * ld + N + n] = im[m];
        }
}

// |Y_j|^2 over the segment [4096 b, +4096) of the 2N columns: thread t adds its
// columns t, t + 256, ... in ascending order, then a tree over the threads.
__global__ __launch_bounds__(kWG) void k_modes_norm2(const double *__restrict__ Y, int64_t ld, int32_t nseg,
                                                     double *__restrict__ part) {
    __shared__ double red[kWG];
    const int32_t j = blockIdx.y, b = blockIdx.x;
    const int64_t c1 = min((int64_t)(b + 1) * kNormSeg, ld);
    double s = 0.0;
    for (int64_t c = (int64_t)b * kNormSeg + threadIdx.x; c < c1; c += kWG) {
        const double y = Y[(int64_t)j * ld + c];
        s = fma(y, y, s);
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = kWG / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[(int64_t)j * nseg + b] = red[0];
}

// sigma_r[j] = sqrt of the segments' sums, added in ascending order
__global__ void k_modes_norm(int32_t r, int32_t nseg, const double *__restrict__ part, double *__restrict__ sigma) {
    const int32_t j = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (j >= r) return;
    double s = 0.0;
    for (int32_t b = 0; b < nseg; ++b) s += part[(int64_t)j * nseg + b];
    sigma[j] = sqrt(s);
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

int32_t modes_chunk() {
    const int c = g_modes_chunk.load();
    return c > 0 ? c : kModesChunk;
}

void check_device(int32_t device) {
    int ndev = 0;
    MOF_HIP(hipGetDeviceCount(&ndev));
    MOF_REQUIRE(device >= 0 && device < ndev, "device ordinal out of range");
}

template <bool CPLX>
void launch_gram(bool vec, dim3 grid, hipStream_t s, const double *V1, const double *V2, int64_t ld, int32_t K,
                 int32_t ncols, int32_t chunk, int32_t nB, double *ws) {
    if (vec)
        k_modes_gram<CPLX, true><<<grid, kWG, 0, s>>>(V1, V2, ld, K, ncols, chunk, nB, ws);
    else
        k_modes_gram<CPLX, false><<<grid, kWG, 0, s>>>(V1, V2, ld, K, ncols, chunk, nB, ws);
    MOF_HIP(hipGetLastError());
}

void modes_gram(const double *V, int32_t K, int32_t N, bool cplx, bool dev_io, hipStream_t s, double *S, double *A) {
    const int32_t chunk = modes_chunk();
    const int32_t nchunk = (N + chunk - 1) / chunk;
    const int32_t nB = (K + kMB - 1) / kMB;
    const int64_t npair = (int64_t)nB * (nB + 1) / 2;
    const int nmat = cplx ? 2 : 1;
    const int64_t slot = (int64_t)nmat * kMB * kMB;
    // chunks per pass: the workspace (and, from host memory, the staged
    // columns of V) stay within their budgets whatever N is
    int64_t per = std::max<int64_t>(1, kModesWsBytes / (npair * slot * 8));
    const int32_t hook = g_modes_pass_rows.load();
    if (hook > 0)  // tests: a pass stages at most hook * 2N values of V
        per = std::max<int64_t>(1, (int64_t)hook * 2 * N / ((int64_t)K * 2 * chunk));
    else if (!dev_io)
        per = std::max<int64_t>(1, std::min(per, kModesStageBytes / ((int64_t)K * 2 * chunk * 8)));
    per = std::min<int64_t>(std::min<int64_t>(per, nchunk), 65535);

    DevArray<double> ws, stage, dS, dA;
    ws.alloc((size_t)(npair * per * slot));
    double *Sd = S, *Ad = A;
    const size_t kk = (size_t)K * K;
    if (!dev_io) {
        stage.alloc((size_t)K * 2 * per * chunk);
        dS.alloc(kk);
        Sd = dS.p;
        if (cplx) {
            dA.alloc(kk);
            Ad = dA.p;
        }
    }
    const int64_t ld2N = 2 * (int64_t)N;
    for (int32_t ch0 = 0; ch0 < nchunk; ch0 += (int32_t)per) {
        const int32_t nch = (int32_t)std::min<int64_t>(per, nchunk - ch0);
        const int32_t col0 = ch0 * chunk;
        const int32_t ncols = std::min<int64_t>((int64_t)nch * chunk, N - col0);
        const double *V1, *V2;
        int64_t ld;
        if (dev_io) {
            V1 = V + col0;
            V2 = V + N + col0;
            ld = ld2N;
        } else {
            // the columns of the pass, both halves: [K][2][ncols rounded up to even]
            const int64_t w = (ncols + 1) & ~(int64_t)1;
            ld = 2 * w;
            MOF_HIP(hipMemcpy2DAsync(stage.p, ld * 8, V + col0, ld2N * 8, (size_t)ncols * 8, K,
                                     hipMemcpyHostToDevice, s));
            MOF_HIP(hipMemcpy2DAsync(stage.p + w, ld * 8, V + N + col0, ld2N * 8, (size_t)ncols * 8, K,
                                     hipMemcpyHostToDevice, s));
            V1 = stage.p;
            V2 = stage.p + w;
        }
        const bool vec = ((uintptr_t)V1 % 16 == 0) && ((uintptr_t)V2 % 16 == 0) && (ld % 2 == 0);
        const dim3 grid((unsigned)npair, (unsigned)nch);
        if (cplx)
            launch_gram<true>(vec, grid, s, V1, V2, ld, K, ncols, chunk, nB, ws.p);
        else
            launch_gram<false>(vec, grid, s, V1, V2, ld, K, ncols, chunk, nB, ws.p);
        const unsigned rb = (unsigned)((kk + kWG - 1) / kWG);
        if (cplx)
            k_modes_reduce<true><<<rb, kWG, 0, s>>>(K, nB, nch, ch0 == 0, ws.p, Sd, Ad);
        else
            k_modes_reduce<false><<<rb, kWG, 0, s>>>(K, nB, nch, ch0 == 0, ws.p, Sd, nullptr);
        MOF_HIP(hipGetLastError());
    }
    if (!dev_io) {
        MOF_HIP(hipMemcpyAsync(S, Sd, kk * 8, hipMemcpyDeviceToHost, s));
        if (cplx) MOF_HIP(hipMemcpyAsync(A, Ad, kk * 8, hipMemcpyDeviceToHost, s));
    }
    MOF_HIP(hipStreamSynchronize(s));  // the workspace leaves scope
}

void modes_project(const double *V, int32_t K, int32_t N, const double *P, const double *Q, int32_t r, bool cplx,
                   bool dev_io, hipStream_t s, double *Y, double *sigma) {
    const int64_t ld = 2 * (int64_t)N;
    const int32_t hook = g_modes_pass_rows.load();
    int32_t rows = K;
    if (hook > 0)
        rows = std::min(hook, K);
    else if (!dev_io)
        rows = (int32_t)std::max<int64_t>(1, std::min<int64_t>(K, kModesStageBytes / (ld * 8)));
    DevArray<double> stage, dP, dQ, dY, dsig, part;
    const double *Pd = P, *Qd = Q;
    double *Yd = Y, *sd = sigma;
    if (!dev_io) {
        stage.alloc((size_t)rows * ld);
        dP.alloc((size_t)K * r);
        dP.upload(P, (size_t)K * r, s);
        Pd = dP.p;
        if (cplx) {
            dQ.alloc((size_t)K * r);
            dQ.upload(Q, (size_t)K * r, s);
            Qd = dQ.p;
        }
        dY.alloc((size_t)r * ld);
        Yd = dY.p;
        if (sigma) {
            dsig.alloc((size_t)r);
            sd = dsig.p;
        }
    }
    if (!cplx) Qd = nullptr;
    const int32_t ncol = cplx ? N : 2 * N;
    const unsigned nblk = (unsigned)((ncol + kWG - 1) / kWG);
    for (int32_t k0 = 0; k0 < K; k0 += rows) {
        const int32_t k1 = std::min(K, k0 + rows);
        const double *Vp = V + (int64_t)k0 * ld;
        if (!dev_io) {
            stage.upload(Vp, (size_t)(k1 - k0) * ld, s);
            Vp = stage.p;
        }
        for (int32_t j0 = 0; j0 < r; j0 += kProjR) {
            if (cplx)
                k_modes_project<true><<<nblk, kWG, 0, s>>>(Vp, N, k0, k1, Pd, Qd, r, j0, k0 == 0, Yd);
            else
                k_modes_project<false><<<nblk, kWG, 0, s>>>(Vp, N, k0, k1, Pd, Qd, r, j0, k0 == 0, Yd);
            MOF_HIP(hipGetLastError());
        }
    }
    if (sigma) {
        const int32_t nseg = (int32_t)((ld + kNormSeg - 1) / kNormSeg);
        part.alloc((size_t)r * nseg);
        // one launch per 65535 modes: the grid's y extent
        for (int32_t j0 = 0; j0 < r; j0 += 65535) {
            const int32_t rr = std::min(65535, r - j0);
            k_modes_norm2<<<dim3((unsigned)nseg, (unsigned)rr), kWG, 0, s>>>(Yd + (int64_t)j0 * ld, ld, nseg,
                                                                            part.p + (int64_t)j0 * nseg);
            MOF_HIP(hipGetLastError());
        }
        k_modes_norm<<<(unsigned)((r + kWG - 1) / kWG), kWG, 0, s>>>(r, nseg, part.p, sd);
        MOF_HIP(hipGetLastError());
    }
    if (!dev_io) {
        MOF_HIP(hipMemcpyAsync(Y, Yd, (size_t)r * ld * 8, hipMemcpyDeviceToHost, s));
        if (sigma) MOF_HIP(hipMemcpyAsync(sigma, sd, (size_t)r * 8, hipMemcpyDeviceToHost, s));
    }
    MOF_HIP(hipStreamSynchronize(s));  // the staging buffers leave scope
}

}  // namespace
}  // namespace mof

extern "C" {

int mof_modes_gram(int32_t device, const double *V, int32_t K, int32_t N, uint32_t flags, void *stream, double *S,
                   double *A) {
    return mof_io_guard([&] {
        MOF_REQUIRE(K >= 1 && N >= 1, "K < 1 fields or N < 1 vertices");
        MOF_REQUIRE(K <= mof::kModesMaxK, "K exceeds " + std::to_string(mof::kModesMaxK) +
                                              " fields: the K x K Gram matrix is meant to be small");
        MOF_REQUIRE(N <= mof::kModesMaxN, "N exceeds 2^29 vertices");
        const bool cplx = (flags & MOF_MODES_COMPLEX) != 0;
        MOF_REQUIRE(V && S, "V or S is NULL");
        MOF_REQUIRE(!cplx || A, "A is NULL with MOF_MODES_COMPLEX");
        mof::check_device(device);
        mof::DeviceGuard dg(device);
        mof::modes_gram(V, K, N, cplx, (flags & MOF_IO_DEVICE) != 0, (hipStream_t)stream, S, A);
    });
}

int mof_modes_project(int32_t device, const double *V, int32_t K, int32_t N, const double *P, const double *Q,
                      int32_t r, uint32_t flags, void *stream, double *Y, double *sigma_r) {
    return mof_io_guard([&] {
        MOF_REQUIRE(K >= 1 && N >= 1, "K < 1 fields or N < 1 vertices");
        MOF_REQUIRE(r >= 1 && r <= K, "r modes outside 1 .. K");
        MOF_REQUIRE(K <= mof::kModesMaxK, "K exceeds " + std::to_string(mof::kModesMaxK) + " fields");
        MOF_REQUIRE(N <= mof::kModesMaxN, "N exceeds 2^29 vertices");
        const bool cplx = (flags & MOF_MODES_COMPLEX) != 0;
        MOF_REQUIRE(V && P && Y, "V, P or Y is NULL");
        MOF_REQUIRE(!cplx || Q, "Q is NULL with MOF_MODES_COMPLEX");
        mof::check_device(device);
        mof::DeviceGuard dg(device);
        mof::modes_project(V, K, N, P, Q, r, cplx, (flags & MOF_IO_DEVICE) != 0, (hipStream_t)stream, Y, sigma_r);
    });
}

int mof_test_modes_chunk(int32_t cols) {
    // whole staging steps, so a chunk boundary never splits a 4-column product
    mof::g_modes_chunk.store(cols > 0 ? (cols + mof::kMW - 1) / mof::kMW * mof::kMW : 0);
    return MOF_OK;
}

int mof_test_modes_pass(int32_t rows) {
    mof::g_modes_pass_rows.store(rows > 0 ? rows : 0);
    return MOF_OK;
}

}  // extern "C"
