// mof_amg.hip -- aggregation multigrid V-cycle on gfx950 (inner-PCG preconditioner).
//
// Per batch of B systems (timesteps) the mesh-only hierarchy of
// mof_amg_host.cpp gets its per-timestep values:
//   k_galerkin_ns      A_{l+1} = Q^T A_l Q, one coarse block of 4 systems per
//                      thread, folded over the pre-built gather lists (no
//                      atomics), plus the 3x3 block-Jacobi inverse of each
//                      coarse node (k_galerkin_ent, k_galerkin3_big and
//                      k_galerkin_sys: the same sums by gather entry, by
//                      chunk and by system slab);
//   k_coarse_inverse   the coarsest operator (<= 128 dofs) inverted by the
//                      symmetric sweep operator in registers (fp64, one
//                      workgroup per system).
// Each PCG iteration applies one symmetric V(1,1)-cycle to the residual r
// (damped block Jacobi: w = 0.85 on level 0, w1 = 1.05 on the coarse levels):
//   level 0 pre-smooth x0 = w D^-1 r is fused into k_pcg_update / k_pcg_init;
//   per level l:  k_res0 / k_res3  r_l = b_l - A_l x_l, written in member
//                                  order of the next level's aggregates
//                 k_restrict / k_restrict0_sa  b_{l+1} = P^T r_l (tentative P:
//                                  contiguous members; smoothed P: list entries),
//                                  x_{l+1} = w1 D^-1 b_{l+1} (next pre-smooth)
//   levels with <= kSubNodes nodes and the coarsest solve y = A_c^-1 b run in
//   one launch (k_subcycle, one workgroup per system);
//   per level l:  k_prolong0 / k_prolong / k_prolong_sa  x_l += P y_{l+1}
//                 k_post0 / k_post3  y_l = x_l + w D^-1 (b_l - A_l x_l); at
//                                  level 0 y = z and the partial r.z of the PCG
// Every launch covers all B systems and skips retired systems. Level 0 sweeps
// a bf16 copy of the inner solver's SELL A (its diagonal blocks give the
// smoother's D), written by the assembly, in the PCG row-kernel layout (XCD-aware,
// batched loads); coarse levels keep fp32 3x3 blocks (12 floats, rows padded
// to 4) for the Galerkin products and int8 copies (9 codes + a bf16 scale,
// 12 B per block, st_a9) for the sweeps, vectors
// as 12-byte rows of three floats (kV3). All sums run in a fixed order: the cycle is
// deterministic and independent of B.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "mof_amg.h"
#include "mof_rowkern.h"

int mof_io_guard(const std::function<void()> &f);  // mof_abi.cpp: status + mof_last_error

namespace mof {

// tests only (mof_test_force_galerkin_ns): amg_setup_batch takes the
// per-position products where the by-entry ones would fit
std::atomic<int> g_force_galerkin_ns{0};
// launches so far (mof_test_galerkin_launches), in this order
enum GalKernel { kGal0Ns, kGal0Ent, kGalSys2F32, kGalSys2Bf16, kGalSys3, kGal3Ns, kGal3Ent, kGal3Big, kGalKernels };
std::atomic<int64_t> g_galerkin_launches[kGalKernels];
// launches so far of each V-cycle kernel instance (mof_test_vcycle_launches),
// in this order; kVcProlong3Sa: k_prolong_sa<3, 0, kNS3>, kVcProlong0SaX1 /
// X2: k_prolong_sa<2, 1 / 2, kNSP>; k_post0_ns's eight from kVcPost0:
// (XM - 1) * 4 + ZH * 2 + PK
enum VcKernel {
    kVcRes0, kVcRes0Pk, kVcRestrict2, kVcRestrict3, kVcRestrict0Sa2, kVcRestrict0Sa3, kVcRes3, kVcSubcycle,
    kVcProlong3, kVcProlong3Sa, kVcProlong0X1, kVcProlong0X2, kVcProlong0SaX1, kVcProlong0SaX2, kVcPost3,
    kVcBsweepH, kVcBsweepF, kVcPost0, kVcKernels = kVcPost0 + 8
};
std::atomic<int64_t> g_vcycle_launches[kVcKernels];

namespace {

constexpr int kB3 = 12;  // floats per coarse 3x3 block / per coarse D^-1

__device__ __forceinline__ bool retired(const int32_t *sysi, int32_t b) {
    return !sysi[b * kSysStride + SI_ACTIVE] || sysi[b * kSysStride + SI_CONV] >= 0;
}

// floats per node of a coarse level's vectors (b, x, r, y at levels >= 1):
// 12-byte rows at 4-byte alignment, system b's rows from b * n * kV3
constexpr int kV3 = 3;
struct F3 {
    float x, y, z;
};
static_assert(sizeof(F3) == kV3 * sizeof(float) && alignof(F3) == alignof(float), "a coarse row is three packed floats");

// per-node vector: BS = 2 -> float2 (stride 2), BS = 3 -> F3 (stride kV3, one 12-byte access)
template <int BS>
__device__ __forceinline__ void ldv(const float *v, int64_t node, float (&x)[BS]) {
    if constexpr (BS == 2) {
        const float2 t = reinterpret_cast<const float2 *>(v)[node];
        x[0] = t.x; x[1] = t.y;
    } else {
        const F3 t = reinterpret_cast<const F3 *>(v)[node];
        x[0] = t.x; x[1] = t.y; x[2] = t.z;
    }
}
// the restricted residual of level BSF: level 0 keeps it as a bf16 pair
// (4 B per vertex, written once by k_res0 and read once by the restriction)
template <int BSF>
__device__ __forceinline__ void ldr(const float *r, int64_t b, int64_t n, int64_t q, float (&x)[BSF]) {
    if constexpr (BSF == 2) {
        const uint32_t h = reinterpret_cast<const uint32_t *>(r)[b * n + q];
        x[0] = bf16_lo(h);
        x[1] = bf16_hi(h);
    } else {
        ldv<BSF>(r + b * n * kV3, q, x);
    }
}
template <int BS>
__device__ __forceinline__ void stv(float *v, int64_t node, const float (&x)[BS]) {
    if constexpr (BS == 2)
        reinterpret_cast<float2 *>(v)[node] = make_float2(x[0], x[1]);
    else
        reinterpret_cast<F3 *>(v)[node] = F3{x[0], x[1], x[2]};
}
// BS x BS block: BS = 2 -> 4 floats, BS = 3 -> 12 floats (rows padded to 4)
template <int BS>
__device__ __forceinline__ void ldm(const float *A, int64_t idx, float (&a)[BS][BS]) {
    if constexpr (BS == 2) {
        const float4 t = reinterpret_cast<const float4 *>(A)[idx];
        a[0][0] = t.x; a[0][1] = t.y; a[1][0] = t.z; a[1][1] = t.w;
    } else {
        const float4 *p = reinterpret_cast<const float4 *>(A) + 3 * idx;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float4 t = p[r];
            a[r][0] = t.x; a[r][1] = t.y; a[r][2] = t.z;
        }
    }
}
template <int BS>
constexpr int bstride() { return BS == 2 ? 4 : kB3; }
// A packed 3x3 block: 9 floats at 4-byte alignment (a level whose fp32
// operator only the next product reads keeps its diagonal and upper blocks
// this way, AmgDevLevel::packed)
constexpr int kB9 = 9;
struct F9 {
    float v[kB9];
};
__device__ __forceinline__ void ldm9(const float *A, int64_t idx, float (&a)[3][3]) {
    const F9 t = reinterpret_cast<const F9 *>(A)[idx];
#pragma unroll
    for (int k = 0; k < kB9; ++k) a[k / 3][k % 3] = t.v[k];
}
__device__ __forceinline__ void st9(float *A, int64_t idx, const float (&a)[3][3]) {
    F9 t;
#pragma unroll
    for (int k = 0; k < kB9; ++k) t.v[k] = a[k / 3][k % 3];
    reinterpret_cast<F9 *>(A)[idx] = t;
}

template <int BS>
__device__ __forceinline__ void matvec(const float (&a)[BS][BS], const float (&x)[BS], float (&y)[BS]) {
#pragma unroll
    for (int r = 0; r < BS; ++r) {
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < BS; ++c) s += a[r][c] * x[c];
        y[r] = s;
    }
}

// 3x3 inverse by cofactors (fp64 inside)
__device__ void inv3(const float (&a)[3][3], float (&o)[3][3]) {
    const double a00 = a[0][0], a01 = a[0][1], a02 = a[0][2], a10 = a[1][0], a11 = a[1][1],
                 a12 = a[1][2], a20 = a[2][0], a21 = a[2][1], a22 = a[2][2];
    const double c00 = a11 * a22 - a12 * a21, c01 = a12 * a20 - a10 * a22, c02 = a10 * a21 - a11 * a20;
    const double det = a00 * c00 + a01 * c01 + a02 * c02;
    const double id = det != 0.0 ? 1.0 / det : 0.0;
    o[0][0] = (float)(c00 * id);
    o[0][1] = (float)((a02 * a21 - a01 * a22) * id);
    o[0][2] = (float)((a01 * a12 - a02 * a11) * id);
    o[1][0] = (float)(c01 * id);
    o[1][1] = (float)((a00 * a22 - a02 * a20) * id);
    o[1][2] = (float)((a02 * a10 - a00 * a12) * id);
    o[2][0] = (float)(c02 * id);
    o[2][1] = (float)((a01 * a20 - a00 * a21) * id);
    o[2][2] = (float)((a00 * a11 - a01 * a10) * id);
}

// A product's diagonal block: its entries (r, c) and (c, r) are the same sum
// folded in two orders; the upper one is kept for both, so the coarse
// operator is symmetric to the bit inside its diagonal blocks too, as
// st_pair makes it across the twins (k_coarse_inverse's sweep takes row k
// for column k: on a matrix symmetric only to rounding its result is off by
// about cond x asymmetry)
__device__ __forceinline__ void sym3(float (&a)[3][3]) {
    a[1][0] = a[0][1];
    a[2][0] = a[0][2];
    a[2][1] = a[1][2];
}

__device__ __forceinline__ void st3(float *A, int64_t idx, const float (&a)[3][3]) {
    float4 *p = reinterpret_cast<float4 *>(A) + 3 * idx;
#pragma unroll
    for (int r = 0; r < 3; ++r) p[r] = make_float4(a[r][0], a[r][1], a[r][2], 0.f);
}

__device__ __forceinline__ void st_h9(uint4 *H, uint16_t *H22, int64_t q, const float (&c)[3][3]) {
    H[q] = make_uint4(bf16_bits(c[0][0]) | (bf16_bits(c[0][1]) << 16), bf16_bits(c[0][2]) | (bf16_bits(c[1][0]) << 16),
                      bf16_bits(c[1][1]) | (bf16_bits(c[1][2]) << 16), bf16_bits(c[2][0]) | (bf16_bits(c[2][1]) << 16));
    H22[q] = (uint16_t)bf16_bits(c[2][2]);
}

// The coarse levels' sweep copy of A (levels >= 1 except the coarsest):
// 12 B per 3x3 block, the 9 entries as offset-binary int8 (q + 128) with one
// bf16 scale per block (s = max |a| / 127): H viewed as uint2[] (entries
// 0..7), H22 as uint32_t[] (entry 8 | scale << 16). A block and its
// transposed twin have the same entries, so the same scale and the same
// codes: the preconditioner stays symmetric (round 2: 18 B bf16 entries
// before, level-1 k_res3 / k_post3 442 / 430 -> 360 / 337 us, C3 +1.6 %).
// uint32 words of Ah and uint16 words of Ah22 per block
constexpr size_t kAhWords = 2, kAh22Words = 2;

// the scale (bf16 bits) and the 9 codes of block c, row-major
__device__ __forceinline__ uint32_t quant_a9(const float (&c)[3][3], uint32_t (&u)[9]) {
    float m = 0.f;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) m = fmaxf(m, fabsf(c[r][k]));
    const uint32_t sb = bf16_bits(m / 127.f);
    const float sc = bf16_lo(sb);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float v = sc > 0.f ? rintf(c[r][k] / sc) : 0.f;
            u[3 * r + k] = (uint32_t)(fminf(fmaxf(v, -127.f), 127.f) + 128.f);
        }
    return sb;
}
// block q's words from its codes; TR: the codes of the transposed block
template <bool TR>
__device__ __forceinline__ void st_a9(uint4 *H, uint16_t *H22, int64_t q, const uint32_t (&u)[9], uint32_t sb) {
    auto e = [&](int k) { return TR ? u[3 * (k % 3) + k / 3] : u[k]; };
    reinterpret_cast<uint2 *>(H)[q] =
        make_uint2(e(0) | (e(1) << 8) | (e(2) << 16) | (e(3) << 24), e(4) | (e(5) << 8) | (e(6) << 16) | (e(7) << 24));
    reinterpret_cast<uint32_t *>(H22)[q] = e(8) | (sb << 16);
}
// A product's block C at position pos of system b and, for an upper block
// (tw >= 0: its lower twin's position, AmgLevel::twin), C^T at the twin: the
// products cover the diagonal and upper blocks only (round 6), and the
// coarse operator is symmetric to the bit. The sweep copy's scale and codes
// are formed once: the twin's words are the same nine bytes, transposed.
// pi >= 0: the level keeps its fp32 blocks packed ([c_npk] blocks of 9 floats
// per system, the diagonal and upper ones alone); C goes to packed index pi
// and the twin gets no fp32 block.
__device__ __forceinline__ void st_pair(float *__restrict__ Ac, uint4 *__restrict__ Ah, uint16_t *__restrict__ Ah22,
                                        int64_t b, int64_t c_sell_nb, int64_t pos, int32_t tw, int64_t c_npk,
                                        int32_t pi, const float (&C)[3][3]) {
    uint32_t u[9] = {}, sb = 0;
    if (Ah) sb = quant_a9(C, u);
    if (pi >= 0)
        st9(Ac, b * c_npk + pi, C);
    else
        st3(Ac, b * c_sell_nb + pos, C);
    if (Ah) st_a9<false>(Ah, Ah22, b * c_sell_nb + pos, u, sb);
    if (tw >= 0) {
        if (pi < 0) {
            float T[3][3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) T[r][c] = C[c][r];
            st3(Ac, b * c_sell_nb + tw, T);
        }
        if (Ah) st_a9<true>(Ah, Ah22, b * c_sell_nb + tw, u, sb);
    }
}

// What every Galerkin product A_c = P^T A_f P takes (gal_args): the coarse
// target, the fine level's gather lists and the batch
struct GalArgs {
    int64_t c_sell_nb;                       // the target's SELL positions per system
    int32_t nC;                              // and nodes
    int32_t B;                               // systems of the batch
    const int32_t *__restrict__ sell_row;    // the target's row of each position (>= nC: padding)
    const int32_t *__restrict__ diag;        // each row's diagonal position
    const uint8_t *__restrict__ dead;        // [nC][3] dofs without a prolongator column
    const int32_t *__restrict__ twin;        // each upper block's lower twin position, or -1
    const int32_t *__restrict__ pk;          // a packed target: each position's packed index, else null
    int64_t c_npk;                           // and its packed blocks per system
    const int32_t *__restrict__ gptr;        // [c_sell_nb + 1] each position's range of gather entries
    const int32_t *__restrict__ gent;        // triples {fine position or packed index (| kMirT), P block of i, of j}
    const float *__restrict__ Q;             // P blocks
    float *__restrict__ Ac;                  // [B][c_sell_nb][12], or packed [B][c_npk][9]
    uint4 *__restrict__ Dh;                  // [B][nC] block-Jacobi D^-1 (st_h9)
    uint16_t *__restrict__ Dh22;
    uint4 *__restrict__ Ah;                  // [B][c_sell_nb] sweep copy (st_a9), or null (the coarsest)
    uint16_t *__restrict__ Ah22;
};

// where a product reads its fine blocks: level 0's bf16 sweep copy (uint2) or
// fp32 A (float4) per block, a level >= 1's fp32 A (packed, 9 floats per
// block; the system slab: 12)
template <int BSF, bool H>
using GalSrc = std::conditional_t<BSF == 3, float, std::conditional_t<H, uint2, float4>>;

// a P block: BSF x 3 floats, row-major (q[k * 3 + c])
template <int BSF>
__device__ __forceinline__ void ld_p(const float *__restrict__ Q, int32_t blk, float (&q)[3 * BSF]) {
#pragma unroll
    for (int k = 0; k < 3 * BSF; ++k) q[k] = Q[(int64_t)blk * (3 * BSF) + k];
}

// The fine block of gather entry fp, at A[base + position * stride] (a
// system's operator: base = b * sell_nb, stride 1; a system slab: base =
// lane, stride kSlab). A level-0 entry with kMirT is the upper twin, read
// transposed; so is a packed coarse level's (PK: fp is the packed index of the
// block or of its upper twin, base = b * npk). fp < 0 is a decomposed part's ghost block: the identity for
// -1, zero otherwise. Position 0 is read for it and dropped: a branch around
// the loads costs k_galerkin3_big and k_galerkin_ns<3> registers across an
// occupancy step (81 and 138 VGPRs; profiles/galerkin_refactor/).
template <int BSF, bool PK = false, typename T>
__device__ __forceinline__ void ld_fine(const T *__restrict__ A, int64_t base, int64_t stride, int32_t fp,
                                        float (&a)[BSF][BSF]) {
    if constexpr (BSF == 3 && PK) {
        ldm9(A, base + (fp < 0 ? 0 : fp & kMirPos) * stride, a);
        const bool tr = fp >= 0 && (fp & kMirT);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = r + 1; c < 3; ++c) {
                const float up = a[r][c], lo = a[c][r];
                a[r][c] = tr ? lo : up;
                a[c][r] = tr ? up : lo;
            }
    } else if constexpr (BSF == 3) {
        ldm<3>(A, base + max(fp, 0) * stride, a);
    } else {
        const int64_t q = base + (fp < 0 ? 0 : fp & kMirPos) * stride;
        if constexpr (std::is_same_v<T, uint2>) {
            h0_dec(h0_ld(A, q), a[0][0], a[0][1], a[1][0], a[1][1]);
        } else {
            const float4 v = A[q];
            a[0][0] = v.x; a[0][1] = v.y; a[1][0] = v.z; a[1][1] = v.w;
        }
        if (fp >= 0 && (fp & kMirT)) {
            const float t01 = a[0][1];
            a[0][1] = a[1][0];
            a[1][0] = t01;
        }
    }
    if (fp < 0) {
#pragma unroll
        for (int r = 0; r < BSF; ++r)
#pragma unroll
            for (int c = 0; c < BSF; ++c) a[r][c] = (fp == -1 && r == c) ? 1.f : 0.f;
    }
}

// One term out = Q_i^T (A Q_j) of a product. No fp contraction, and the
// pragma is lexical -- it has to stand here, a caller's does not reach an
// inlined body: the kernels with several systems per thread unroll over them,
// and every system slot must round alike (a system's bits must not depend on
// its slot, i.e. on the batch split). k_galerkin_sys alone keeps a contracted
// form of its own.
template <int BSF>
__device__ __forceinline__ void gal_term(const float (&a)[BSF][BSF], const float (&qi)[3 * BSF],
                                         const float (&qj)[3 * BSF], float (&out)[3][3]) {
#pragma clang fp contract(off)
    float T[BSF][3];  // A Q_j
#pragma unroll
    for (int r = 0; r < BSF; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float sum = 0.f;
#pragma unroll
            for (int k = 0; k < BSF; ++k) sum += a[r][k] * qj[k * 3 + c];
            T[r][c] = sum;
        }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float sum = 0.f;
#pragma unroll
            for (int k = 0; k < BSF; ++k) sum += qi[k * 3 + r] * T[k][c];
            out[r][c] = sum;
        }
}

// The folded block Cm of position pos (row I) of system b goes to the target:
// a diagonal block (diag) gets 1 on its dead dofs, is made symmetric to the
// bit (sym3) and leaves its inverse as the level's D^-1; then the block and
// its lower twin (st_pair), whose position is returned (-1: none)
__device__ __forceinline__ int32_t gal_finish(const GalArgs &g, int32_t b, int64_t pos, int32_t I, bool diag,
                                              float (&Cm)[3][3]) {
    // read ahead of the stores: __restrict__ on a member promises the
    // compiler nothing, so it would not move this load above them itself
    const int32_t tw = g.twin[pos];
    const int32_t pi = g.pk ? g.pk[pos] : -1;
    if (diag) {
#pragma unroll
        for (int d = 0; d < 3; ++d)
            if (g.dead[3 * (int64_t)I + d]) Cm[d][d] += 1.f;
        sym3(Cm);
        float D[3][3];
        inv3(Cm, D);
        st_h9(g.Dh, g.Dh22, (int64_t)b * g.nC + I, D);
    }
    st_pair(g.Ac, g.Ah, g.Ah22, b, g.c_sell_nb, pos, tw, g.c_npk, pi, Cm);
    return tw;
}

// ---- per-timestep setup --------------------------------------------------

// A32 -> the level-0 sweep copy (h0_st)
__global__ __launch_bounds__(kWG) void k_to_h0(int64_t n, const float4 *__restrict__ A, uint2 *__restrict__ H) {
    const int64_t q = (int64_t)blockIdx.x * kWG + threadIdx.x;
    if (q >= n) return;
    const float4 v = A[q];
    h0_st(H, q, v.x, v.y, v.z, v.w);
}

// Plain-read meshes: the assembly forms a lower block (i, j), j < i, on its
// own, and now and then it rounds to another bf16 than its upper twin (one
// bf16 ulp on a few blocks of a 3,000-vertex hull); the sweeps read every
// block at its own position, so the smoother's operator -- and the V-cycle --
// would be symmetric only to that rounding. Each lower block of the sweep copy
// becomes its upper twin transposed, through the mirror table the level-0
// gather lists already read by (symmetric-read meshes read that way anyway).
// Grid (position blocks, systems).
__global__ __launch_bounds__(kWG) void k_h0_twins(int64_t nb, const int32_t *__restrict__ mir,
                                                  uint2 *__restrict__ H) {
    const int64_t p = (int64_t)blockIdx.x * kWG + threadIdx.x;
    if (p >= nb) return;
    const int32_t mr = mir[p];
    if (mr < 0 || !(mr & kMirT)) return;  // padding, the diagonal and upper blocks
    const int64_t o = (int64_t)blockIdx.y * nb;
    H[o + p] = h0_tr(h0_ld(H, o + (mr & kMirPos)));
}

// The Galerkin product per coarse position, NS systems per thread: the
// gather entry (fine position, P blocks of i and j) and both P blocks are
// loaded once and applied to the fine blocks of every system, folded per
// system in list order. Level 0 (BSF = 2; 7.5x the entries with a smoothed
// prolongator) reads the smoother's bf16 copy (Afh) or, Afh null, the fp32 A
// (Af); levels >= 1 (BSF = 3) the packed fp32 3x3 blocks of Af (f_sell_nb:
// the source's blocks per system, packed ones there).
// Level 0, systems per thread: C3 (512 systems) 6.08 ms per launch at 4, 8.06
// at 8, 14.7 at 16 (the per-system fine-block gathers, not the shared gather
// lists, bound it; more systems per thread only lower the occupancy); one
// system per thread (k_galerkin<2>): 9.02 ms. One gather entry per load
// batch (92 VGPRs, 5 waves per SIMD) instead of 2 (140, 3 waves): 6.37 ->
// 5.92 ms per launch (round 3).
// The system quads of a coarse tile run back to back on an XCD in groups of
// kGrpGal (8 quads = 32 systems); 2 quads per group (fewer systems' fine
// blocks in flight per tile) measured slower: C3 3424-3428 vs 3443-3446
// timesteps/s (round 3, profiles/r03_ab/gal2_*).
// Level 1 at C3 (512 systems): 1217 us per launch with one system per thread
// (round 2's k_galerkin<3>, 4 entries per load batch), 935 with 2, 851 with 4
// (132 VGPRs, 3 waves); C3 +0.5 %, R3 (denser level 1) within noise (round 3).
constexpr int kGalNS = 4;
constexpr int kGal3NS = 4;
template <int BSF, int NS>
__global__ __launch_bounds__(kWG) void k_galerkin_ns(GalArgs g, const float *__restrict__ Af, int64_t f_sell_nb,
                                                     const uint2 *__restrict__ Afh) {
    // no fp contraction: every system slot of the unrolled loops rounds alike
    // (gal_term)
#pragma clang fp contract(off)
    int32_t tile, bq;
    if (!xcd_map((int32_t)((g.c_sell_nb + kWG - 1) / kWG), (g.B + NS - 1) / NS, tile, bq, kGrpGal)) return;
    const int64_t pos = (int64_t)tile * kWG + threadIdx.x;
    if (pos >= g.c_sell_nb) return;
    const int32_t I = g.sell_row[pos];
    if (I >= g.nC) return;
    const int32_t b0 = bq * NS;
    float Cm[NS][3][3] = {};
    const int32_t e0 = g.gptr[pos], e1 = g.gptr[pos + 1];
    const bool diag = pos == g.diag[I];
    if (e0 == e1 && !diag) return;  // a lower block (its upper twin writes it, st_pair) or padding
    for (int64_t e = e0; e < e1; ++e) {
        const int32_t fp = g.gent[3 * e], ii = g.gent[3 * e + 1], jj = g.gent[3 * e + 2];
        float qi[3 * BSF], qj[3 * BSF], a[NS][BSF][BSF];
        ld_p<BSF>(g.Q, ii, qi);
        ld_p<BSF>(g.Q, jj, qj);
#pragma unroll
        for (int t = 0; t < NS; ++t) {
            const int64_t base = (int64_t)min(b0 + t, g.B - 1) * f_sell_nb;
            if constexpr (BSF == 3)
                ld_fine<3, true>(Af, base, 1, fp, a[t]);
            else if (Afh)
                ld_fine<2>(Afh, base, 1, fp, a[t]);
            else
                ld_fine<2>(reinterpret_cast<const float4 *>(Af), base, 1, fp, a[t]);
        }
#pragma unroll
        for (int t = 0; t < NS; ++t) {
            float T[3][3];
            gal_term<BSF>(a[t], qi, qj, T);
#pragma unroll
            for (int k = 0; k < 9; ++k) Cm[t][k / 3][k % 3] += T[k / 3][k % 3];
        }
    }
#pragma unroll
    for (int t = 0; t < NS; ++t)
        if (b0 + t < g.B) gal_finish(g, b0 + t, pos, I, diag, Cm[t]);
}

// The Galerkin product by gather entry (tentative prolongator; BSF = 2:
// level 0 from the bf16 sweep copy, BSF = 3: levels >= 1): a workgroup takes
// a range of coarse positions with at most kWG gather entries in total
// (ggrp, built on the host), one entry per thread for kGalENS systems -- the
// entry and its two Q rows loaded once, every fine block of the systems
// gathered at once -- stages each term Q_i^T A_ij Q_j in LDS, then one thread
// per (coarse position, system) sums its terms in list order. The same terms
// in the same order as k_galerkin_ns (bit-identical), with two dependent
// loads per thread instead of two per entry of a position.
// Systems per workgroup (level 0 at C3, 512 systems, one box, round 3: 4 ->
// 5288 us per launch, 4 with the first task's position data loaded beside the
// entry 4978, 2 4670-4735, 1 5613, 8 6271; the old per-position kernel 5952,
// its reads 32.5 -> 4.35 GB per launch). Spreading the sums over the 9 block
// entries (every thread busy, a second barrier) took 9376 us.
constexpr int kGalENS = 2;
template <int BSF>
__global__ __launch_bounds__(kWG) void k_galerkin_ent(GalArgs g, int32_t ngrp, const int32_t *__restrict__ ggrp,
                                                      const GalSrc<BSF, true> *__restrict__ Af, int64_t f_sell_nb) {
    // no fp contraction: every system slot rounds alike, and as k_galerkin_ns
#pragma clang fp contract(off)
    __shared__ float con[kGalENS][9][kWG];
    int32_t grp, bq;
    const int32_t nq = (g.B + kGalENS - 1) / kGalENS;
    if (!xcd_map(ngrp, nq, grp, bq, kGrpGal)) return;
    const int32_t b0 = bq * kGalENS;
    const int32_t p0 = ggrp[2 * grp], p1 = ggrp[2 * grp + 1];
    const int32_t e0 = g.gptr[p0], e1 = g.gptr[p1];
    const int64_t e = e0 + (int32_t)threadIdx.x;
    const int32_t np = p1 - p0;
    // the first task's position data, loaded beside the entry's (the tasks
    // run after the barrier; most groups have one task per thread or fewer)
    int32_t tI = g.nC, tq0 = 0, tq1 = 0, tdg = -1;
    if ((int32_t)threadIdx.x < np * kGalENS) {
        const int32_t pos = p0 + (int32_t)threadIdx.x / kGalENS;
        tI = g.sell_row[pos];
        tq0 = g.gptr[pos];
        tq1 = g.gptr[pos + 1];
        if (tI < g.nC) tdg = g.diag[tI];
    }
    if (e < e1) {
        const int32_t fp = g.gent[3 * e], ii = g.gent[3 * e + 1], jj = g.gent[3 * e + 2];
        float qi[3 * BSF], qj[3 * BSF], a[kGalENS][BSF][BSF];
        ld_p<BSF>(g.Q, ii, qi);
        ld_p<BSF>(g.Q, jj, qj);
#pragma unroll
        for (int t = 0; t < kGalENS; ++t)
            ld_fine<BSF, BSF == 3>(Af, (int64_t)min(b0 + t, g.B - 1) * f_sell_nb, 1, fp, a[t]);
#pragma unroll
        for (int t = 0; t < kGalENS; ++t) {
            float T[3][3];
            gal_term<BSF>(a[t], qi, qj, T);
#pragma unroll
            for (int k = 0; k < 9; ++k) con[t][k][threadIdx.x] = T[k / 3][k % 3];
        }
    }
    __syncthreads();
    for (int32_t task = threadIdx.x; task < np * kGalENS; task += kWG) {
        const int32_t pos = p0 + task / kGalENS, t = task % kGalENS, b = b0 + t;
        const bool first = task == (int32_t)threadIdx.x;
        const int32_t I = first ? tI : g.sell_row[pos];
        if (I >= g.nC || b >= g.B) continue;
        float Cm[3][3] = {};
        const int32_t q0 = first ? tq0 : g.gptr[pos], q1 = first ? tq1 : g.gptr[pos + 1];
        const bool diag = pos == (first ? tdg : g.diag[I]);
        if (q0 == q1 && !diag) continue;  // a lower block (its upper twin writes it, st_pair) or padding
        for (int32_t q = q0; q < q1; ++q)
#pragma unroll
            for (int k = 0; k < 9; ++k) Cm[k / 3][k % 3] += con[t][k][q - e0];
        gal_finish(g, b, pos, I, diag, Cm);
    }
}

// Level 0 with the smoothed prolongator, by system slab: the gather lists
// are wave-uniform and the 64 lanes of a wave are 64 systems of one coarse
// position. The per-position kernel above (one position of 4 systems per
// thread) gathers a 16-byte fine block per system from 4 lines 20 MB apart,
// 64 positions' scattered blocks per load: S1 122 ms per 1536-system batch,
// L2-line bound. Here a slab of kSlab systems' fp32 level-0 blocks is first
// transposed to [fine position][system] (k_a_slab), so one fine block of
// the whole wave is one 1 KB read, and the entry and its two P blocks are
// scalar loads shared by the 64 systems. Every system runs the same
// instructions in its own lane: the bits do not depend on the batch split.
// S1, per 1536-system batch: level 0 122.5 -> 12.3 (k_a_slab) + 40.6 ms,
// S1 1014 -> 1064 timesteps/s; with level 1 -> 2 from the slab copy level 0
// writes beside its A (k_galerkin_sys<3>, instead of the chunked / by-entry
// products, 55 ms): level 0 46.5 + level 1 29.6 ms, R3 906 -> 918
// (profiles/r05_ab/gal_slab/).
constexpr int kSlab = 64;
constexpr int kSlabPos = 64;  // fine positions per k_a_slab workgroup
// T = float4: the fp32 A; T = uint2 (round 6, regular closed meshes -- F3):
// the level-0 sweep copy's bf16 blocks, as the tentative product by entry
// reads them, half the bytes for the transpose and for the product's ~7
// reads of each block: F3 +4 %; on the open patch S1 the bf16 coarse
// operator cost 14 of 3,072 solves a recovery (profiles/r06/slab_bf16/)
template <typename T>
__global__ __launch_bounds__(kWG) void k_a_slab(int64_t f_sell_nb, int32_t b0, int32_t nb,
                                                const T *__restrict__ Af, T *__restrict__ AI) {
    __shared__ T t[kSlabPos][kSlab + 1];
    const int64_t q0 = (int64_t)blockIdx.x * kSlabPos;
    const int32_t lane = (int32_t)threadIdx.x & 63, w = (int32_t)threadIdx.x >> 6;
    // read: a wave takes one system's 64 consecutive blocks
    for (int32_t s = w; s < kSlab; s += kWG / 64) {
        const int64_t q = q0 + lane;
        T v = {};
        if (s < nb && q < f_sell_nb) v = Af[(int64_t)(b0 + s) * f_sell_nb + q];
        t[lane][s] = v;
    }
    __syncthreads();
    // write: a wave takes one fine position's 64 systems
    for (int32_t k = w; k < kSlabPos; k += kWG / 64) {
        const int64_t q = q0 + k;
        if (q < f_sell_nb) AI[q * kSlab + lane] = t[k][lane];
    }
}

constexpr int kGalSysPos = kWG / 64;  // coarse positions per workgroup, one per wave
// Level l's Galerkin product over the system slab of b0: BSF = 2 reads the
// level-0 slab (k_a_slab, float4 blocks or, H, bf16 as uint2; mirror
// entries), BSF = 3 the slab a level l >= 1 product wrote beside its level's
// A (CS: [sell_nb][kSlab][3] float4, the stored rows). Gather entries per
// load batch: 4 at level 0, 2 on the coarse levels (their P blocks are 18
// scalar registers each).
template <int BSF, bool H = false>
__global__ __launch_bounds__(kWG) void k_galerkin_sys(GalArgs g, const GalSrc<BSF, H> *__restrict__ FS, int32_t b0,
                                                      float4 *__restrict__ CS) {
    constexpr int U = BSF == 2 ? 4 : 2;
    int32_t tile, bq;
    if (!xcd_map((int32_t)((g.c_sell_nb + kGalSysPos - 1) / kGalSysPos), 1, tile, bq, 1)) return;
    const int64_t pos = (int64_t)tile * kGalSysPos + __builtin_amdgcn_readfirstlane((int32_t)threadIdx.x >> 6);
    if (pos >= g.c_sell_nb) return;
    const int32_t I = g.sell_row[pos];
    if (I >= g.nC) return;
    const int32_t lane = (int32_t)threadIdx.x & 63;
    float Cm[3][3] = {};
    const int32_t e0 = g.gptr[pos], e1 = g.gptr[pos + 1];
    const bool diag = pos == g.diag[I];
    if (e0 == e1 && !diag) return;  // a lower block (its upper twin writes it, st_pair) or padding
    // U entries per load batch (the entries' scalar loads, then their fine
    // blocks, in flight together); a batch's tail entries past e1 are
    // clamped to the last one and skipped (wave-uniform)
    for (int32_t t0 = e0; t0 < e1; t0 += U) {
        int32_t fp[U];
        float qi[U][3 * BSF], qj[U][3 * BSF], a[U][BSF][BSF];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t e = min(t0 + u, e1 - 1);
            fp[u] = g.gent[3 * e];
            ld_p<BSF>(g.Q, g.gent[3 * e + 1], qi[u]);
            ld_p<BSF>(g.Q, g.gent[3 * e + 2], qj[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) ld_fine<BSF>(FS, lane, kSlab, fp[u], a[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (t0 + u >= e1) break;
            // gal_term's sums written out where fp contraction is on, as this
            // kernel has always had it: each lane is one system and runs the
            // same instructions, so contraction is uniform over the batch,
            // and the contracted bits are the results on every smoothed mesh
            float T[BSF][3];  // A Q_j
#pragma unroll
            for (int r = 0; r < BSF; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float sum = 0.f;
#pragma unroll
                    for (int k = 0; k < BSF; ++k) sum += a[u][r][k] * qj[u][k * 3 + c];
                    T[r][c] = sum;
                }
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float sum = 0.f;
#pragma unroll
                    for (int k = 0; k < BSF; ++k) sum += qi[u][k * 3 + r] * T[k][c];
                    Cm[r][c] += sum;
                }
        }
    }
    const int32_t b = b0 + lane;
    if (b >= g.B) return;
    const int32_t tw = gal_finish(g, b, pos, I, diag, Cm);
    if (CS) {  // the next product's slab: the block as stored, and its lower twin
        float4 *p = CS + (pos * kSlab + lane) * 3;
#pragma unroll
        for (int r = 0; r < 3; ++r) p[r] = make_float4(Cm[r][0], Cm[r][1], Cm[r][2], 0.f);
        if (tw >= 0) {
            float4 *q = CS + ((int64_t)tw * kSlab + lane) * 3;
#pragma unroll
            for (int r = 0; r < 3; ++r) q[r] = make_float4(Cm[0][r], Cm[1][r], Cm[2][r], 0.f);
        }
    }
}

// Levels >= 1, the coarse positions with more than kGalBig gather entries
// (a smoothed level's: S1 level 1 mean 105, p90 247, max 789 entries; 85 %
// of its terms sit in positions past 128, where one thread per position
// leaves a SELL wave 0.24 busy): one workgroup per (position, NSB systems)
// walks the list in chunks of kWG entries -- every thread one entry's term
// for the NSB systems, staged in LDS -- and 9 NSB threads, one per (system,
// block entry), fold each chunk in list order. Each block entry is a sum of
// its own terms, so the bits are k_galerkin_ns's. S1 (1536 systems), level
// 1 -> 2: 42.8 ms per launch per position -> 20.9 by chunk (and 4.6 ms for
// the positions below the bound by entry); 4 systems per workgroup 23.1, 8
// 25.8, bound 64 entries 24.9 + 3.3 (profiles/r05_ab/gal_slab/).
constexpr int kGalBig = 128;
constexpr int kGalBigNS = 2;
template <int NSB>
__global__ __launch_bounds__(kWG) void k_galerkin3_big(GalArgs g, int32_t nbig, const int32_t *__restrict__ gbig,
                                                       const float *__restrict__ Af, int64_t f_sell_nb) {
#pragma clang fp contract(off)
    // rows padded by one word: the 9 NSB summing lanes read one column at
    // a time, kWG + 1 words apart -- distinct banks
    __shared__ float con[NSB][9][kWG + 1];
    __shared__ float fin[NSB][9];
    int32_t grp, bq;
    if (!xcd_map(nbig, (g.B + NSB - 1) / NSB, grp, bq, kGrpGal)) return;
    const int32_t b0 = bq * NSB;
    const int32_t pos = gbig[grp];
    const int32_t e0 = g.gptr[pos], e1 = g.gptr[pos + 1];
    const int32_t sk = (int32_t)threadIdx.x;  // summing lane: system sk / 9, block entry sk % 9
    float acc = 0.f;
    for (int32_t c0 = e0; c0 < e1; c0 += kWG) {
        const int64_t e = c0 + (int32_t)threadIdx.x;
        if (e < e1) {
            const int32_t fp = g.gent[3 * e], ii = g.gent[3 * e + 1], jj = g.gent[3 * e + 2];
            float qi[9], qj[9], a[NSB][3][3];
            ld_p<3>(g.Q, ii, qi);
            ld_p<3>(g.Q, jj, qj);
#pragma unroll
            for (int t = 0; t < NSB; ++t)
                ld_fine<3, true>(Af, (int64_t)min(b0 + t, g.B - 1) * f_sell_nb, 1, fp, a[t]);
#pragma unroll
            for (int t = 0; t < NSB; ++t) {
                float T[3][3];
                gal_term<3>(a[t], qi, qj, T);
#pragma unroll
                for (int k = 0; k < 9; ++k) con[t][k][threadIdx.x] = T[k / 3][k % 3];
            }
        }
        __syncthreads();
        if (sk < 9 * NSB) {
            const float *row = con[sk / 9][sk % 9];
            const int32_t m = min(kWG, e1 - c0);
            int32_t q = 0;
            for (; q + 8 <= m; q += 8) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = row[q + u];
#pragma unroll
                for (int u = 0; u < 8; ++u) acc += v[u];
            }
            for (; q < m; ++q) acc += row[q];
        }
        __syncthreads();
    }
    if (sk < 9 * NSB) fin[sk / 9][sk % 9] = acc;
    __syncthreads();
    if ((int32_t)threadIdx.x >= NSB) return;
    const int32_t t = (int32_t)threadIdx.x, b = b0 + t;
    if (b >= g.B) return;
    const int32_t I = g.sell_row[pos];
    float Cm[3][3];
#pragma unroll
    for (int k = 0; k < 9; ++k) Cm[k / 3][k % 3] = fin[t][k];
    gal_finish(g, b, pos, I, pos == g.diag[I], Cm);
}


constexpr int kMaxCoarse = 128;
constexpr int kInvWG = 1024;
constexpr int kSweepRows = kMaxCoarse * kMaxCoarse / kInvWG;  // 16 matrix rows per thread

// Inverse of the coarsest operator (nc = 3 n <= 128 dofs) of system b by the
// symmetric sweep operator: sweeping pivot k maps
//   a_kk -> -1/a_kk, a_ik -> a_ik/a_kk, a_kj -> a_kj/a_kk,
//   a_ij -> a_ij - a_ik a_kj / a_kk,
// and after all pivots the matrix holds -A^-1. Symmetry gives column k =
// row k, so a step broadcasts one row through LDS. Thread t owns column
// t % 128 of rows (t / 128) * 16 + [0, 16) in fp64 registers.
__global__ __launch_bounds__(kInvWG) void k_coarse_inverse(int32_t n, const int32_t *__restrict__ sell_off,
                                                        const int32_t *__restrict__ sell_col,
                                                        const float *__restrict__ Ac, int64_t sell_nb,
                                                        float *__restrict__ cinv) {
    __shared__ float M[kMaxCoarse][kMaxCoarse + 1];
    __shared__ double rowk[kMaxCoarse];
    const int32_t b = blockIdx.x;
    const int32_t nc = 3 * n;
    for (int32_t q = threadIdx.x; q < kMaxCoarse * kMaxCoarse; q += kInvWG)
        M[q / kMaxCoarse][q % kMaxCoarse] = 0.f;
    __syncthreads();
    const float *A = Ac + (int64_t)b * sell_nb * kB3;
    // one thread per node row: no two threads write the same row
    for (int32_t I = threadIdx.x; I < n; I += kInvWG) {
        const int32_t s = I >> 6, l = I & 63;
        const int32_t o = sell_off[s], w = (sell_off[s + 1] - o) >> 6;
        for (int32_t t = 0; t < w; ++t) {
            const int64_t pos = (int64_t)o + t * kSlice + l;
            const int32_t J = sell_col[pos];
            float a[3][3];
            ldm<3>(A, pos, a);
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) M[3 * I + r][3 * J + c] += a[r][c];
        }
    }
    __syncthreads();
    const int32_t c = threadIdx.x & (kMaxCoarse - 1);
    const int32_t h = threadIdx.x / kMaxCoarse;
    double a[kSweepRows];
#pragma unroll
    for (int mm = 0; mm < kSweepRows; ++mm) a[mm] = (double)M[h * kSweepRows + mm][c];
    if (threadIdx.x < kMaxCoarse) rowk[threadIdx.x] = 0.0;
    __syncthreads();
    for (int32_t k = 0; k < nc; ++k) {
        if (h == k / kSweepRows && c < nc) {
            const int32_t mk = k % kSweepRows;
            double v = 0.0;
#pragma unroll
            for (int mm = 0; mm < kSweepRows; ++mm) v = (mm == mk) ? a[mm] : v;
            rowk[c] = v;
        }
        __syncthreads();
        double piv = rowk[k];
        piv = piv != 0.0 ? piv : 1.0;
        const double ip = 1.0 / piv;
        const double akc = rowk[c] * ip;
        const bool ck = c == k;
        const double rowfix = ck ? -ip : akc;  // the new row k
        // branch-free (every LDS read unconditional, so they pipeline):
        // column k scales by 1/piv, row k is replaced, the rest updates
        const double f = ck ? 0.0 : akc, sc = ck ? ip : 1.0;
#pragma unroll
        for (int mm = 0; mm < kSweepRows; ++mm) {
            const int32_t r = h * kSweepRows + mm;
            const double v = fma(-rowk[r], f, a[mm]) * sc;
            a[mm] = (r == k) ? rowfix : v;
        }
        __syncthreads();
    }
    float *out = cinv + (int64_t)b * nc * nc;
    if (c < nc) {
#pragma unroll
        for (int mm = 0; mm < kSweepRows; ++mm) {
            const int32_t r = h * kSweepRows + mm;
            if (r < nc) out[(int64_t)r * nc + c] = (float)(-a[mm]);
        }
    }
}

// ---- V-cycle ---------------------------------------------------------------

// Device view of one level (pointers to system 0; system b adds its stride).
struct Lvl {
    int32_t n;
    int64_t sell_nb;
    const int32_t *sell_off, *sell_col;  // level >= 1
    const float *A;                      // level >= 1: [B][sell_nb][12]
    const uint4 *Dh;                     // level >= 1: 3x3 D^-1, bf16 entries 0..7 [B][n]
    const uint16_t *Dh22;                // and entry (2,2)
    const uint4 *Ah;                     // bf16 A for the sweeps: [B][sell_nb] entries 0..7, or null
    const uint16_t *Ah22;                // [B][sell_nb] entry (2,2)
    float *b, *x, *r, *y;                // [B][n][3] (level 0: x [B][n][2], r bf16 [B][n][2])
    const int32_t *agg, *mptr, *apos;    // transition to level + 1
    const int32_t *mlist;                // aggregate members (level 0: r1 gathered in member order)
    const float *Q, *Qm;                 // tentative rows (node order / member order), or P blocks
    const int32_t *pptr, *pcol;          // smoothed P: row blocks of each fine node
    const int32_t *rptr, *rent;          // smoothed P: {fine node, P block} per coarse node
    const int32_t *rperm;                // smoothed P: each restriction group's entries by fine node
    SysMap sm;                           // the systems the cycle's launches cover (amg_vcycle)
};

// 3x3 bf16 block stored as 8 entries in 16 B + entry (2,2) in 2 B
__device__ __forceinline__ void ld_h9(const uint4 *H, const uint16_t *H22, int64_t q, float (&a)[3][3]) {
    const uint4 h = H[q];
    a[0][0] = bf16_lo(h.x);
    a[0][1] = bf16_hi(h.x);
    a[0][2] = bf16_lo(h.y);
    a[1][0] = bf16_hi(h.y);
    a[1][1] = bf16_lo(h.z);
    a[1][2] = bf16_hi(h.z);
    a[2][0] = bf16_lo(h.w);
    a[2][1] = bf16_hi(h.w);
    a[2][2] = bf16_lo((uint32_t)H22[q]);
}
// block q of a coarse level's sweep copy (st_a9)
__device__ __forceinline__ void ld_a9(const uint4 *H, const uint16_t *H22, int64_t q, float (&a)[3][3]) {
    {
        const uint2 h = reinterpret_cast<const uint2 *>(H)[q];
        const uint32_t t = reinterpret_cast<const uint32_t *>(H22)[q];
        const float sc = bf16_hi(t);
        const uint32_t w[3] = {h.x, h.y, t};
#pragma unroll
        for (int e = 0; e < 9; ++e)
            a[e / 3][e % 3] = (float)((int32_t)((w[e >> 2] >> (8 * (e & 3))) & 0xffu) - 128) * sc;
    }
}
// the smoother's 3x3 D^-1 of node i of system b
__device__ __forceinline__ void ld_dh(const Lvl &L, int32_t b, int32_t i, float (&d)[3][3]) {
    ld_h9(L.Dh, L.Dh22, (int64_t)b * L.n + i, d);
}

// (A x)_i of a coarse level, slots U at a time with all loads of a chunk
// issued first (as spmv_row).
__device__ __forceinline__ void spmv_row3(const Lvl &L, int32_t b, int32_t i, const float *__restrict__ xb,
                                          float (&acc)[3]) {
    constexpr int U = 4;
    const float *Ab = L.A + (int64_t)b * L.sell_nb * kB3;
    const int64_t hb = (int64_t)b * L.sell_nb;  // system b's first block of the sweep copy (ld_a9 index)
    const bool half = L.Ah != nullptr;
    const int32_t s = i >> 6, l = i & 63;
    const int32_t o = L.sell_off[s], w = (L.sell_off[s + 1] - o) >> 6;
    acc[0] = acc[1] = acc[2] = 0.f;
    for (int32_t t0 = 0; t0 < w; t0 += U) {
        int32_t j[U];
        float a[U][3][3], xj[U][3];
#pragma unroll
        for (int u = 0; u < U; ++u) j[u] = L.sell_col[(int64_t)o + min(t0 + u, w - 1) * kSlice + l];
        if (half) {
#pragma unroll
            for (int u = 0; u < U; ++u) ld_a9(L.Ah, L.Ah22, hb + o + min(t0 + u, w - 1) * kSlice + l, a[u]);
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) ldm<3>(Ab, (int64_t)o + min(t0 + u, w - 1) * kSlice + l, a[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) ldv<3>(xb, j[u], xj[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool on = t0 + u < w;
            float ax[3];
            matvec<3>(a[u], xj[u], ax);
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += on ? ax[c] : 0.f;
        }
    }
}

// coarse level: r = b - A x at the member position of node i
__device__ __forceinline__ void res3_node(const Lvl &L, int32_t b, int32_t i) {
    const int64_t vo = (int64_t)b * L.n * kV3;
    float ax[3], bi[3];
    spmv_row3(L, b, i, L.x + vo, ax);
    ldv<3>(L.b + vo, i, bi);
    const float ri[3] = {bi[0] - ax[0], bi[1] - ax[1], bi[2] - ax[2]};
    stv<3>(L.r + vo, L.apos[i], ri);
}

// The NS systems a workgroup or thread of a multi-system kernel carries:
// slot t is logical system l0 + t of the launch (SysMap). b(t) is its system
// (sm_b clamps a slot past the launch's last system to that one, so loads
// stay in bounds); act(t): the slot is inside the launch and its system not
// retired -- only those slots store.
template <int NS>
struct SysGroup {
    const SysMap &sm;
    const int32_t *sysi;
    int32_t l0;
    __device__ __forceinline__ int32_t b(int t) const { return sm_b(sm, l0 + t); }
    __device__ __forceinline__ bool act(int t) const { return l0 + t < sm.n && !retired(sysi, b(t)); }
    __device__ __forceinline__ bool any() const {
        bool a = false;
#pragma unroll
        for (int t = 0; t < NS; ++t) a |= act(t);
        return a;
    }
};

// A restriction's finish: b_C[I] = acc; with smooth also the coarse level's
// pre-smoothed iterate x_C[I] = w D_C^-1 b_C[I]. The same bits from every
// caller, with fp contraction on or off: matvec contracts as it is defined
// and the scaling is a single multiply.
__device__ __forceinline__ void coarse_store(const Lvl &C, int32_t b, int32_t I, const float (&acc)[3], bool smooth,
                                             float omega) {
    const int64_t vo = (int64_t)b * C.n * kV3;
    stv<3>(C.b + vo, I, acc);
    if (smooth) {
        float d[3][3], x[3];
        ld_dh(C, b, I, d);
        matvec<3>(d, acc, x);
#pragma unroll
        for (int c = 0; c < 3; ++c) x[c] *= omega;
        stv<3>(C.x + vo, I, x);
    }
}

// The iterate a prolongation corrects, node i of system b. Level 0 (BSF = 2)
// reads the x0 word of F.x and writes the corrected pair back in that format
// in place (XM = 1) or as float2 into F.y, full precision for the
// post-smoothing (XM = 2, see AmgDevice::xm); a coarse level (BSF = 3) keeps
// 12-byte rows in F.x.
template <int BSF>
__device__ __forceinline__ void ld_xf(const Lvl &F, int32_t b, int32_t i, float (&x)[BSF]) {
    if constexpr (BSF == 2) {
        const float2 t = ld_x0(F.x, (int64_t)b * F.n + i);
        x[0] = t.x;
        x[1] = t.y;
    } else {
        ldv<3>(F.x + (int64_t)b * F.n * kV3, i, x);
    }
}
template <int BSF, int XM = 0>
__device__ __forceinline__ void st_xf(const Lvl &F, int32_t b, int32_t i, const float (&x)[BSF]) {
    if constexpr (BSF == 3)
        stv<3>(F.x + (int64_t)b * F.n * kV3, i, x);
    else if constexpr (XM == 2)
        reinterpret_cast<float2 *>(F.y)[(int64_t)b * F.n + i] = make_float2(x[0], x[1]);
    else
        st_x0(F.x, (int64_t)b * F.n + i, x[0], x[1]);
}

// b_C[I] = sum over the members of aggregate I of Q^T r (member order,
// contiguous, U at a time); with smooth also x_C[I] = w D_C^-1 b_C[I].
// Level 0's restricted residual r1 stays in aggregate member order too
// (k_res0_ns scatters into it): node order made k_res0's stores coalesced
// (1053 -> 961 us) but the restriction's member gathers scattered (233 ->
// 361 us), a net loss (round 2, C3, B = 512).
template <int BSF>
__device__ __forceinline__ void restrict_node(const Lvl &F, const Lvl &C, int32_t b, int32_t I, bool smooth,
                                              float omega) {
    constexpr int U = 4;
    float acc[3] = {0.f, 0.f, 0.f};
    const int32_t q0 = F.mptr[I], q1 = F.mptr[I + 1];
    for (int32_t t0 = q0; t0 < q1; t0 += U) {
        float ri[U][BSF], qm[U][BSF * 3];
#pragma unroll
        for (int u = 0; u < U; ++u) ldr<BSF>(F.r, b, F.n, min(t0 + u, q1 - 1), ri[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float *p = F.Qm + (int64_t)min(t0 + u, q1 - 1) * BSF * 3;
#pragma unroll
            for (int k = 0; k < BSF * 3; ++k) qm[u][k] = p[k];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float on = t0 + u < q1 ? 1.f : 0.f;
#pragma unroll
            for (int k = 0; k < BSF; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c] += qm[u][3 * k + c] * (on * ri[u][k]);
        }
    }
    coarse_store(C, b, I, acc, smooth, omega);
}

// coarse level, tentative prolongator: x_i += Q_i y_C[agg(i)]
__device__ __forceinline__ void prolong_node(const Lvl &F, const Lvl &C, int32_t b, int32_t i) {
    float y[3], xi[3];
    ldv<3>(C.y + (int64_t)b * C.n * kV3, F.agg[i], y);
    ld_xf<3>(F, b, i, xi);
    const float *qi = F.Q + (int64_t)i * 9;
#pragma unroll
    for (int k = 0; k < 3; ++k) xi[k] += qi[3 * k] * y[0] + qi[3 * k + 1] * y[1] + qi[3 * k + 2] * y[2];
    st_xf<3>(F, b, i, xi);
}

// coarse level: y = x + w D^-1 (b - A x)
__device__ __forceinline__ void post3_node(const Lvl &L, int32_t b, int32_t i, float omega) {
    const int64_t vo = (int64_t)b * L.n * kV3;
    float ax[3], res[3], xi[3], d[3][3], dr[3];
    spmv_row3(L, b, i, L.x + vo, ax);
    ldv<3>(L.b + vo, i, res);
    ldv<3>(L.x + vo, i, xi);
    ld_dh(L, b, i, d);
#pragma unroll
    for (int c = 0; c < 3; ++c) res[c] -= ax[c];
    matvec<3>(d, res, dr);
#pragma unroll
    for (int c = 0; c < 3; ++c) xi[c] += omega * dr[c];
    stv<3>(L.y + vo, i, xi);
}

__global__ __launch_bounds__(kWG) void k_res3(Lvl L, const int32_t *__restrict__ sysi) {
    const int32_t i = blockIdx.x * kWG + threadIdx.x, b = sm_b(L.sm, blockIdx.y);
    if (i >= L.n || retired(sysi, b)) return;
    res3_node(L, b, i);
}

// Restriction by aggregate groups: a workgroup takes whole aggregates with
// at most kRG members in total (group boundaries built on the host), reads
// its members' r and Q rows coalesced (one member per thread), stages the
// per-member contributions Q_q^T r_q in LDS, and one thread per aggregate
// sums them in member order (deterministic). An aggregate with more than
// kRG members forms its own group and is summed straight from memory.
constexpr int kRG = 1024;

// NS systems per workgroup share each member's Q row load; the contributions
// of all NS systems are staged in LDS (level 0: NS = kRestrS = 2, C3 232 ->
// 194 us per 512-system launch; NS = 4: 235 us, its 48-KB LDS stage lowers
// the occupancy).
constexpr int kRestrS = 2;
template <int BSF, int NS = 1>
__global__ __launch_bounds__(kWG) void k_restrict(Lvl F, Lvl C, const int32_t *__restrict__ grp, int32_t ngrp,
                                                  int32_t smooth, float omega, const int32_t *__restrict__ sysi) {
    // no fp contraction: every system slot of the unrolled loops rounds alike
#pragma clang fp contract(off)
    __shared__ float con[NS][3][kRG];
    int32_t g, bq;
    if (!xcd_map(ngrp, (F.sm.n + NS - 1) / NS, g, bq, kGrpRestr)) return;
    const SysGroup<NS> sg{F.sm, sysi, bq * NS};
    if (!sg.any()) return;
    const int32_t I0 = grp[g], I1 = grp[g + 1];
    const int32_t q0 = F.mptr[I0], q1 = F.mptr[I1];
    if (q1 - q0 > kRG) {  // one oversized aggregate
        if (threadIdx.x == 0)
            for (int t = 0; t < NS; ++t)
                if (sg.act(t)) restrict_node<BSF>(F, C, sg.b(t), I0, smooth != 0, omega);
        return;
    }
    for (int32_t q = q0 + threadIdx.x; q < q1; q += kWG) {
        float ri[NS][BSF];
#pragma unroll
        for (int t = 0; t < NS; ++t) ldr<BSF>(F.r, sg.b(t), F.n, q, ri[t]);
        const float *qm = F.Qm + (int64_t)q * BSF * 3;
        float qv[BSF * 3];
#pragma unroll
        for (int k = 0; k < BSF * 3; ++k) qv[k] = qm[k];
#pragma unroll
        for (int t = 0; t < NS; ++t) {
            float c3[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < BSF; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) c3[c] += qv[3 * k + c] * ri[t][k];
#pragma unroll
            for (int c = 0; c < 3; ++c) con[t][c][q - q0] = c3[c];
        }
    }
    __syncthreads();
    for (int32_t I = I0 + threadIdx.x; I < I1; I += kWG) {
        float acc[NS][3] = {};
        for (int32_t q = F.mptr[I]; q < F.mptr[I + 1]; ++q)
#pragma unroll
            for (int t = 0; t < NS; ++t)
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[t][c] += con[t][c][q - q0];
#pragma unroll
        for (int t = 0; t < NS; ++t)
            if (sg.act(t)) coarse_store(C, sg.b(t), I, acc[t], smooth, omega);
    }
}

// Level 0 with a smoothed prolongator: b_C[I] = sum over I's restriction
// list (fine node order) of P^T r (r in node order). As k_restrict: a
// workgroup takes whole coarse nodes with at most kRGS list entries in
// total and kNSR systems; one thread per entry loads the entry and its P
// block once and forms P_e^T r_i of every system into LDS, then one thread
// per (coarse node, system) sums the node's entries in list order; with
// smooth also x_C[I] = w D_C^-1 b_C[I].
// Round 4 (S1, B = 1024, rocprof, profiles/r04_ab/sa_xfer/; V bit-identical,
// tools/vhash.py): the sums by coarse node alone left most of the
// workgroup idle behind a few long serial loops -- by (node, system)
// 1615 -> 1434 us per launch, and 8 instead of 4 systems per workgroup
// 1344 us (48-KB LDS stage); the prolongation with 8 systems per thread
// 1263 -> 1112 us: S1 990 -> 1018 timesteps/s; 16 per thread (72 VGPRs, no
// scratch) 1089 -> 975 us, while 16 systems per restriction workgroup over
// 256-entry groups stay at 1347 us (profiles/r04_ab/sa_xfer/call38/); two
// list entries per thread and pass with their loads in flight together
// 1347 -> 1300 us (call42/).
// Round 5: the entry pass in fine-node order within each group (rperm;
// the per-node sums keep list order, same bits): S1 (1536 systems) 1653 ->
// 1445 us per launch, the level-1 restriction 533 -> 439 us, S1 +0.9 %
// (profiles/r05_ab/restr_sort/).
// (The tentative k_restrict by (aggregate, system): 397 -> 448 us at C3,
// and with two members per thread and pass: 360 vs 360 us (call43/); neither
// kept.)
constexpr int kNSR = 8;    // systems per workgroup in the smoothed-P restriction
constexpr int kNSP = 16;   // systems per thread in the smoothed-P prolongation
constexpr int kRGS = 512;  // list entries per restriction group (smoothed P)
// BSF = 3: level 1's smoothed prolongator (AmgParams::smooth1), r as 12-byte rows
// in node order; round 5 (F3): 938 us per 1024-system launch with one
// (coarse node, system) per thread walking its list
template <int BSF = 2>
__global__ __launch_bounds__(kWG) void k_restrict0_sa(Lvl F, Lvl C, const int32_t *__restrict__ grp, int32_t ngrp,
                                                      int32_t smooth, float omega,
                                                      const int32_t *__restrict__ sysi) {
    // no fp contraction: every system slot of the unrolled loops rounds alike
    // (a system's bits must not depend on its slot, i.e. on the batch split)
#pragma clang fp contract(off)
    __shared__ float con[kNSR][3][kRGS];
    int32_t g, bq;
    const int32_t nq = (F.sm.n + kNSR - 1) / kNSR;
    if (!xcd_map(ngrp, nq, g, bq, kGrpRestr)) return;
    const SysGroup<kNSR> sg{F.sm, sysi, bq * kNSR};
    if (!sg.any()) return;
    const int32_t I0 = grp[g], I1 = grp[g + 1];
    const int32_t e0 = F.rptr[I0], e1 = F.rptr[I1];
    const bool big = e1 - e0 > kRGS;  // one coarse node with an oversized list: summed from memory
    auto contrib = [&](int32_t e, float (&c3)[kNSR][3]) {
        const int32_t i = F.rent[2 * (int64_t)e];
        const float *p = F.Q + (int64_t)F.rent[2 * (int64_t)e + 1] * (BSF * 3);
        float pm[BSF * 3];
#pragma unroll
        for (int k = 0; k < BSF * 3; ++k) pm[k] = p[k];
        float ri[kNSR][BSF];
#pragma unroll
        for (int t = 0; t < kNSR; ++t) ldr<BSF>(F.r, sg.b(t), F.n, i, ri[t]);
#pragma unroll
        for (int t = 0; t < kNSR; ++t)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float v = pm[c] * ri[t][0] + pm[3 + c] * ri[t][1];
                if constexpr (BSF == 3) v += pm[6 + c] * ri[t][2];
                c3[t][c] = v;
            }
    };
    // two entries per thread and pass, both entries' loads in flight together;
    // the entries visited in fine-node order (rperm: adjacent lanes gather
    // adjacent r), each staged at its list slot
    for (int32_t q = e0 + threadIdx.x; q < e1 && !big; q += 2 * kWG) {
        const bool two = q + kWG < e1;
        const int32_t ea = F.rperm ? F.rperm[q] : q;
        const int32_t eb = two ? (F.rperm ? F.rperm[q + kWG] : q + kWG) : ea;
        float c3[2][kNSR][3];
        contrib(ea, c3[0]);
        contrib(eb, c3[1]);
#pragma unroll
        for (int t = 0; t < kNSR; ++t)
#pragma unroll
            for (int c = 0; c < 3; ++c) con[t][c][ea - e0] = c3[0][t][c];
        if (two)
#pragma unroll
            for (int t = 0; t < kNSR; ++t)
#pragma unroll
                for (int c = 0; c < 3; ++c) con[t][c][eb - e0] = c3[1][t][c];
    }
    __syncthreads();
    // one thread per (coarse node, system), nodes adjacent across threads:
    // kNSR times the threads of one per node, each summing its node's
    // entries in list order (the same per-system sums, bit for bit)
    const int32_t nI = I1 - I0;
    for (int32_t q = threadIdx.x; q < nI * kNSR; q += kWG) {
        const int32_t t = q / nI, I = I0 + q - t * nI;
        if (!sg.act(t)) continue;
        float acc[3] = {};
        for (int32_t e = F.rptr[I]; e < F.rptr[I + 1]; ++e) {
            float c3[3];
            if (big) {
                float all[kNSR][3];
                contrib(e, all);
#pragma unroll
                for (int c = 0; c < 3; ++c) c3[c] = all[t][c];
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) c3[c] = con[t][c][e - e0];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += c3[c];
        }
        coarse_store(C, sg.b(t), I, acc, smooth, omega);
    }
}

// Smoothed prolongator: x_i += sum over the fine node's P blocks of
// P_ik y_C[pcol k]; NS systems per thread share the row's P blocks and
// columns, each loaded once. Level 0 (BSF = 2, NS = kNSP; the measurements
// above kNSR): x0_i read as the x0 word, the sum stored in the XM format
// (st_xf). Level 1 (BSF = 3, NS = kNS3, AmgParams::smooth1): 12-byte rows in
// place (round 5, F3: 559 us per 1024-system launch with one system per
// thread).
constexpr int kNS3 = 8;
template <int BSF, int XM, int NS>
__global__ __launch_bounds__(kWG) void k_prolong_sa(Lvl F, Lvl C, int32_t nblk, const int32_t *__restrict__ sysi) {
    // no fp contraction: every system slot of the unrolled loops rounds alike
    // (a system's bits must not depend on its slot, i.e. on the batch split)
#pragma clang fp contract(off)
    int32_t rb, bq;
    if (!xcd_map(nblk, (F.sm.n + NS - 1) / NS, rb, bq, kGrpProl)) return;
    const SysGroup<NS> sg{F.sm, sysi, bq * NS};
    const int32_t i = rb * kWG + threadIdx.x;
    if (i >= F.n) return;
    float x[NS][BSF];
#pragma unroll
    for (int t = 0; t < NS; ++t) ld_xf<BSF>(F, sg.b(t), i, x[t]);
    const int32_t k0 = F.pptr[i], k1 = F.pptr[i + 1];
    for (int32_t k = k0; k < k1; ++k) {
        const int32_t K = F.pcol[k];
        const float *p = F.Q + (int64_t)k * (BSF * 3);
        float pm[BSF * 3];
#pragma unroll
        for (int c = 0; c < BSF * 3; ++c) pm[c] = p[c];
        float y[NS][3];
#pragma unroll
        for (int t = 0; t < NS; ++t) ldv<3>(C.y + (int64_t)sg.b(t) * C.n * kV3, K, y[t]);
#pragma unroll
        for (int t = 0; t < NS; ++t)
#pragma unroll
            for (int r = 0; r < BSF; ++r) x[t][r] += pm[3 * r] * y[t][0] + pm[3 * r + 1] * y[t][1] + pm[3 * r + 2] * y[t][2];
    }
#pragma unroll
    for (int t = 0; t < NS; ++t)
        if (sg.act(t)) st_xf<BSF, XM>(F, sg.b(t), i, x[t]);
}

// coarse level, tentative prolongator: one (node, system) per thread
__global__ __launch_bounds__(kWG) void k_prolong(Lvl F, Lvl C, const int32_t *__restrict__ sysi) {
    const int32_t i = blockIdx.x * kWG + threadIdx.x, b = sm_b(F.sm, blockIdx.y);
    if (i >= F.n || retired(sysi, b)) return;
    prolong_node(F, C, b, i);
}

// Level 0, tentative prolongator, with the XCD-aware (node block, system)
// order: the B systems of a node block run back to back on one XCD and share
// its Q rows in L2 instead of re-reading Q per system (183 vs 261 us per
// 256-system launch with the system-major grid; the coarse levels' kernels
// measured slower this way). One node of kProlS systems per thread, every
// load of the batch issued before the first store: one node of one system per
// thread left each wave a dependent agg -> y gather and little else
// (latency-bound), and the systems of a thread share the node's agg and Q row
// loads. C3, 512 systems, nodes x systems per thread: 314 us (1 x 1), 270
// (4 x 1), 231 (2 x 2), 202 (1 x 4), 210 (1 x 8)
constexpr int kProlS = 4;
template <int XM>
__global__ __launch_bounds__(kWG) void k_prolong0(Lvl F, Lvl C, int32_t nblk, const int32_t *__restrict__ sysi) {
    // no fp contraction: every system slot of the unrolled loops rounds alike
#pragma clang fp contract(off)
    int32_t rb, bq;
    if (!xcd_map(nblk, (F.sm.n + kProlS - 1) / kProlS, rb, bq, kGrpProl)) return;
    const SysGroup<kProlS> sg{F.sm, sysi, bq * kProlS};
    const int32_t ii = rb * kWG + threadIdx.x, i = min(ii, F.n - 1);  // a lane past the last node loads that one
    const int32_t ag = F.agg[i];
    float q[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) q[k] = F.Q[(int64_t)i * 6 + k];
    float x[kProlS][2], y[kProlS][3];
#pragma unroll
    for (int t = 0; t < kProlS; ++t) {
        ld_xf<2>(F, sg.b(t), i, x[t]);
        ldv<3>(C.y + (int64_t)sg.b(t) * C.n * kV3, ag, y[t]);
    }
#pragma unroll
    for (int t = 0; t < kProlS; ++t) {
        if (!sg.act(t) || ii >= F.n) continue;
#pragma unroll
        for (int k = 0; k < 2; ++k) x[t][k] += q[3 * k] * y[t][0] + q[3 * k + 1] * y[t][1] + q[3 * k + 2] * y[t][2];
        st_xf<2, XM>(F, sg.b(t), ii, x[t]);
    }
}

__global__ __launch_bounds__(kWG) void k_post3(Lvl L, float omega, const int32_t *__restrict__ sysi) {
    const int32_t i = blockIdx.x * kWG + threadIdx.x, b = sm_b(L.sm, blockIdx.y);
    if (i >= L.n || retired(sysi, b)) return;
    post3_node(L, b, i, omega);
}

// The cycle below level S (all levels with <= kSubNodes nodes) in one launch:
// one workgroup per system walks the tiny levels with barriers in between,
// replacing ~4 launches per level.
// 512 threads: a 400-node level (the 3,249-vertex S1s's level 1) takes one
// row per thread in its sweeps instead of two
constexpr int kSubWG = 512;
// kSubNodes: mof_amg.h
constexpr int kMaxLevels = 12;

struct SubArgs {
    int32_t first, last;  // levels first..last (last = coarsest), first >= 1
    Lvl lv[kMaxLevels];
    const float *cinv;
    float omega;
    const int32_t *sysi;
};

__global__ __launch_bounds__(kSubWG) void k_subcycle(SubArgs a) {
    const int32_t b = sm_b(a.lv[0].sm, blockIdx.x);
    if (retired(a.sysi, b)) return;
    const int32_t tid = threadIdx.x;
    // down: level first already holds b and the pre-smoothed x
    for (int32_t l = a.first; l < a.last; ++l) {
        const Lvl &F = a.lv[l], &C = a.lv[l + 1];
        for (int32_t i = tid; i < F.n; i += kSubWG) res3_node(F, b, i);
        __syncthreads();
        for (int32_t I = tid; I < C.n; I += kSubWG) restrict_node<3>(F, C, b, I, l + 1 < a.last, a.omega);
        __syncthreads();
    }
    // coarsest: y = A_c^-1 b (the inverse is symmetric: read by columns);
    // b staged in LDS, the k range split over the kH groups of kMaxCoarse
    // threads, 16 independent loads in flight per thread, the groups'
    // partial sums added in group order
    {
        constexpr int kH = kSubWG / kMaxCoarse;
        __shared__ float bl[kMaxCoarse];
        __shared__ float part[kH][kMaxCoarse];
        const Lvl &C = a.lv[a.last];
        const int32_t nc = 3 * C.n;
        const float *Mi = a.cinv + (int64_t)b * nc * nc;
        const float *bb = C.b + (int64_t)b * C.n * kV3;  // dof q of the level: word q
        for (int32_t q = tid; q < nc; q += kSubWG) bl[q] = bb[q];
        __syncthreads();
        const int32_t d = tid % kMaxCoarse, hf = tid / kMaxCoarse;
        const int32_t chunk = (nc + kH - 1) / kH;
        const int32_t k0 = min(nc, hf * chunk), k1 = min(nc, k0 + chunk);
        float sum = 0.f;
        if (d < nc) {
            constexpr int U = 16;
            for (int32_t k = k0; k < k1; k += U) {
                float mv[U];
#pragma unroll
                for (int u = 0; u < U; ++u) mv[u] = Mi[(int64_t)min(k + u, k1 - 1) * nc + d];
#pragma unroll
                for (int u = 0; u < U; ++u) sum += (k + u < k1) ? mv[u] * bl[min(k + u, k1 - 1)] : 0.f;
            }
        }
        part[hf][d] = sum;
        __syncthreads();
        if (!hf && d < nc) {
            float t = part[0][d];
#pragma unroll
            for (int h = 1; h < kH; ++h) t += part[h][d];
            C.y[(int64_t)b * C.n * kV3 + d] = t;
        }
        __syncthreads();
    }
    // up
    for (int32_t l = a.last - 1; l >= a.first; --l) {
        const Lvl &F = a.lv[l], &C = a.lv[l + 1];
        for (int32_t i = tid; i < F.n; i += kSubWG) prolong_node(F, C, b, i);
        __syncthreads();
        for (int32_t i = tid; i < F.n; i += kSubWG) post3_node(F, b, i, a.omega);
        __syncthreads();
    }
}

// Level 0: r1 = r - A x0 (x0 = w D^-1 r from the PCG update), stored at the
// member position of each vertex; PCG row layout. NS systems per thread sharing the row's column / mirror loads:
// grid over (row block, system group of NS) in the XCD order (round 2: 916
// -> 829 us per 512-system launch at NS = 2; 4 lowered the occupancy).
// PK: the packed index words (kIxPack) instead of the run-time choice between
// the plain and the mirrored 32-bit tables; the launcher picks the instance.
constexpr int kRes0NS = 2, kRes0U = kSweepU;
template <int NS, bool PK>
__global__ __launch_bounds__(kWG) MOF_ROW_OCC void k_res0_ns(int32_t N, int32_t nblk, SysMap sm, MatH mat,
                                                 const float *__restrict__ rv, const float *__restrict__ xv,
                                                 const int32_t *__restrict__ apos,
                                                 const int32_t *__restrict__ sysi, float *__restrict__ r1) {
#pragma clang fp contract(off)
    int32_t rb, bq;
    if (!xcd_map(nblk, (sm.n + NS - 1) / NS, rb, bq, kGrpSmooth > NS ? kGrpSmooth / NS : 1)) return;
    int32_t bs[NS];
    bool act[NS];
    bool any = false;
#pragma unroll
    for (int t = 0; t < NS; ++t) {
        const int32_t l = bq * NS + t;
        bs[t] = sm_b(sm, l);
        act[t] = l < sm.n && !retired(sysi, bs[t]);
        any |= act[t];
    }
    if (!any) return;
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const int32_t i = rb * kRowsPerWG + r * kWG + threadIdx.x;
        if (i >= N) break;
        float y[NS][2];
        auto xl = [&](int t, int32_t j) { return ld_x0(xv, (int64_t)bs[t] * N + j); };
        if constexpr (PK)
            spmv_row_hx_ns<kIxPack, NS, kRes0U>(mat, bs, i, xl, y);
        else if (mat.sell_mir)
            spmv_row_hx_ns<kIxMir, NS, kRes0U>(mat, bs, i, xl, y);
        else
            spmv_row_hx_ns<kIxPlain, NS, kRes0U>(mat, bs, i, xl, y);
#pragma unroll
        for (int t = 0; t < NS; ++t) {
            if (!act[t]) continue;
            const int64_t vb = (int64_t)bs[t] * N;
            const float2 ri = reinterpret_cast<const float2 *>(rv)[vb + i];
            reinterpret_cast<uint32_t *>(r1)[vb + (apos ? apos[i] : i)] =
                bf16_bits(ri.x - y[t][0]) | (bf16_bits(ri.y - y[t][1]) << 16);
        }
    }
}

// Level 0's post-smoothing z = x + w D^-1 (r - A x) and the PCG's partial
// r.z, NS systems per thread sharing the row's column / mirror loads, 4 slots
// per load batch to keep the waves (round 2: 918 -> 864 us per 512-system
// launch; 8 slots per batch 1030 us). D^-1 from the row's own diagonal block.
constexpr int kPost0NS = 2, kPost0U = 4;
template <int XM, bool ZH, int NS, bool PK>
__global__ __launch_bounds__(kWG) MOF_ROW_OCC void k_post0_ns(int32_t N, int32_t nblk, int32_t B, SysMap sm, MatH mat,
                                                  const float *__restrict__ rv,
                                                  const float *__restrict__ xv, float omega,
                                                  const int32_t *__restrict__ sysi,
                                                  float *__restrict__ zv, double *__restrict__ part,
                                                  RedArgs rd) {
#pragma clang fp contract(off)
    __shared__ double lds[8 * NS];
    int32_t rb, bq;
    if (!xcd_map(nblk, (sm.n + NS - 1) / NS, rb, bq, kGrpSmooth > NS ? kGrpSmooth / NS : 1)) return;
    int32_t bs[NS];
    bool act[NS];
    bool any = false;
#pragma unroll
    for (int t = 0; t < NS; ++t) {
        const int32_t l = bq * NS + t;
        bs[t] = sm_b(sm, l);
        act[t] = l < sm.n && !retired(sysi, bs[t]);
        any |= act[t];
    }
    if (!any) return;
    double rz[NS];
#pragma unroll
    for (int t = 0; t < NS; ++t) rz[t] = 0.0;
#pragma unroll
    for (int g = 0; g < kRows; ++g) {
        const int32_t i = rb * kRowsPerWG + g * kWG + threadIdx.x;
        if (i >= N) break;
        float y[NS][2];
        uint2 dg[NS];  // the rows' diagonal blocks (slot 0), kept from the SpMV
        auto xl = [&](int t, int32_t j) {
            const int64_t vj = (int64_t)bs[t] * N + j;
            if constexpr (XM == 2)
                return reinterpret_cast<const float2 *>(xv)[vj];
            else
                return ld_x0(xv, vj);
        };
        if constexpr (PK)
            spmv_row_hx_ns<kIxPack, NS, kPost0U>(mat, bs, i, xl, y, dg);
        else if (mat.sell_mir)
            spmv_row_hx_ns<kIxMir, NS, kPost0U>(mat, bs, i, xl, y, dg);
        else
            spmv_row_hx_ns<kIxPlain, NS, kPost0U>(mat, bs, i, xl, y, dg);
#pragma unroll
        for (int t = 0; t < NS; ++t) {
            const int64_t vb = (int64_t)bs[t] * N;
            const float2 xi = xl(t, i);
            const float2 ri = reinterpret_cast<const float2 *>(rv)[vb + i];
            const float2 ds = bf16_diag_solve(dg[t], ri.x - y[t][0], ri.y - y[t][1]);
            float z0 = xi.x + omega * ds.x;
            float z1 = xi.y + omega * ds.y;
            if constexpr (ZH) {
                const uint32_t h = bf16_bits(z0) | (bf16_bits(z1) << 16);
                if (act[t]) reinterpret_cast<uint32_t *>(zv)[vb + i] = h;
                z0 = bf16_lo(h);
                z1 = bf16_hi(h);
            } else {
                if (act[t]) reinterpret_cast<float2 *>(zv)[vb + i] = make_float2(z0, z1);
            }
            if (i < rd.nown) rz[t] += (double)ri.x * z0 + (double)ri.y * z1;
        }
    }
    block_sum<NS>(rz, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int t = 0; t < NS; ++t)
            if (act[t]) part[2 * (((int64_t)rd.part * B + bs[t]) * rd.nmax + rb)] = rz[t];
    }
}

// Open surfaces: `sweeps` extra block-Jacobi sweeps (damping omega, b = r)
// on the boundary rows and their neighbour ring only, after the fused
// pre-smoothing and before the post-smoothing (the cycle stays symmetric).
// At a Neumann boundary vertex the diagonal block lacks the missing
// triangles, so one damped sweep leaves those rows least smoothed.
// The ring is its own small SELL-64 matrix (per mesh, host-built: ring
// position p's slot t at bsw_roff[p/64] + 64 t + p%64, the same slots in the
// same order as the row's level-0 SELL slots, padding included): per slot
// the operand's source, a ring position (>= 0), an outside column (-1 - k:
// bsw_ocol[k]) or none (kBswOff), and per batch the slot's bf16 block
// gathered (transposed where the symmetric reads would) from the level-0
// sweep copy by k_bsw_extract. One workgroup per system: the ring's iterates
// (two buffers: a Jacobi sweep reads only the previous one) and the outside
// operands, which do not change, live in LDS; the blocks stream coalesced.
// The same products summed in the same order as spmv_row_hx_ns: the same
// bits as the level-0 kernels' arithmetic. Round 6: the first version read
// the ring rows' slots in place (three dependent trips per slot, one
// scattered line per block): 705 us per 2-sweep launch on S1, 1536 systems.
// F32X: x as fp32 pairs (the corrected iterate with xm = 2), else the bf16
// x0 format.
constexpr int kBswWG = 1024;
constexpr int32_t kBswOff = INT32_MIN;
constexpr int64_t kBswLdsMax = 160 * 1024;  // a workgroup may take the CU's whole LDS (gfx950)
struct BswArgs {
    int32_t N, nbr, nout, nslot;
    const int32_t *rows, *roff, *wrow, *xsrc, *ocol;
    const uint2 *A;  // [cap][nslot] blocks
};
template <bool F32X>
__device__ __forceinline__ float2 bsw_ldx(const float *xv, int64_t vj) {
    if constexpr (F32X)
        return reinterpret_cast<const float2 *>(xv)[vj];
    else
        return ld_x0(xv, vj);
}
// per batch: the ring slots' blocks of every system from the level-0 copy
__global__ __launch_bounds__(kWG) void k_bsw_extract(int32_t nslot, int32_t B, const int32_t *__restrict__ bsrc,
                                                     const uint2 *__restrict__ A0h, int64_t sell_nb,
                                                     uint2 *__restrict__ out) {
    const int64_t q = (int64_t)blockIdx.x * kWG + threadIdx.x;
    if (q >= (int64_t)nslot * B) return;
    const int32_t b = (int32_t)(q / nslot), t = (int32_t)(q - (int64_t)b * nslot);
    const int32_t src = bsrc[t];
    uint2 h = make_uint2(0u, 0u);
    if (src >= 0) {
        h = h0_ld(A0h, (int64_t)b * sell_nb + (src & kMirPos));
        if (src & kMirT) h = h0_tr(h);
    }
    out[q] = h;
}
template <bool F32X>
__global__ __launch_bounds__(kBswWG) void k_bsweep(BswArgs a, SysMap sm, const float *__restrict__ rv,
                                                   float *__restrict__ xv, float omega, int32_t sweeps,
                                                   const int32_t *__restrict__ sysi) {
#pragma clang fp contract(off)
    extern __shared__ float2 bsw_lds[];  // [2][nbr] iterates, [nout] outside operands
    if ((int32_t)blockIdx.x >= sm.n) return;
    const int32_t b = sm_b(sm, blockIdx.x);
    if (retired(sysi, b)) return;
    const int64_t vb = (int64_t)b * a.N;
    float2 *xs[2] = {bsw_lds, bsw_lds + a.nbr};
    float2 *xo = bsw_lds + 2 * a.nbr;
    for (int32_t p = threadIdx.x; p < a.nbr; p += kBswWG) xs[0][p] = bsw_ldx<F32X>(xv, vb + a.rows[p]);
    for (int32_t k = threadIdx.x; k < a.nout; k += kBswWG) xo[k] = bsw_ldx<F32X>(xv, vb + a.ocol[k]);
    __syncthreads();
    const uint2 *Ab = a.A + (int64_t)b * a.nslot;
    constexpr int U = kPost0U;
    int cur = 0;
    for (int32_t k = 0; k < sweeps; ++k) {
        for (int32_t p = threadIdx.x; p < a.nbr; p += kBswWG) {
            const int32_t base = a.roff[p >> 6] + (p & 63), w = a.wrow[p];
            const float2 ri = reinterpret_cast<const float2 *>(rv)[vb + a.rows[p]];
            float acc0 = 0.f, acc1 = 0.f;
            uint2 dg = make_uint2(0u, 0u);
            for (int32_t t0 = 0; t0 < w; t0 += U) {
                int32_t src[U];
                uint2 blk[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int32_t q = base + min(t0 + u, w - 1) * kSlice;
                    src[u] = a.xsrc[q];
                    blk[u] = Ab[q];
                }
                if (t0 == 0) dg = blk[0];  // slot 0: the diagonal block
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const bool on = t0 + u < w && src[u] != kBswOff;
                    float2 xj = make_float2(0.f, 0.f);
                    if (on) xj = src[u] >= 0 ? xs[cur][src[u]] : xo[-1 - src[u]];
                    float e00, e01, e10, e11;
                    h0_dec(blk[u], e00, e01, e10, e11);
                    acc0 += on ? e00 * xj.x + e01 * xj.y : 0.f;
                    acc1 += on ? e10 * xj.x + e11 * xj.y : 0.f;
                }
            }
            const float2 ds = bf16_diag_solve(dg, ri.x - acc0, ri.y - acc1);
            const float2 xi = xs[cur][p];
            xs[cur ^ 1][p] = make_float2(xi.x + omega * ds.x, xi.y + omega * ds.y);
        }
        __syncthreads();
        cur ^= 1;
    }
    for (int32_t p = threadIdx.x; p < a.nbr; p += kBswWG) {
        const float2 v = xs[cur][p];
        if constexpr (F32X)
            reinterpret_cast<float2 *>(xv)[vb + a.rows[p]] = v;
        else
            st_x0(xv, vb + a.rows[p], v.x, v.y);
    }
}
BswArgs bsw_args(const AmgDevice &G) {
    BswArgs a;
    a.N = G.bsw_N;
    a.nbr = G.bsw_n;
    a.nout = G.bsw_nout;
    a.nslot = G.bsw_nslot;
    a.rows = G.bsw_rows.p;
    a.roff = G.bsw_roff.p;
    a.wrow = G.bsw_wrow.p;
    a.xsrc = G.bsw_xsrc.p;
    a.ocol = G.bsw_ocol.p;
    a.A = reinterpret_cast<const uint2 *>(G.bsw_A.p);
    return a;
}
template <bool F32X>
void launch_bsweep(const AmgDevice &G, SysMap sm, const float *rv, float *xv, float omega, const int32_t *sysi,
                   hipStream_t s) {
    const size_t lds = sizeof(float2) * (2 * (size_t)G.bsw_n + G.bsw_nout);
    ++g_vcycle_launches[F32X ? kVcBsweepF : kVcBsweepH];
    k_bsweep<F32X><<<dim3((unsigned)sm.n), kBswWG, lds, s>>>(bsw_args(G), sm, rv, xv, omega, G.bsw_sweeps, sysi);
}

template <int XM, typename... Args>
void launch_post0(bool zh, bool packed, int32_t nblk, int32_t B, hipStream_t s, Args... args) {
    const dim3 g(xcd_grid(nblk, (B + kPost0NS - 1) / kPost0NS, kGrpSmooth > kPost0NS ? kGrpSmooth / kPost0NS : 1));
    ++g_vcycle_launches[kVcPost0 + (XM - 1) * 4 + (zh ? 2 : 0) + (packed ? 1 : 0)];
    (zh ? (packed ? k_post0_ns<XM, true, kPost0NS, true> : k_post0_ns<XM, true, kPost0NS, false>)
        : (packed ? k_post0_ns<XM, false, kPost0NS, true> : k_post0_ns<XM, false, kPost0NS, false>))
        <<<g, kWG, 0, s>>>(args...);
}

inline dim3 grid2(int64_t n, int32_t B) { return dim3((unsigned)((n + kWG - 1) / kWG), (unsigned)B); }

MatH level0_mat(mof_mesh *m) {
    MatH mt;
    mt.sell_nb = m->pat.sell_nb();
    mt.sell_off = m->sell_off.p;
    mt.sell_col = m->sell_col.p;
    mt.sell_mir = m->sym_reads ? m->sell_mir.p : nullptr;
    mt.sell_idx = m->sym_reads && m->idx_packed ? m->sell_idx.p : nullptr;
    mt.vptr = m->sym_reads ? nullptr : m->vptr.p;
    mt.A = reinterpret_cast<const uint2 *>(m->amg->A0h.p);
    return mt;
}

}  // namespace

// ---- host side ---------------------------------------------------------------

bool amg_build(mof_mesh *m) {
    AmgParams prm;
    // an open surface (boundary edges: 3 M != 2 E) damps the fine smoother
    // more: at a Neumann boundary vertex the diagonal block lacks the missing
    // triangles while its couplings stay, and 0.85 leaves the block-Jacobi
    // sweep non-contractive there -- round 4, the S1-like patches: every
    // multigrid solve broke down at 0.85 (3,249 and 160,801 vertices), none at
    // 0.7 (S1s 22.5 PCG its/timestep); on the closed meshes 0.7 costs C3
    // 17.0 -> 18.5 its (-7 %) and C2 21.6 -> 23.0, R3 51.4 -> 50.6
    // (profiles/r04_ab/call4/). A decomposed part keeps 0.85 (its ghost rows
    // are decoupled, not a Neumann boundary).
    const bool open_surface = [&] {
        const int64_t E = ((int64_t)m->pat.nblocks() - m->N) / 2;
        return m->n_own == m->N && 3 * (int64_t)m->M != 2 * E;
    }();
    // and takes the smoothed prolongator (the translations an open patch
    // nearly leaves free converge slowly on the tentative one: S1, 160,801
    // vertices, 86 -> 51.5 PCG its/timestep; the 3,249-vertex S1s is
    // irregular enough to have it already)
    if (open_surface) {
        prm.omega = 0.7f;
        prm.smooth = 1;
    }
    // MOF_AMG_OMEGA = w0[,w1]: the fine [and coarse] smoother damping
    float omega1_set = 0.f;
    if (const char *v = knob(Knob::AmgOmega)) {
        char *end = nullptr;
        prm.omega = std::strtof(v, &end);
        if (end && *end == ',') omega1_set = prm.omega1 = std::strtof(end + 1, nullptr);
    }
    if (knob(Knob::AmgSmooth)) prm.smooth = knob_int(Knob::AmgSmooth, 0) != 0;  // 1 / 0 force, unset auto
    // level 1's smoothed prolongator: auto (below: where level 0 is smoothed,
    // and folded closed surfaces)
    prm.smooth1 = -1;
    if (m->n_own < m->N) prm.nown = m->n_own;
    if (m->amg && m->amg->built) return m->amg->lv.size() >= 2;
    if (!m->amg) m->amg = new AmgDevice();
    AmgDevice &G = *m->amg;
    hipStream_t s = m->stream;
    // the host hierarchy of this mesh and parameter set: built once per mesh
    // and shared by its handles on other devices (MeshShared); the inputs
    // (pattern, e, a2) are the same on every device, bit for bit
    MeshShared *sh = m->shared.get();
    char key[160];
    std::snprintf(key, sizeof(key), "%a/%a/%d/%d/%a/%d/%d", (double)prm.omega, (double)prm.omega1, prm.smooth,
                  prm.nown, (double)prm.smooth_omega, (int)m->sym_reads, prm.smooth1);
    std::unique_lock<std::mutex> build_lock;
    std::shared_ptr<const AmgHierarchy> Hp;
    if (sh) {
        build_lock = std::unique_lock<std::mutex>(sh->amg_build_mu);
        std::lock_guard<std::mutex> lk(sh->mu);
        for (const auto &kv : sh->amg)
            if (kv.first == key) Hp = kv.second;
    }
    if (!Hp) {
        std::vector<double> e(6 * (size_t)m->N);
        MOF_HIP(hipMemcpyAsync(e.data(), m->e.p, e.size() * sizeof(double), hipMemcpyDeviceToHost, s));
        MOF_HIP(hipStreamSynchronize(s));
        // the mesh's a2 (unscaled, fine SELL layout) for the smoothed prolongator
        std::vector<double> a2;
        if (prm.nown < 0 && ((prm.smooth != 0 && (prm.smooth > 0 || amg_auto_smooth(m->pat))) || prm.smooth1 != 0)) {
            a2.resize(4 * (size_t)m->pat.sell_nb());
            MOF_HIP(hipMemcpyAsync(a2.data(), m->a2.p, a2.size() * sizeof(double), hipMemcpyDeviceToHost, s));
            MOF_HIP(hipStreamSynchronize(s));
            prm.a2 = a2.data();
        }
        if (!m->agg_order.empty()) prm.order = m->agg_order.data();
        // the level-0 gather lists read every lower block as its upper twin
        // transposed, whichever way the row kernels read: with plain reads the
        // fp32 operator's lower blocks are assembled on their own and differ
        // from the transposed upper ones by rounding, and the products (which
        // compute the upper coarse blocks and mirror them, st_pair) would
        // otherwise give the Galerkin operator of no single matrix
        const std::vector<int32_t> mir = sell_mirror(m->pat, m->n_own, 1, nullptr);
        prm.mirror = mir.data();
        auto built = std::make_shared<AmgHierarchy>();
        AmgParams p1 = prm;
        // level 1 smoothed at once where level 0 is (irregular or open
        // surfaces): round 5, same box (profiles/r05_ab/sa1/): R3 742 ->
        // 842 timesteps/s (53.6 -> 41.8 PCG its), S1 905 (with the level-1
        // W-cycle, since removed) -> 995 (44.8 its)
        const bool l0_smooth = prm.nown < 0 && prm.a2 && prm.smooth != 0 && (prm.smooth > 0 || amg_auto_smooth(m->pat));
        p1.smooth1 = prm.smooth1 > 0 ? prm.smooth1 : (prm.smooth1 < 0 && l0_smooth ? 1 : 0);
        // open surfaces: every explicit coarse level smoothed (with the
        // boundary sweeps below; round 6, same box, profiles/r06/bsw/): S1
        // 1,188 -> 1,377 timesteps/s, 42.9 -> 35.5 PCG its (alone, without the
        // sweeps: 1,121 at 46.1 its -- the CPU prototype agrees, 36 -> 36
        // its to 1e-8 alone, 30 with them, tools/amg_proto.py); S1m / S1s
        // have no explicit level past 1 (the same hierarchy)
        if (open_surface && p1.smooth1 == 1) p1.smooth1 = 2;
        build_amg(m->pat, e.data(), p1, *built);
        // auto: a closed surface whose coarse aggregates turn strongly (the
        // median sigma_3 / sigma_1 of their near-null blocks >= kFoldCurl at
        // some level: folds at the coarse levels' scale) is rebuilt with
        // level 1's prolongator smoothed, and level 0's too where the finest
        // aggregates stay flat (curl[0] < kFlatCurl: a folded surface, not a
        // rough one -- the 640k jittered sphere C5 turns 0.34 at level 0 and
        // loses 9 % with level 0 smoothed, 945 -> 859 timesteps/s at 15.2 ->
        // 13.0 its, profiles/r06/sweep/C5.json; F3 turns 0.07 there;
        // MOF_AMG_SMOOTH = 0 keeps level 0 tentative). Round 5, same box
        // (profiles/r05_ab/sa1/): level 1 alone, F3 (curl 0.46-0.51) 2003 ->
        // 2292 timesteps/s, 31.0 -> 26.2 PCG its; C3 (curl <= 0.25) gains no
        // iteration (17.0) and loses 12 % to the level-1 product. Round 6,
        // same box (profiles/r06/f3_fold/): level 0 as well, with the
        // regular mesh's storage formats kept (below), F3 2548 / 2584 ->
        // 2794 / 2797 timesteps/s, 26.2 -> 17.5 its (level 0 smoothed with
        // the irregular meshes' fp32 iterates: 19.0 its, 2546)
        if (prm.smooth1 < 0 && p1.smooth1 == 0 && prm.nown < 0 && prm.a2 && !built->levels.empty() &&
            !built->levels[0].smoothed && built->max_curl >= kFoldCurl) {
            const double curl = built->max_curl;
            p1.smooth1 = 1;
            if (prm.smooth != 0 && !built->curl.empty() && built->curl[0] < kFlatCurl) p1.smooth = 1;
            auto again = std::make_shared<AmgHierarchy>();
            build_amg(m->pat, e.data(), p1, *again);
            again->max_curl = curl;
            again->folded = true;
            built = again;
        }
        built->mirror = mir;
        Hp = built;
        if (sh) {
            std::lock_guard<std::mutex> lk(sh->mu);
            sh->amg.emplace_back(key, Hp);
        }
    }
    if (build_lock.owns_lock()) build_lock.unlock();
    const AmgHierarchy &H = *Hp;
    G.H = Hp;
    G.omega = prm.omega;
    G.omega1 = prm.omega1;
    // level 0's corrected iterate x0 + Q y: bf16 in place on meshes with the
    // tentative prolongator (C3 +3.8 %, C2 mixed +3.3 %, same iterations),
    // fp32 with the smoothed one (R3: bf16 costs 54.5 vs 50 its, -5 %)
    G.xm = 2;
    G.lv.clear();
    G.built = true;
    // a mesh that does not coarsen (<= 42 vertices) keeps block Jacobi
    if (H.levels.size() < 2) return false;
    // The bf16 iterates (x here, z in the PCG) and omega1 = 1.1 were tuned on
    // the regular meshes; an irregular mesh keeps fp32 and 1.05 whichever
    // prolongator it runs (round 3: R3 forced onto the tentative P took
    // 146.5 PCG its/timestep with the regular meshes' choices)
    // (round 4: and closed -- an open patch's near-null modes suffer from
    // the bf16 iterates as from the stronger coarse damping). The choice
    // follows the mesh, not the prolongator: a regular closed mesh keeps
    // them with a smoothed level 0 too (round 6: F3 folded 17.5 its, +9 %;
    // C3 forced smoothed, round 5: 3653-3730 vs 3253-3268 timesteps/s
    // without them)
    G.regular = !amg_auto_smooth(m->pat) && !open_surface;
    G.xm = G.regular ? 1 : 2;
    // coarse-level damping: 1.1 on regular meshes (round 2, C3 17.2 -> 17.0
    // its, +1.8 %; C2 mixed +2 %), 1.05 otherwise (R3 as measured; 1.2
    // diverges there with the tentative P)
    if (omega1_set <= 0.f) G.omega1 = G.regular ? 1.1f : 1.05f;
    // (a W-cycle at level 1 -- the levels below visited twice -- was
    // measured in rounds 5-6 and removed: slower than level 1's smoothed
    // prolongator on every mesh (S1 905 vs 995, F3 1934 vs 2292, C3 3370 vs
    // 3652 timesteps/s, profiles/r05_ab/wcycle/), and together with it it
    // broke 15 of 3072 S1 solves down: the cycle below level 1 over-corrects
    // there (lambda(B2 A2) up to 2.2 with the coarse damping 1.05,
    // tools/wcycle_study.py), which a V-cycle tolerates and the second
    // coarse correction of a W-cycle does not)
    MOF_REQUIRE(H.coarse_dofs <= kMaxCoarse, "coarsest multigrid level too large");
    MOF_REQUIRE(H.levels.size() <= (size_t)kMaxLevels, "too many multigrid levels");
    G.lv.resize(H.levels.size());
    auto put_i = [&](DevArray<int32_t> &d, const std::vector<int32_t> &h) {
        d.alloc(h.size());
        if (!h.empty()) d.upload(h.data(), h.size(), s);
    };
    auto put_f = [&](DevArray<float> &d, const std::vector<float> &h) {
        d.alloc(h.size());
        if (!h.empty()) d.upload(h.data(), h.size(), s);
    };
    // k_h0_twins; a decomposed part's table (built with nown) names a twin for its owned-owned
    // lower blocks alone, so the ghost rows and columns keep their identity / zero blocks
    if (!m->sym_reads) put_i(G.mir0, H.mirror);
    // open surfaces: the boundary rows (fewer incident triangles than
    // neighbours: the diagonal block's contribution list has one entry per
    // incident triangle) and one ring of their neighbours, for k_bsweep: 2
    // sweeps per side on every open surface whose ring fits the sweep
    // kernel's LDS (a larger ring keeps no boundary sweeps, said under
    // MOF_VERBOSE); MOF_AMG_BSW = sweeps per side (0 off). Round 5 (one
    // workgroup reading the ring rows in place, 705 us per launch on S1) ran
    // them only where the ring is >= 1/20 of the rows (S1s, 14 %: 28.6 ->
    // 19.8 PCG its/timestep); round 6, the ring as its own SELL matrix (180
    // us), same box (profiles/r06/bsw/): S1s 27,458 -> 29,287 timesteps/s
    // (same bits), S1m (ring 4 %) 4,646 -> 6,012 at 43.9 -> 30.9 its, S1
    // (2 %, with its coarse levels smoothed, above) 1,148 -> 1,377.
    G.bsw_n = 0;
    G.bsw_sweeps = 0;
    int32_t bsw = -1;
    if (knob(Knob::AmgBsw)) bsw = std::max(0, std::min(8, knob_int(Knob::AmgBsw, 0)));
    if (open_surface && bsw != 0) {
        const Pattern &P = m->pat;
        std::vector<uint8_t> mark(m->N, 0);
        for (int32_t i = 0; i < m->N; ++i) {
            const int32_t a = P.vptr[i], e2 = P.vptr[i + 1];
            const int32_t d = (int32_t)(std::lower_bound(P.vcol.begin() + a, P.vcol.begin() + e2, i) - P.vcol.begin());
            if (P.cptr[d + 1] - P.cptr[d] < e2 - a - 1) mark[i] = 1;
        }
        std::vector<uint8_t> ring(mark);
        for (int32_t i = 0; i < m->N; ++i)
            if (mark[i])
                for (int32_t q = P.vptr[i]; q < P.vptr[i + 1]; ++q) ring[P.vcol[q]] = 1;
        std::vector<int32_t> rows, pos(m->N, -1);
        for (int32_t i = 0; i < m->N; ++i)
            if (ring[i]) {
                pos[i] = (int32_t)rows.size();
                rows.push_back(i);
            }
        if (!rows.empty()) {
            // the ring's SELL-64 matrix: ring position p's slots are row
            // rows[p]'s level-0 slots (spmv_row_hx_ns's order and masks)
            const int32_t nbr = (int32_t)rows.size(), nrs = (nbr + kSlice - 1) / kSlice;
            std::vector<int32_t> mir;
            if (m->sym_reads) mir = sell_mirror(P, m->n_own, 1, nullptr);
            std::vector<int32_t> wrow(nbr), roff(nrs + 1, 0), ocol, opos(m->N, -1);
            for (int32_t p = 0; p < nbr; ++p) {
                const int32_t s0 = rows[p] / kSlice;
                wrow[p] = (int32_t)((P.sell_off[s0 + 1] - P.sell_off[s0]) / kSlice);
            }
            for (int32_t r = 0; r < nrs; ++r) {
                int32_t wmax = 0;
                for (int32_t p = r * kSlice; p < std::min(nbr, (r + 1) * kSlice); ++p) wmax = std::max(wmax, wrow[p]);
                roff[r + 1] = roff[r] + wmax * kSlice;
            }
            const int32_t nslot = roff[nrs];
            std::vector<int32_t> xsrc(nslot, kBswOff), bsrc(nslot, -1);
            for (int32_t p = 0; p < nbr; ++p) {
                const int32_t i = rows[p], s0 = i / kSlice, l = i % kSlice;
                const int64_t o = P.sell_off[s0];
                const int32_t w = wrow[p];
                const int32_t wl = m->sym_reads ? w : std::min(w, P.vptr[i + 1] - P.vptr[i]);
                for (int32_t t = 0; t < w; ++t) {
                    const int64_t pp = o + (int64_t)std::min(t, wl - 1) * kSlice + l;
                    const int32_t j = P.sell_col[pp];
                    int32_t src = (int32_t)pp;
                    bool on = t < wl;
                    if (m->sym_reads) {
                        const int32_t mr = mir[pp];
                        on = on && mr >= 0;
                        src = mr < 0 ? (int32_t)(o + l) : mr;  // position | kMirT (transposed)
                    }
                    if (!on) continue;
                    const int64_t q = roff[p / kSlice] + (int64_t)t * kSlice + p % kSlice;
                    bsrc[q] = src;
                    if (pos[j] >= 0) {
                        xsrc[q] = pos[j];
                    } else {
                        if (opos[j] < 0) {
                            opos[j] = (int32_t)ocol.size();
                            ocol.push_back(j);
                        }
                        xsrc[q] = -1 - opos[j];
                    }
                }
            }
            const int64_t lds = (int64_t)sizeof(float2) * (2 * (int64_t)nbr + (int64_t)ocol.size());
            if (lds > kBswLdsMax) {
                if (knob(Knob::Verbose))
                    std::fprintf(stderr, "mof amg: boundary ring of %d rows needs %lld B of LDS: no boundary sweeps\n",
                                 nbr, (long long)lds);
            } else {
                put_i(G.bsw_rows, rows);
                put_i(G.bsw_roff, roff);
                put_i(G.bsw_wrow, wrow);
                put_i(G.bsw_xsrc, xsrc);
                put_i(G.bsw_bsrc, bsrc);
                put_i(G.bsw_ocol, ocol);
                G.bsw_N = m->N;
                G.bsw_n = nbr;
                G.bsw_nout = (int32_t)ocol.size();
                G.bsw_nslot = nslot;
                G.bsw_sweeps = bsw > 0 ? bsw : 2;
                if (knob(Knob::Verbose))
                    std::fprintf(stderr, "mof amg: boundary sweeps x%d on a ring of %d rows (%d outside, %lld B of LDS)\n",
                                 G.bsw_sweeps, nbr, G.bsw_nout, (long long)lds);
                // the fixed cap, never this ring's own size: a later mesh's smaller
                // ring must not lower the limit under this mesh's launches
                static LdsLimit limit;
                raise_lds_limit(limit, m->device,
                                {reinterpret_cast<const void *>(&k_bsweep<true>),
                                 reinterpret_cast<const void *>(&k_bsweep<false>)},
                                kBswLdsMax);
            }
        }
    }
    for (size_t l = 0; l < H.levels.size(); ++l) {
        const AmgLevel &L = H.levels[l];
        AmgDevLevel &D = G.lv[l];
        D.n = L.n;
        D.bs = L.bs;
        D.sell_nb = L.sell_nb();
        if (l > 0) {
            {  // each upper block's lower twin (st_pair), -1 elsewhere
                std::vector<int32_t> tw((size_t)L.sell_nb(), -1);
                for (size_t k = 0; k < L.low.size(); ++k) tw[L.twin[k]] = L.low[k];
                put_i(D.twin, tw);
            }
            // the fp32 operator packed (diagonal and upper blocks, 9 floats each) where only
            // the next product reads it: not the coarsest level (k_coarse_inverse), and not
            // level 1 under a smoothed level 0 when its product runs from the system slab
            // (amg_ensure's C.slab, k_galerkin_sys), which keeps [sell_nb][12]
            const bool slab_src = l == 1 && H.levels[0].smoothed && H.levels.size() >= 3 && L.n > kSubNodes;
            D.packed = l + 1 < H.levels.size() && !slab_src;
            D.npk = D.packed ? L.npk : 0;
            if (D.packed) {
                MOF_REQUIRE((int64_t)L.pk.size() == L.sell_nb(), "the level has no packed index table");
                put_i(D.pk, L.pk);
            }
            put_i(D.sell_off, L.sell_off);
            put_i(D.sell_col, L.sell_col);
            put_i(D.sell_row, L.sell_row);
            put_i(D.diag_pos, L.diag_pos);
            D.dead.alloc(L.dead.size());
            D.dead.upload(L.dead.data(), L.dead.size(), s);
        }
        if (l + 1 < H.levels.size()) {
            put_i(D.agg, L.agg);
            put_i(D.mptr, L.mptr);
            put_i(D.mlist, L.mlist);
            put_i(D.apos, L.apos);
            put_i(D.gptr, L.gptr);
            if (D.packed) {
                // the lists name packed blocks: a lower block is its upper twin's, transposed
                std::vector<int32_t> up((size_t)L.sell_nb(), -1), ge(L.gent);
                for (size_t k = 0; k < L.low.size(); ++k) up[L.low[k]] = L.twin[k];
                for (size_t e = 0; e < ge.size(); e += 3) {
                    const int32_t fp = ge[e];
                    if (fp < 0) continue;
                    const int32_t pi = L.pk[fp] >= 0 ? L.pk[fp] : (up[fp] >= 0 ? L.pk[up[fp]] | kMirT : -1);
                    MOF_REQUIRE(pi >= 0, "a gather entry names a position without a block");
                    ge[e] = pi;
                }
                put_i(D.gent, ge);
            } else {
                put_i(D.gent, L.gent);
            }
            put_f(D.Q, L.Q);
            put_f(D.Qm, L.Qm);
            D.smoothed = L.smoothed;
            if (L.smoothed) {
                put_i(D.pptr, L.pptr);
                put_i(D.pcol, L.pcol);
                put_i(D.rptr, L.rptr);
                put_i(D.rent, L.rent);
            }
            // restriction groups: whole aggregates, <= kRG members (smoothed P:
            // restriction list entries) each
            std::vector<int32_t> grp{0};
            const std::vector<int32_t> &gp = L.smoothed ? L.rptr : L.mptr;
            const int32_t na = (int32_t)gp.size() - 1;
            for (int32_t I = 0; I < na; ++I) {
                const int32_t g0 = grp.back();
                if (I > g0 && gp[I + 1] - gp[g0] > (L.smoothed ? kRGS : kRG)) grp.push_back(I);
            }
            grp.push_back(na);
            D.ngrp = (int32_t)grp.size() - 1;
            put_i(D.rgrp, grp);
            // smoothed P: each group's list entries by fine node (stable), for
            // k_restrict0_sa's gathers (same bits as list order)
            if (L.smoothed) {
                std::vector<int32_t> perm(L.rent.size() / 2);
                for (int32_t g = 0; g + 1 < (int32_t)grp.size(); ++g) {
                    const int32_t e0 = L.rptr[grp[g]], e1 = L.rptr[grp[g + 1]];
                    for (int32_t e = e0; e < e1; ++e) perm[e] = e;
                    std::stable_sort(perm.begin() + e0, perm.begin() + e1,
                                     [&](int32_t x, int32_t y) { return L.rent[2 * x] < L.rent[2 * y]; });
                }
                put_i(D.rperm, perm);
            }
            // tentative P (every level but a smoothed level 0): coarse position
            // ranges of <= kWG gather entries and positions for the products by
            // entry, k_galerkin_ent<2> / k_galerkin_ent<3> (unless a level-0
            // position has more). Levels >= 1: positions past kGalBig entries
            // go to k_galerkin3_big.
            if (!L.smoothed || l >= 1) {
                const int32_t big = l == 0 ? 0 : std::min<int32_t>(kWG, kGalBig);
                const std::vector<int32_t> &gq = L.gptr;
                const int32_t npos = (int32_t)gq.size() - 1;
                bool ok = true;
                for (int32_t p = 0; p < npos && ok; ++p) ok = big > 0 || gq[p + 1] - gq[p] <= kWG;
                if (ok) {
                    // [p0, p1) pairs of consecutive positions within the bound;
                    // a big position closes the open range
                    std::vector<int32_t> gg, gbig;
                    int32_t p0 = -1;
                    for (int32_t p = 0; p < npos; ++p) {
                        const bool isbig = big > 0 && gq[p + 1] - gq[p] > big;
                        if (p0 >= 0 && (isbig || gq[p + 1] - gq[p0] > kWG || p - p0 >= kWG)) {
                            gg.push_back(p0);
                            gg.push_back(p);
                            p0 = -1;
                        }
                        if (isbig)
                            gbig.push_back(p);
                        else if (p0 < 0)
                            p0 = p;
                    }
                    if (p0 >= 0) {
                        gg.push_back(p0);
                        gg.push_back(npos);
                    }
                    D.nggrp = (int32_t)gg.size() / 2;
                    put_i(D.ggrp, gg);
                    D.nbig = (int32_t)gbig.size();
                    put_i(D.gbig, gbig);
                }
            }
        }
    }
    G.nc = H.coarse_dofs;
    G.cap = 0;
    if (knob(Knob::Verbose)) {
        for (size_t l = 0; l < H.levels.size(); ++l)
            std::fprintf(stderr, "mof amg level %zu: n=%d bs=%d blocks=%zu sell=%lld%s curl %.3f%s\n", l,
                         H.levels[l].n, H.levels[l].bs, H.levels[l].vcol.size(), (long long)H.levels[l].sell_nb(),
                         H.levels[l].smoothed ? " (smoothed P)" : "", l < H.curl.size() ? H.curl[l] : 0.0,
                         l == 0 && H.folded ? " (folded)" : "");
    }
    MOF_HIP(hipStreamSynchronize(s));
    return true;
}

void amg_ensure(mof_mesh *m, int32_t B) {
    AmgDevice &G = *m->amg;
    if (G.cap >= B) return;
    hipStream_t s = m->stream;
    for (size_t l = 0; l < G.lv.size(); ++l) {
        AmgDevLevel &D = G.lv[l];
        const size_t n = D.n;
        if (l == 0) {
            D.x.alloc(2 * n * B);
            if (G.xm == 2) D.y.alloc(2 * n * B);
            D.r.alloc(n * B);  // bf16 pairs (ldr<2>)
            G.A0h.alloc((size_t)(2 * m->pat.sell_nb() * B));  // 8 B per block
            G.A0h.zero(s);  // SELL padding: never written by the assembly, read as 0
            // the smoothed level-0 Galerkin product by system slab (k_a_slab,
            // k_galerkin_sys)
            if (D.smoothed && G.aslab.n == 0) G.aslab.alloc((size_t)4 * kSlab * m->pat.sell_nb());
        } else {
            D.A.alloc(D.packed ? (size_t)kB9 * D.npk * B : (size_t)kB3 * D.sell_nb * B);
            D.A.zero(s);
            // (a level 1 of the fused tiny levels keeps its product by entry:
            // S1s, 400 nodes, 25050 -> 26450 timesteps/s without the chain)
            if (l == 1 && G.aslab.n > 0 && G.lv.size() >= 3 && D.n > kSubNodes && D.slab.n == 0)
                D.slab.alloc((size_t)kB3 * kSlab * D.sell_nb);
            if (l + 1 < G.lv.size()) {  // sweep copy, st_a9 (the coarsest stays fp32)
                D.Ah.alloc(kAhWords * D.sell_nb * B);
                D.Ah.zero(s);
                D.Ah22.alloc(kAh22Words * D.sell_nb * B);
                D.Ah22.zero(s);
            }
            D.Dh.alloc((size_t)4 * n * B);
            D.Dh22.alloc((size_t)n * B);
            D.b.alloc(kV3 * n * B);
            D.x.alloc(kV3 * n * B);
            D.r.alloc(kV3 * n * B);
            D.y.alloc(kV3 * n * B);
        }
    }
    G.cinv.alloc((size_t)G.nc * G.nc * B);
    if (G.bsw_n > 0) G.bsw_A.alloc((size_t)2 * G.bsw_nslot * B);  // the ring slots' blocks (uint2)
    G.cap = B;
    MOF_HIP(hipStreamSynchronize(s));
}

AmgBf16 amg_bf16_targets(mof_mesh *m, int32_t B) {
    AmgDevice &G = *m->amg;
    MOF_REQUIRE(G.cap >= B, "multigrid storage not sized for the batch");
    G.bf16_fresh = true;
    return AmgBf16{reinterpret_cast<uint2 *>(G.A0h.p)};
}

AmgFine amg_fine(mof_mesh *m) {
    AmgDevice &G = *m->amg;
    AmgFine f;
    f.A0h = G.A0h.p;
    f.sell_nb = m->pat.sell_nb();
    f.sell_off = m->sell_off.p;
    f.x0 = G.lv[0].x.p;
    f.omega = G.omega;
    f.smoothed = G.lv[0].smoothed;
    f.regular = G.regular;
    return f;
}

// the product of level F into level C for a batch of B systems (a sweep copy
// only where C keeps one: every level but the coarsest)
static GalArgs gal_args(const AmgDevLevel &F, const AmgDevLevel &C, int32_t B) {
    GalArgs g;
    g.c_sell_nb = C.sell_nb;
    g.nC = C.n;
    g.B = B;
    g.sell_row = C.sell_row.p;
    g.diag = C.diag_pos.p;
    g.dead = C.dead.p;
    g.twin = C.twin.p;
    g.pk = C.packed ? C.pk.p : nullptr;
    g.c_npk = C.npk;
    g.gptr = F.gptr.p;
    g.gent = F.gent.p;
    g.Q = F.Q.p;
    g.Ac = C.A.p;
    g.Dh = reinterpret_cast<uint4 *>(C.Dh.p);
    g.Dh22 = C.Dh22.p;
    g.Ah = C.Ah.n > 1 ? reinterpret_cast<uint4 *>(C.Ah.p) : nullptr;
    g.Ah22 = C.Ah22.n > 1 ? C.Ah22.p : nullptr;
    return g;
}

void amg_setup_batch(mof_mesh *m, int32_t B, hipStream_t s) {
    AmgDevice &G = *m->amg;
    Workspace &w = m->ws;
    const size_t L = G.lv.size();
    if (!G.bf16_fresh) {
        const int64_t nb0 = m->pat.sell_nb() * B;
        k_to_h0<<<dim3((unsigned)((nb0 + kWG - 1) / kWG)), kWG, 0, s>>>(
            nb0, reinterpret_cast<const float4 *>(w.A32.p), reinterpret_cast<uint2 *>(G.A0h.p));
    }
    G.bf16_fresh = false;
    if (G.mir0.n > 1) {
        const int64_t nb = m->pat.sell_nb();
        MOF_REQUIRE((int64_t)G.mir0.n == nb, "level 0's mirror table does not fit the mesh");
        k_h0_twins<<<dim3((unsigned)((nb + kWG - 1) / kWG), (unsigned)B), kWG, 0, s>>>(
            nb, G.mir0.p, reinterpret_cast<uint2 *>(G.A0h.p));
    }
    if (G.bsw_n > 0) {
        const int64_t n = (int64_t)G.bsw_nslot * B;
        k_bsw_extract<<<dim3((unsigned)((n + kWG - 1) / kWG)), kWG, 0, s>>>(
            G.bsw_nslot, B, G.bsw_bsrc.p, reinterpret_cast<const uint2 *>(G.A0h.p), m->pat.sell_nb(),
            reinterpret_cast<uint2 *>(G.bsw_A.p));
    }
    // a dispatch's grid is at most 2^32 - 1 work-items: a by-entry product
    // whose (group, system pair) grid would pass it (a batch of 1024 over
    // more than ~32k entry groups) takes the per-position kernel -- the same
    // terms in the same order, bit-identical (round 4: an unsliced by-entry
    // launch past the bound skipped workgroups)
    auto fits = [&](int32_t nblk, int32_t ns) {
        const int64_t nq = (B + ns - 1) / ns, sg = sys_group((int32_t)nq, kGrpGal);
        return 8 * sg * ((nq + sg - 1) / sg) * ((nblk + 7) / 8) * kWG < ((int64_t)1 << 32);
    };
    auto ent_fits = [&](const AmgDevLevel &F) {
        return !g_force_galerkin_ns.load() && (F.nggrp > 0 || F.nbig > 0) && fits(F.nggrp, kGalENS) &&
               fits(F.nbig, kGalBigNS);
    };
    // nblk workgroups for each ns systems of the batch
    auto gal_grid = [&](int64_t nblk, int32_t ns) { return dim3(xcd_grid((int32_t)nblk, (B + ns - 1) / ns, kGrpGal)); };
    const int64_t fnb = m->pat.sell_nb();
    const uint2 *A0h = reinterpret_cast<const uint2 *>(G.A0h.p);
    // a smoothed level 0: its product, and level 1's when level 1 kept a
    // slab copy, by system slab (k_a_slab -> k_galerkin_sys<2> -> <3>)
    size_t l_first = 0;
    if (G.lv[0].smoothed && G.aslab.n > 0) {
        AmgDevLevel &C = G.lv[1];
        const bool l1 = L >= 3 && C.slab.n > 0;
        const GalArgs g0 = gal_args(G.lv[0], C, B), g1 = l1 ? gal_args(C, G.lv[2], B) : GalArgs{};
        auto sys_grid = [](int64_t nb) { return dim3(xcd_grid((int32_t)((nb + kGalSysPos - 1) / kGalSysPos), 1, 1)); };
        const dim3 gs((unsigned)((fnb + kSlabPos - 1) / kSlabPos));
        auto *cs = l1 ? reinterpret_cast<float4 *>(C.slab.p) : nullptr;
        for (int32_t b0 = 0; b0 < B; b0 += kSlab) {
            const int32_t nb = std::min(kSlab, B - b0);
            if (G.regular) {
                auto *slab = reinterpret_cast<uint2 *>(G.aslab.p);
                k_a_slab<uint2><<<gs, kWG, 0, s>>>(fnb, b0, nb, A0h, slab);
                ++g_galerkin_launches[kGalSys2Bf16];
                k_galerkin_sys<2, true><<<sys_grid(g0.c_sell_nb), kWG, 0, s>>>(g0, slab, b0, cs);
            } else {
                auto *slab = reinterpret_cast<float4 *>(G.aslab.p);
                k_a_slab<float4><<<gs, kWG, 0, s>>>(fnb, b0, nb, reinterpret_cast<const float4 *>(w.A32.p), slab);
                ++g_galerkin_launches[kGalSys2F32];
                k_galerkin_sys<2><<<sys_grid(g0.c_sell_nb), kWG, 0, s>>>(g0, slab, b0, cs);
            }
            if (l1) {
                ++g_galerkin_launches[kGalSys3];
                k_galerkin_sys<3><<<sys_grid(g1.c_sell_nb), kWG, 0, s>>>(g1, C.slab.p, b0, nullptr);
            }
        }
        l_first = l1 ? 2 : 1;
    }
    // the other levels: by gather entry where the lists allow it (ent_fits),
    // else per position
    for (size_t l = l_first; l + 1 < L; ++l) {
        AmgDevLevel &F = G.lv[l], &C = G.lv[l + 1];
        MOF_REQUIRE(l == 0 || F.packed, "a product's coarse source keeps no packed operator");
        const GalArgs g = gal_args(F, C, B);
        const bool ent = ent_fits(F);
        if (l == 0 && ent) {
            ++g_galerkin_launches[kGal0Ent];
            k_galerkin_ent<2><<<gal_grid(F.nggrp, kGalENS), kWG, 0, s>>>(g, F.nggrp, F.ggrp.p, A0h, fnb);
        } else if (l == 0) {
            ++g_galerkin_launches[kGal0Ns];
            k_galerkin_ns<2, kGalNS><<<gal_grid((C.sell_nb + kWG - 1) / kWG, kGalNS), kWG, 0, s>>>(
                g, w.A32.p, fnb, F.smoothed ? nullptr : A0h);
        } else if (ent) {
            if (F.nggrp > 0) {
                ++g_galerkin_launches[kGal3Ent];
                k_galerkin_ent<3><<<gal_grid(F.nggrp, kGalENS), kWG, 0, s>>>(g, F.nggrp, F.ggrp.p, F.A.p, F.npk);
            }
            if (F.nbig > 0) {
                ++g_galerkin_launches[kGal3Big];
                k_galerkin3_big<kGalBigNS><<<gal_grid(F.nbig, kGalBigNS), kWG, 0, s>>>(g, F.nbig, F.gbig.p, F.A.p,
                                                                                      F.npk);
            }
        } else {
            ++g_galerkin_launches[kGal3Ns];
            k_galerkin_ns<3, kGal3NS><<<gal_grid((C.sell_nb + kWG - 1) / kWG, kGal3NS), kWG, 0, s>>>(
                g, F.A.p, F.npk, nullptr);
        }
    }
    AmgDevLevel &Lc = G.lv[L - 1];
    k_coarse_inverse<<<dim3((unsigned)B), kInvWG, 0, s>>>(Lc.n, Lc.sell_off.p, Lc.sell_col.p, Lc.A.p,
                                                       Lc.sell_nb, G.cinv.p);
    MOF_HIP(hipGetLastError());
}

Lvl level_view(const AmgDevLevel &D) {
    Lvl v;
    v.n = D.n;
    v.sell_nb = D.sell_nb;
    v.sell_off = D.sell_off.p;
    v.sell_col = D.sell_col.p;
    v.A = D.A.p;
    v.Dh = reinterpret_cast<const uint4 *>(D.Dh.p);
    v.Dh22 = D.Dh22.p;
    v.Ah = D.Ah.n > 1 ? reinterpret_cast<const uint4 *>(D.Ah.p) : nullptr;
    v.Ah22 = D.Ah22.n > 1 ? D.Ah22.p : nullptr;
    v.b = D.b.p;
    v.x = D.x.p;
    v.r = D.r.p;
    v.y = D.y.p;
    v.agg = D.agg.p;
    v.mptr = D.mptr.p;
    v.mlist = D.mlist.p;
    v.apos = D.apos.p;
    v.Q = D.Q.p;
    v.Qm = D.Qm.p;
    v.pptr = D.pptr.p;
    v.pcol = D.pcol.p;
    v.rptr = D.rptr.p;
    v.rent = D.rent.p;
    v.rperm = D.rperm.n > 0 ? D.rperm.p : nullptr;
    return v;
}

void amg_vcycle(mof_mesh *m, int32_t B, const float *r0, float *z0, double *part_slot, int32_t nblk,
                const RedArgs &rd, hipStream_t s, bool zh, const int32_t *smap, int32_t nl, float *tap) {
    AmgDevice &G = *m->amg;
    Workspace &w = m->ws;
    const int32_t L = (int32_t)G.lv.size();
    const int32_t *sysi = w.sysi.p;
    const float om = G.omega;
    const float om1 = G.omega1;  // levels >= 1
    const MatH mat0 = level0_mat(m);
    Lvl v[kMaxLevels];
    // the launches cover nL systems: smap's (the PCG's tail iterations) or all B
    const int32_t nL = smap ? nl : B;
    const SysMap sm{smap, nL};
    for (int32_t l = 0; l < L; ++l) {
        v[l] = level_view(G.lv[l]);
        v[l].sm = sm;
    }
    // levels S.. run fused in k_subcycle
    int32_t S = 1;
    while (S < L - 1 && G.lv[S].n > kSubNodes) ++S;
    // tests only (mof_test_amg_vcycle; null in production): level 0's iterate
    // of all B systems copied to tap[k] (2 B N floats each) before the
    // in-place updates overwrite it -- stream-ordered copies between the
    // launches, which do not depend on them
    auto tap_x = [&](int k, const float *x, size_t words_per_vertex) {
        if (!tap) return;
        MOF_HIP(hipMemcpyAsync(tap + (size_t)k * 2 * B * v[0].n, x, sizeof(float) * words_per_vertex * B * v[0].n,
                               hipMemcpyDeviceToDevice, s));
    };
    tap_x(0, v[0].x, 1);
    // the fused tiny levels first .. L - 1 and the coarsest solve
    auto subcycle = [&](int32_t first) {
        SubArgs sa;
        sa.first = first;
        sa.last = L - 1;
        for (int32_t l = 0; l < L; ++l) sa.lv[l] = v[l];
        sa.cinv = G.cinv.p;
        sa.omega = om1;
        sa.sysi = sysi;
        k_subcycle<<<dim3((unsigned)nL), kSubWG, 0, s>>>(sa);
        ++g_vcycle_launches[kVcSubcycle];
    };
    // the cycle below level 0 from level 1's restricted b and pre-smoothed
    // x: down (residual, restriction + next pre-smooth), the fused tiny
    // levels, up (prolongation, post-smoothing into y)
    const bool xm2 = G.xm == 2;
    // b_{l+1} = P_l^T r_l and level l + 1's pre-smooth (the coarsest level has
    // none): tentative or smoothed P, level 0 (BSF = 2) or a coarse level
    auto launch_restrict = [&](int32_t l) {
        const AmgDevLevel &D = G.lv[l];
        const int32_t ns = D.smoothed ? kNSR : l == 0 ? kRestrS : 1;  // systems per workgroup
        ++g_vcycle_launches[D.smoothed ? (l == 0 ? kVcRestrict0Sa2 : kVcRestrict0Sa3)
                                       : (l == 0 ? kVcRestrict2 : kVcRestrict3)];
        (D.smoothed ? (l == 0 ? k_restrict0_sa<2> : k_restrict0_sa<3>) : (l == 0 ? k_restrict<2, kRestrS> : k_restrict<3>))
            <<<dim3(xcd_grid(D.ngrp, (nL + ns - 1) / ns, kGrpRestr)), kWG, 0, s>>>(v[l], v[l + 1], D.rgrp.p, D.ngrp,
                                                                                   l + 1 < L - 1, om1, sysi);
    };
    // x_l += P_l y_{l+1}; level 0 writes the corrected iterate in the xm format
    auto launch_prolong = [&](int32_t l) {
        const AmgDevLevel &D = G.lv[l];
        if (l > 0 && !D.smoothed) {
            ++g_vcycle_launches[kVcProlong3];
            k_prolong<<<grid2(v[l].n, nL), kWG, 0, s>>>(v[l], v[l + 1], sysi);
            return;
        }
        const int32_t ns = l > 0 ? kNS3 : D.smoothed ? kNSP : kProlS;  // systems per thread
        const int32_t nb = (v[l].n + kWG - 1) / kWG;
        ++g_vcycle_launches[l > 0 ? kVcProlong3Sa : (D.smoothed ? kVcProlong0SaX1 : kVcProlong0X1) + (xm2 ? 1 : 0)];
        (l > 0 ? k_prolong_sa<3, 0, kNS3>
               : D.smoothed ? (xm2 ? k_prolong_sa<2, 2, kNSP> : k_prolong_sa<2, 1, kNSP>)
                            : (xm2 ? k_prolong0<2> : k_prolong0<1>))
            <<<dim3(xcd_grid(nb, (nL + ns - 1) / ns, kGrpProl)), kWG, 0, s>>>(v[l], v[l + 1], nb, sysi);
    };
    auto coarse = [&]() {
        for (int32_t l = 1; l < S; ++l) {
            k_res3<<<grid2(v[l].n, nL), kWG, 0, s>>>(v[l], sysi);
            ++g_vcycle_launches[kVcRes3];
            launch_restrict(l);
        }
        subcycle(S);
        for (int32_t l = S - 1; l >= 1; --l) {
            launch_prolong(l);
            ++g_vcycle_launches[kVcPost3];
            k_post3<<<grid2(v[l].n, nL), kWG, 0, s>>>(v[l], om1, sysi);
        }
    };
    // down at level 0: residual of the pre-smoothed x, restriction (+ level
    // 1's pre-smooth)
    {
        if (G.bsw_n > 0) launch_bsweep<false>(G, sm, r0, v[0].x, om, sysi, s);
        tap_x(1, v[0].x, 1);
        ++g_vcycle_launches[mat0.sell_idx ? kVcRes0Pk : kVcRes0];
        const dim3 gr(xcd_grid(nblk, (nL + kRes0NS - 1) / kRes0NS, kGrpSmooth > kRes0NS ? kGrpSmooth / kRes0NS : 1));
        (mat0.sell_idx ? k_res0_ns<kRes0NS, true> : k_res0_ns<kRes0NS, false>)<<<gr, kWG, 0, s>>>(
            v[0].n, nblk, sm, mat0, r0, v[0].x, G.lv[0].smoothed ? nullptr : v[0].apos, sysi, v[0].r);
        launch_restrict(0);
    }
    if (S == 1)  // level 1 is already one of the fused tiny levels
        subcycle(1);
    else
        coarse();
    // up at level 0: coarse correction, post-smooth, on the corrected iterate
    // -- float2 in y (xm = 2), or the x0 word in place
    {
        float *x = xm2 ? v[0].y : v[0].x;
        const size_t words = xm2 ? 2 : 1;  // per vertex
        const bool packed = mat0.sell_idx != nullptr;
        launch_prolong(0);
        tap_x(2, x, words);
        if (G.bsw_n > 0) (xm2 ? launch_bsweep<true> : launch_bsweep<false>)(G, sm, r0, x, om, sysi, s);
        tap_x(3, x, words);
        auto post0 = [&](auto xm) {
            launch_post0<decltype(xm)::value>(zh, packed, nblk, nL, s, v[0].n, nblk, B, sm, mat0, r0, x, om, sysi, z0,
                                              part_slot, rd);
        };
        if (xm2)
            post0(std::integral_constant<int, 2>());
        else
            post0(std::integral_constant<int, 1>());
    }
    MOF_HIP(hipGetLastError());
}

void amg_destroy(AmgDevice *g) { delete g; }

float amg_set_omega(mof_mesh *m, float omega) {
    if (!m->amg) return 0.f;
    const float old = m->amg->omega;
    m->amg->omega = omega;
    return old;
}

int32_t amg_levels(const mof_mesh *m) { return m->amg && m->amg->built ? (int32_t)m->amg->lv.size() : 0; }
int32_t amg_capacity(const mof_mesh *m) { return m->amg && m->amg->built ? m->amg->cap : 0; }

namespace {
struct DeviceGuard {
    int prev = 0;
    explicit DeviceGuard(int d) {
        (void)hipGetDevice(&prev);
        MOF_HIP(hipSetDevice(d));
    }
    ~DeviceGuard() { (void)hipSetDevice(prev); }
};

// tests only (mof_test_amg_vcycle): the level-0 pre-smoothing x0 = w D^-1 r
// of every system, the expression of k_pcg_init / k_pcg_update
__global__ __launch_bounds__(kWG) void k_test_presmooth(int32_t N, const uint2 *__restrict__ dA, int64_t dA_nb,
                                                        const int32_t *__restrict__ dA_off,
                                                        const float *__restrict__ r, float omega,
                                                        float *__restrict__ x0) {
    const int32_t i = blockIdx.x * kWG + threadIdx.x, b = blockIdx.y;
    const int64_t vi = (int64_t)b * N + min(i, N - 1);
    const float2 ri = reinterpret_cast<const float2 *>(r)[vi];
    const float2 d = bf16_diag_solve(bf16_diag_block(dA, dA_nb, dA_off, b, min(i, N - 1)), ri.x, ri.y);
    if (i < N) st_x0(x0, vi, omega * d.x, omega * d.y);
}

// the handle's per-system flags replaced for one test cycle and put back
struct SysiSwap {
    int32_t *dev;
    std::vector<int32_t> saved;
    SysiSwap(int32_t *d, int32_t B, const uint8_t *retired_mask) : dev(d), saved((size_t)B * kSysStride) {
        MOF_HIP(hipMemcpy(saved.data(), dev, saved.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        std::vector<int32_t> now(saved.size(), 0);
        for (int32_t b = 0; b < B; ++b) {
            now[(size_t)b * kSysStride + SI_CONV] = -1;
            now[(size_t)b * kSysStride + SI_ACTIVE] = !(retired_mask && retired_mask[b]);
        }
        MOF_HIP(hipMemcpy(dev, now.data(), now.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    ~SysiSwap() { (void)hipMemcpy(dev, saved.data(), saved.size() * sizeof(int32_t), hipMemcpyHostToDevice); }
};
}  // namespace

}  // namespace mof

// ---- test hooks (include/mof.h) ------------------------------------------------

extern "C" {

int mof_test_amg_levels(mof_mesh *m, int32_t level, int32_t *n_levels, int64_t *sizes, float *omegas,
                        int32_t *sell_off, int32_t *sell_col, int32_t *sell_row, int32_t *diag_pos, uint8_t *dead,
                        int32_t *twin, int32_t *mirror, int32_t *agg, int32_t *pptr, int32_t *pcol, float *Q,
                        int32_t *gptr, int32_t *gent) {
    return mof_io_guard([&] {
        MOF_REQUIRE(m && n_levels, "NULL argument");
        mof::mesh_join_prep(m);
        const mof::AmgDevice *G = m->amg;
        MOF_REQUIRE(G && G->built && G->H && G->lv.size() >= 2 && G->H->levels.size() == G->lv.size(),
                    "the handle has no built multigrid");
        const mof::AmgHierarchy &H = *G->H;
        *n_levels = (int32_t)H.levels.size();
        if (omegas) {
            omegas[0] = G->omega;
            omegas[1] = G->omega1;
        }
        if (level < 0) return;  // the level count alone
        MOF_REQUIRE(level < *n_levels, "no such level");
        const mof::AmgLevel &L = H.levels[level];
        // level 0: the mesh's own SELL layout (the hierarchy's level 0 only
        // carries the adjacency) and the mirror table on the device
        const std::vector<int32_t> &off = level == 0 ? m->pat.sell_off : L.sell_off;
        const std::vector<int32_t> &col = level == 0 ? m->pat.sell_col : L.sell_col;
        const std::vector<int32_t> &dpos = level == 0 ? m->pat.diag_pos : L.diag_pos;
        const int64_t nb = off.empty() ? 0 : off.back();
        MOF_REQUIRE(nb == G->lv[level].sell_nb && L.n == G->lv[level].n, "host and device levels disagree");
        if (sizes) {
            const int64_t v[16] = {L.n,
                                   L.bs,
                                   nb,
                                   (int64_t)off.size(),
                                   L.smoothed,
                                   (int64_t)L.agg.size(),
                                   (int64_t)L.pptr.size(),
                                   (int64_t)L.pcol.size(),
                                   (int64_t)L.Q.size(),
                                   (int64_t)L.gptr.size(),
                                   (int64_t)L.gent.size(),
                                   G->regular,
                                   level == 0 && m->sym_reads,
                                   G->nc,
                                   G->cap,
                                   (G->lv[level].Ah.n > 1 ? 1 : 0) | (G->lv[level].packed ? 2 : 0)};
            std::copy(v, v + 16, sizes);
        }
        auto put = [](auto *dst, const auto &src) {
            if (dst) std::copy(src.begin(), src.end(), dst);
        };
        put(sell_off, off);
        put(sell_col, col);
        put(diag_pos, dpos);
        if (sell_row) {
            if (level == 0)
                for (size_t s = 0; s + 1 < off.size(); ++s)
                    for (int64_t q = off[s]; q < off[s + 1]; ++q)
                        sell_row[q] = (int32_t)(s * mof::kSlice + (q - off[s]) % mof::kSlice);
            else
                put(sell_row, L.sell_row);
        }
        if (level > 0) {
            put(dead, L.dead);
            if (twin) {  // as amg_build uploads it: each upper block's lower twin, -1 elsewhere
                std::fill(twin, twin + nb, -1);
                for (size_t k = 0; k < L.low.size(); ++k) twin[L.twin[k]] = L.low[k];
            }
        } else if (mirror) {
            MOF_REQUIRE((int64_t)H.mirror.size() == nb, "the hierarchy keeps no level-0 mirror table");
            put(mirror, H.mirror);
        }
        put(agg, L.agg);
        put(pptr, L.pptr);
        put(pcol, L.pcol);
        put(Q, L.Q);
        put(gptr, L.gptr);
        put(gent, L.gent);
    });
}

int mof_test_amg_readback(mof_mesh *m, int32_t level, int32_t system, float *A, uint32_t *Dh, uint16_t *Dh22,
                          uint32_t *Ah, uint16_t *Ah22, float *cinv) {
    return mof_io_guard([&] {
        MOF_REQUIRE(m, "mesh is NULL");
        mof::mesh_join_prep(m);
        mof::AmgDevice *G = m->amg;
        MOF_REQUIRE(G && G->built && G->lv.size() >= 2, "the handle has no built multigrid");
        MOF_REQUIRE(level >= 1 && level < (int32_t)G->lv.size(), "no such coarse level");
        MOF_REQUIRE(system >= 0 && system < G->cap, "no multigrid storage for that system");
        mof::AmgDevLevel &D = G->lv[level];
        const bool sweep = D.Ah.n > 1, last = level + 1 == (int32_t)G->lv.size();
        MOF_REQUIRE(sweep || !(Ah || Ah22), "that level keeps no sweep copy");
        MOF_REQUIRE(last || !cinv, "cinv belongs to the coarsest level");
        mof::DeviceGuard dg(m->device);
        MOF_HIP(hipStreamSynchronize(m->stream));
        const size_t b = (size_t)system, nb = (size_t)D.sell_nb, n = (size_t)D.n, nc = (size_t)G->nc;
        auto get = [&](auto *dst, const auto &src, size_t per) {
            if (!dst) return;
            MOF_REQUIRE(src.n >= per * (b + 1), "multigrid storage smaller than its capacity");
            MOF_HIP(hipMemcpy(dst, src.p + per * b, per * sizeof(*dst), hipMemcpyDeviceToHost));
        };
        if (A && D.packed) {
            // the packed blocks widened to [sell_nb][12]: each lower block is its upper twin transposed
            MOF_REQUIRE(G->H && G->H->levels.size() == G->lv.size(), "the handle keeps no host hierarchy");
            const mof::AmgLevel &HL = G->H->levels[level];
            const size_t npk = (size_t)D.npk;
            MOF_REQUIRE(D.A.n >= mof::kB9 * npk * (b + 1), "multigrid storage smaller than its capacity");
            std::vector<float> pa(mof::kB9 * npk);
            MOF_HIP(hipMemcpy(pa.data(), D.A.p + mof::kB9 * npk * b, sizeof(float) * pa.size(), hipMemcpyDeviceToHost));
            std::fill(A, A + mof::kB3 * nb, 0.f);
            auto blk = [&](size_t pos, int32_t pi, bool tr) {
                for (int r = 0; r < 3; ++r)
                    for (int c = 0; c < 3; ++c) A[mof::kB3 * pos + 4 * r + c] = pa[mof::kB9 * pi + (tr ? 3 * c + r : 3 * r + c)];
            };
            for (size_t pos = 0; pos < nb; ++pos)
                if (HL.pk[pos] >= 0) blk(pos, HL.pk[pos], false);
            for (size_t k = 0; k < HL.low.size(); ++k) blk((size_t)HL.low[k], HL.pk[HL.twin[k]], true);
        } else {
            get(A, D.A, mof::kB3 * nb);
        }
        get(Dh, D.Dh, 4 * n);
        get(Dh22, D.Dh22, n);
        get(Ah, D.Ah, mof::kAhWords * nb);
        get(Ah22, D.Ah22, mof::kAh22Words * nb);
        get(cinv, G->cinv, nc * nc);
    });
}

int mof_test_force_galerkin_ns(int32_t on) {
    mof::g_force_galerkin_ns.store(on != 0);
    return MOF_OK;
}

int mof_test_galerkin_launches(int64_t *counts) {
    return mof_io_guard([&] {
        MOF_REQUIRE(counts, "NULL argument");
        for (int k = 0; k < mof::kGalKernels; ++k) counts[k] = mof::g_galerkin_launches[k].load();
    });
}

int mof_test_vcycle_launches(int64_t *counts) {
    return mof_io_guard([&] {
        MOF_REQUIRE(counts, "NULL argument");
        for (int k = 0; k < mof::kVcKernels; ++k) counts[k] = mof::g_vcycle_launches[k].load();
    });
}

int mof_test_amg_vcycle_tables(mof_mesh *m, int32_t level, int32_t system, int64_t *sizes, int32_t *apos,
                               int32_t *mptr, int32_t *mlist, int32_t *rptr, int32_t *rent, int32_t *bsw_rows,
                               int32_t *bsw_bsrc, uint32_t *bsw_A) {
    return mof_io_guard([&] {
        MOF_REQUIRE(m, "mesh is NULL");
        mof::mesh_join_prep(m);
        mof::AmgDevice *G = m->amg;
        MOF_REQUIRE(G && G->built && G->H && G->lv.size() >= 2 && G->H->levels.size() == G->lv.size(),
                    "the handle has no built multigrid");
        const int32_t L = (int32_t)G->lv.size();
        MOF_REQUIRE(level >= 0 && level < L, "no such level");
        const mof::AmgLevel &H = G->H->levels[level];
        int32_t S = 1;
        while (S < L - 1 && G->lv[S].n > mof::kSubNodes) ++S;
        if (sizes) {
            const int64_t v[12] = {(int64_t)H.apos.size(), (int64_t)H.mptr.size(), (int64_t)H.mlist.size(),
                                   (int64_t)H.rptr.size(), (int64_t)H.rent.size(), G->xm, G->regular, S,
                                   G->bsw_n, G->bsw_sweeps, G->bsw_nslot, m->ws.nblk};
            std::copy(v, v + 12, sizes);
        }
        auto put = [](int32_t *dst, const std::vector<int32_t> &src) {
            if (dst) std::copy(src.begin(), src.end(), dst);
        };
        put(apos, H.apos);
        put(mptr, H.mptr);
        put(mlist, H.mlist);
        put(rptr, H.rptr);
        put(rent, H.rent);
        if (!(bsw_rows || bsw_bsrc || bsw_A)) return;
        MOF_REQUIRE(G->bsw_n > 0, "the handle runs no boundary sweeps");
        MOF_REQUIRE(system >= 0 && system < G->cap, "no multigrid storage for that system");
        mof::DeviceGuard dg(m->device);
        MOF_HIP(hipStreamSynchronize(m->stream));
        if (bsw_rows)
            MOF_HIP(hipMemcpy(bsw_rows, G->bsw_rows.p, sizeof(int32_t) * G->bsw_n, hipMemcpyDeviceToHost));
        if (bsw_bsrc)
            MOF_HIP(hipMemcpy(bsw_bsrc, G->bsw_bsrc.p, sizeof(int32_t) * G->bsw_nslot, hipMemcpyDeviceToHost));
        if (bsw_A)
            MOF_HIP(hipMemcpy(bsw_A, G->bsw_A.p + (size_t)2 * G->bsw_nslot * system,
                              sizeof(uint32_t) * 2 * G->bsw_nslot, hipMemcpyDeviceToHost));
    });
}

int mof_test_amg_vcycle(mof_mesh *m, int32_t B, const float *r, const int32_t *smap, int32_t nl,
                        const uint8_t *retired, int32_t zh, int32_t tap, const uint32_t *sentinel, uint32_t *z,
                        double *rz, int32_t nsys, const int32_t *systems, uint32_t *r1, uint32_t *taps,
                        float *coarse, int32_t *meta) {
    return mof_io_guard([&] {
        MOF_REQUIRE(m && r && z, "NULL argument");
        mof::mesh_join_prep(m);
        mof::AmgDevice *Gp = m->amg;
        MOF_REQUIRE(Gp && Gp->built && Gp->lv.size() >= 2, "the handle has no built multigrid");
        mof::AmgDevice &G = *Gp;
        mof::Workspace &w = m->ws;
        MOF_REQUIRE(B >= 1 && B <= G.cap && B <= w.cap, "the handle's last batch had fewer systems");
        MOF_REQUIRE(!smap || (nl >= 1 && nl <= B), "bad system map");
        for (int32_t l = 0; smap && l < nl; ++l) MOF_REQUIRE(smap[l] >= 0 && smap[l] < B, "bad system map");
        for (int32_t k = 0; k < nsys; ++k)
            MOF_REQUIRE(systems && systems[k] >= 0 && systems[k] < B, "bad system to read back");
        // a decomposed part: the cycle as pcg() runs it on the parts (float2 z, the sums over the owned rows)
        const bool zhb = zh < 0 ? (G.regular && m->n_own == m->N) : zh != 0;
        const int32_t L = (int32_t)G.lv.size();
        const size_t N = (size_t)m->N, nv = N * B;
        mof::DeviceGuard dg(m->device);
        hipStream_t s = m->stream;
        MOF_HIP(hipStreamSynchronize(s));
        float *rv = reinterpret_cast<float *>(w.vr.p), *zv = reinterpret_cast<float *>(w.vz.p);
        MOF_HIP(hipMemcpy(rv, r, sizeof(float) * 2 * nv, hipMemcpyHostToDevice));
        mof::SysiSwap swap(w.sysi.p, B, retired);
        const mof::AmgFine f = mof::amg_fine(m);
        mof::k_test_presmooth<<<mof::grid2((int64_t)N, B), mof::kWG, 0, s>>>(
            (int32_t)N, static_cast<const uint2 *>(f.A0h), f.sell_nb, f.sell_off, rv, f.omega, f.x0);
        auto fill = [&](void *p, size_t words) {
            if (sentinel) MOF_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p), (int)*sentinel, words, s));
        };
        fill(zv, 2 * nv);
        fill(G.lv[0].r.p, nv);
        if (G.xm == 2) fill(G.lv[0].y.p, 2 * nv);
        for (int32_t l = 1; l < L; ++l) {
            mof::AmgDevLevel &D = G.lv[l];
            for (mof::DevArray<float> *a : {&D.b, &D.x, &D.r, &D.y}) fill(a->p, (size_t)mof::kV3 * D.n * B);
        }
        mof::DevArray<int32_t> dmap;
        if (smap) {
            dmap.alloc((size_t)nl);
            MOF_HIP(hipMemcpyAsync(dmap.p, smap, sizeof(int32_t) * nl, hipMemcpyHostToDevice, s));
        }
        mof::DevArray<float> dtap;
        if (tap) {
            dtap.alloc(8 * nv);
            dtap.zero(s);
        }
        const size_t nrec = (size_t)2 * B * w.nblk;
        MOF_REQUIRE(w.part_rzrr.n >= nrec, "partial records smaller than the batch");
        MOF_HIP(hipMemsetAsync(w.part_rzrr.p, 0, sizeof(double) * nrec, s));
        mof::amg_vcycle(m, B, rv, zv, w.part_rzrr.p, w.nblk, mof::RedArgs{1, 0, w.nblk, m->n_own}, s, zhb,
                        smap ? dmap.p : nullptr, nl, tap ? dtap.p : nullptr);
        MOF_HIP(hipStreamSynchronize(s));
        MOF_HIP(hipMemcpy(z, zv, sizeof(uint32_t) * (zhb ? 1 : 2) * nv, hipMemcpyDeviceToHost));
        if (rz) {
            std::vector<double> part(nrec);
            MOF_HIP(hipMemcpy(part.data(), w.part_rzrr.p, sizeof(double) * nrec, hipMemcpyDeviceToHost));
            for (int32_t b = 0; b < B; ++b) {
                double t = 0.0;
                for (int32_t k = 0; k < w.nblk; ++k) t += part[2 * ((size_t)b * w.nblk + k)];
                rz[b] = t;
            }
        }
        if (meta) {
            int32_t S = 1;
            while (S < L - 1 && G.lv[S].n > mof::kSubNodes) ++S;
            const int32_t v[4] = {zhb, G.xm, S, w.nblk};
            std::copy(v, v + 4, meta);
        }
        size_t per = 0;
        for (int32_t l = 1; l < L; ++l) per += (size_t)16 * G.lv[l].n;
        std::vector<float> row;
        for (int32_t k = 0; k < nsys; ++k) {
            const size_t b = (size_t)systems[k];
            if (r1)
                MOF_HIP(hipMemcpy(r1 + k * N, G.lv[0].r.p + b * N, sizeof(uint32_t) * N, hipMemcpyDeviceToHost));
            // a tap's words of system b: N (the x0 format) or 2 N (float2) from its 2 B N
            for (int t = 0; t < 4 && taps && tap; ++t) {
                const size_t wpv = t >= 2 && G.xm == 2 ? 2 : 1;
                MOF_HIP(hipMemcpy(taps + (4 * k + t) * 2 * N, dtap.p + t * 2 * nv + b * wpv * N,
                                  sizeof(uint32_t) * wpv * N, hipMemcpyDeviceToHost));
            }
            float *o = coarse ? coarse + k * per : nullptr;
            for (int32_t l = 1; l < L && o; ++l) {
                mof::AmgDevLevel &D = G.lv[l];
                // the stored 12-byte rows, widened to the hook's [n][4]: the fourth word is 0, or
                // the sentinel on a row that still holds it in all three words
                const size_t n3 = (size_t)mof::kV3 * D.n;
                row.resize(n3);
                for (mof::DevArray<float> *a : {&D.b, &D.x, &D.r, &D.y}) {
                    MOF_HIP(hipMemcpy(row.data(), a->p + b * n3, sizeof(float) * n3, hipMemcpyDeviceToHost));
                    for (size_t i = 0; i < (size_t)D.n; ++i, o += 4) {
                        uint32_t wd[4] = {0u, 0u, 0u, 0u};
                        std::memcpy(wd, &row[mof::kV3 * i], sizeof(float) * mof::kV3);
                        if (sentinel && wd[0] == *sentinel && wd[1] == *sentinel && wd[2] == *sentinel) wd[3] = *sentinel;
                        std::memcpy(o, wd, sizeof(wd));
                    }
                }
            }
        }
    });
}

}  // extern "C"
