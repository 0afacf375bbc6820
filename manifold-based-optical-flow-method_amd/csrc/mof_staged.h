// mof_staged.h -- what the slice-staged row kernels share (k_residual_lds,
// mof_pcg.hip; k_assemble_lds, mof_assemble.hip): the operator's argument
// block, the one launch, and the LDS planes both stage and read alike. The
// size rule, per-mesh state and test hooks of a kind: mof_internal.h.
#pragma once
#include "mof_internal.h"
#include "mof_rowkern.h"

namespace mof {
namespace {

// The operator of B systems sharing a mesh.
template <typename V>
struct OpArgs {
    int32_t N, M;
    const int32_t *sell_off, *sell_col;  // a2 blocks, SELL-64
    const V *a2s;                        // [sell_nb][4] lambda * a2
    const int32_t *tsell_off;            // vertex -> incident triangles, SELL-64
    const int4 *tinc;                    // {T, corner, vertex of corner+1, vertex of corner+2}
    const V *w12;                        // [M+1] A_T / 12 (slot M = 0)
    const V *u;                          // [B][M+1][6] u_T per system (slot M = 0), or null:
    // u re-formed from the timestep's I row as k_tri_step forms it
    const double *gw, *e;                // [M][9] hat gradients, [N][6] tangent bases
    const double *I0;                    // [B][ldI] I_k rows (internal order)
    int64_t ldI;
};

template <typename V>
OpArgs<V> make_op(mof_mesh *m, const V *a2s, const V *w12, const V *u) {
    return OpArgs<V>{m->N, m->M, m->sell_off.p, m->sell_col.p, a2s, m->tsell_off.p,
                     reinterpret_cast<const int4 *>(m->tinc.p), w12, u, m->gw.p, m->e.p, m->ws.J0, m->N};
}

// One staged launch over (slice, chunk of W TRIPS units): a workgroup is one
// SELL-64 slice x W waves, and a wave takes TRIPS of the launch's `units`
// (system pairs or systems). A small mesh or batch -- fewer than `fill`
// workgroups -- takes kern1, the one-trip instance, instead, so the launch
// still fills the CUs; a system's bits do not depend on the split. The dynamic-
// LDS limit is raised once per process and device to the kind's fixed cap, never
// to a mesh's own size (a later, wider mesh would otherwise launch past it).
template <int W, int TRIPS, typename K, typename... Args>
void launch_staged(K kern, K kern1, int64_t fill, int32_t grp, int32_t units, const mof_mesh *m,
                   const StagedKind &kind, const StagedState &st, StagedHooks &hooks, LdsLimit &limit,
                   hipStream_t s, Args... args) {
    raise_lds_limit(limit, m->device, {reinterpret_cast<const void *>(kern), reinterpret_cast<const void *>(kern1)},
                    kind.lds_cap);
    const int32_t nsl = m->pat.nslices;
    int32_t nchunk = (units + W * TRIPS - 1) / (W * TRIPS);
    const bool one = (int64_t)nsl * nchunk < fill && !hooks.force_trips.load();
    if (one) nchunk = (units + W - 1) / W;
    MOF_REQUIRE((kind.max_w == 0 || m->pat.max_w <= kind.max_w) && st.bytes <= kind.lds_cap,
                "staged launch: mesh not eligible");
    const unsigned grid = xcd_grid(nsl, nchunk, grp);
    MOF_REQUIRE((int64_t)grid * 64 * W < ((int64_t)1 << 32), "launch grid past 2^32 work-items");
    hooks.launches[one ? 1 : 2]++;
    (one ? kern1 : kern)<<<dim3(grid), 64 * W, (size_t)st.bytes, s>>>(args...);
}

// ---- device pieces. Planes are lane-major and 16 bytes wide: plane p of a
// slice holds lane l's double2 at [64 p + l], so a wave's ds_read_b128 of a
// plane is 1 KiB of consecutive LDS.

// Slice s of the two SELL-64 tables: its first a2 position o and a2 slots wa,
// its first incidence position to and incidence slots wt.
struct SliceView {
    int32_t o, wa, to, wt;
};
__device__ __forceinline__ SliceView slice_view(const int32_t *sell_off, const int32_t *tsell_off, int32_t s) {
    const int32_t o = sell_off[s], to = tsell_off[s];
    return SliceView{o, (sell_off[s + 1] - o) >> 6, to, (tsell_off[s + 1] - to) >> 6};
}

// E: the three planes of the slice's rows' tangent bases (lanes past row
// N - 1 of the last slice stage row N - 1's), by all NT threads.
template <int NT>
__device__ __forceinline__ void stage_e(double2 *E, const double *e, int32_t s, int32_t N) {
    for (int32_t q = threadIdx.x; q < 3 * 64; q += NT) {
        const int32_t k = q >> 6, ll = q & 63;
        E[q] = ld2(e + 6 * (int64_t)min(64 * s + ll, N - 1) + 2 * k);
    }
}
__device__ __forceinline__ void ld_e(const double2 *E, int32_t l, double (&ei)[6]) {
    const double2 e0 = E[l], e1 = E[64 + l], e2 = E[128 + l];
    ei[0] = e0.x; ei[1] = e0.y; ei[2] = e1.x; ei[3] = e1.y; ei[4] = e2.x; ei[5] = e2.y;
}

// Incidence slot t of a slice takes STRIDE planes (12 in the residual, 7 in
// the assembly); the first six are the same in both: {tinc record | g0 g1 |
// g2 g3 | g4 g5 | g6 g7 | g8 tail}, g the triangle's nine hat gradients (a
// padding incidence, T = M, stages triangle M - 1's) and tail the kernel's own
// per-triangle double, tail[ti] (A_T / 12 in the residual, A_T in the assembly),
// loaded after the gradients. Part 0 stages planes 0-3 (the record last: with
// like ends the two parts' last planes are merged into 8-byte loads and writes),
// part 1 planes 4-5. Returns the slot's first plane at lane ll.
template <int STRIDE>
__device__ __forceinline__ double2 *stage_inc_geo(double2 *INC, int32_t t, int32_t ll, int32_t part, int4 rec,
                                                  const double *gw, int32_t M, const double *tail, int64_t ti) {
    double2 *P = INC + (STRIDE * t) * 64 + ll;
    const double *g = gw + 9 * (int64_t)min(rec.x, M - 1);
    if (part == 0) {
        P[1 * 64] = make_double2(g[0], g[1]);
        P[2 * 64] = make_double2(g[2], g[3]);
        P[3 * 64] = make_double2(g[4], g[5]);
        *reinterpret_cast<int4 *>(P) = rec;
    } else if (part == 1) {
        P[4 * 64] = make_double2(g[6], g[7]);
        P[5 * 64] = make_double2(g[8], tail[ti]);
    }
    return P;
}
// Read back by lane l: the record first (the kernel issues its global gathers
// at the record's vertices next), then the gradients and the tail.
template <int STRIDE>
__device__ __forceinline__ const double2 *ld_inc_rec(const double2 *INC, int32_t t, int32_t l, int4 &rec) {
    const double2 *P = INC + (STRIDE * t) * 64 + l;
    rec = *reinterpret_cast<const int4 *>(P);
    return P;
}
__device__ __forceinline__ void ld_inc_geo(const double2 *P, double (&g)[9], double &tail) {
    const double2 g01 = P[1 * 64], g23 = P[2 * 64], g45 = P[3 * 64], g67 = P[4 * 64], g8t = P[5 * 64];
    g[0] = g01.x; g[1] = g01.y; g[2] = g23.x; g[3] = g23.y; g[4] = g45.x; g[5] = g45.y;
    g[6] = g67.x; g[7] = g67.y; g[8] = g8t.x; tail = g8t.y;
}

}  // namespace
}  // namespace mof
