// mof_winding_host.cpp -- the host half of the winding numbers
// (mof_winding.hip): ring membership. Ring l of a centre is the set of
// vertices at edge distance exactly l + 1 from it (pyvista's
// point_neighbors_levels): an integer breadth-first search over the handle's
// vertex adjacency, one stamp array per host thread, centres dealt out in
// blocks. The polar order within a ring is the device's work.
#include <algorithm>
#include <thread>

#include "mof_internal.h"

namespace mof {

namespace {

// host threads: MOF_IO_THREADS, else OMP_NUM_THREADS (at most 16), else 4 --
// never the host's core count, which on a shared host is not the process's
// share -- and never more than one per 16 centres
int32_t bfs_threads(int32_t C) {
    int32_t t = knob_threads(16);
    if (t <= 0) t = 4;
    return std::max(1, std::min(t, C / 16));
}

struct CentreRings {
    std::vector<int32_t> vtx;  // the rings one after the other
    std::vector<int32_t> end;  // (L) end of ring l in vtx
};

// stamp[v] == tag: v has been reached from this centre
void bfs_one(const Pattern &pat, int32_t c, int32_t L, std::vector<int32_t> &stamp, int32_t tag, CentreRings &out) {
    out.vtx.clear();
    out.end.assign((size_t)L, 0);
    stamp[c] = tag;
    size_t f0 = 0, f1 = 0;  // the frontier is vtx[f0, f1), the centre itself for ring 0
    for (int32_t l = 0; l < L; ++l) {
        const size_t before = out.vtx.size();
        auto visit = [&](int32_t i) {
            for (int32_t q = pat.vptr[i]; q < pat.vptr[i + 1]; ++q) {
                const int32_t j = pat.vcol[q];
                if (stamp[j] != tag) {
                    stamp[j] = tag;
                    out.vtx.push_back(j);
                }
            }
        };
        if (l == 0)
            visit(c);
        else
            for (size_t p = f0; p < f1; ++p) visit(out.vtx[p]);
        f0 = before;
        f1 = out.vtx.size();
        for (int32_t r = l; r < L; ++r) out.end[r] = (int32_t)f1;
        if (f1 == f0) break;  // exhausted: the later rings stay empty
    }
}

}  // namespace

void wind_bfs(const Pattern &pat, const int32_t *centres, int32_t C, int32_t L, std::vector<int64_t> &off,
              std::vector<int32_t> &vtx) {
    std::vector<CentreRings> rings((size_t)C);
    const int32_t T = bfs_threads(C);
    auto work = [&](int32_t t) {
        std::vector<int32_t> stamp((size_t)pat.N, -1);
        for (int32_t q = t; q < C; q += T) bfs_one(pat, centres[q], L, stamp, q, rings[q]);
    };
    if (T == 1) {
        work(0);
    } else {
        std::vector<std::thread> pool;
        for (int32_t t = 0; t < T; ++t) pool.emplace_back(work, t);
        for (auto &th : pool) th.join();
    }
    off.assign((size_t)C * (L + 1), 0);
    int64_t tot = 0;
    for (int32_t q = 0; q < C; ++q) {
        int64_t *o = off.data() + (size_t)q * (L + 1);
        o[0] = tot;
        for (int32_t l = 0; l < L; ++l) o[l + 1] = tot + rings[q].end[l];
        tot += (int64_t)rings[q].vtx.size();
    }
    vtx.resize((size_t)tot);
    for (int32_t q = 0; q < C; ++q)
        std::copy(rings[q].vtx.begin(), rings[q].vtx.end(), vtx.begin() + off[(size_t)q * (L + 1)]);
}

}  // namespace mof
