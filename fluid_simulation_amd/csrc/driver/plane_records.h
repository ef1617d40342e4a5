// driver/plane_records.h -- per-plane records on their way to the host: how the forces, the solve residuals and the probes
// bring every slab's records together and add them up in one order.
#pragma once
#include "common.h"
#include "../forces.h"

namespace {

// Every rank's plane records (`mine`: `blocks` blocks of g.D records each) -> `all`: rank r's blocks at r * mine.size()
// (a slab's planes follow the lower slabs' planes).  Collective on slab handles; the host holds everything afterwards.
// `what`: "obstacle forces" / "solve residuals" (the records of both travel the same way)
template <class T>
int gather_plane_records(Engine<T>& e, const std::vector<double>& mine, std::vector<double>& all, const char* what)
{
    fs_sim* const S = e.S;
    if (!S->comm.active()) { all = mine; return FS_OK; }
    if (S->comm.null_transport) return fail(FS_EINVAL, "%s need the other slabs' planes; the FSNULL transport carries none", what);
    all.assign(mine.size() * (size_t)S->comm.nranks, 0.0);
    if (mine.empty()) return FS_OK;
    return e.comm_op([&](hipStream_t st) { return S->comm.allgather_host(st, mine.data(), all.data(), mine.size() * sizeof(double), e.g, S->D); },
                     "gather of the plane records");
}

// Sum of the records of global planes 1..D in increasing z, in fp64: `rec(r, zl)` = record of local plane zl of rank r.
// Single-GPU and slab handles add the same numbers in the same order.
// Records of `ncols` columns; column `maxcol` (if any) is a maximum, not a sum.
template <class F>
void combine_planes(const fs_sim* S, const fs::GridDesc& g, F&& rec, double* out, int ncols = fs::FORCE_REC, int maxcol = -1)
{
    const int nr = S->comm.active() ? S->comm.nranks : 1;
    for (int k = 0; k < ncols; ++k) out[k] = 0.0;
    for (int r = 0; r < nr; ++r)
        for (int zl = 0; zl < g.D; ++zl) {
            const double* q = rec(r, zl);
            for (int k = 0; k < ncols; ++k) out[k] = (k == maxcol) ? std::fmax(out[k], q[k]) : out[k] + q[k];
        }
}

}  // namespace
