// driver/confine.h -- vorticity confinement (csrc/confine.h; beyond the reference)
#pragma once
#include "common.h"
#include "../confine.h"

namespace {

template <class T>
struct Confine {
    explicit Confine(Engine<T>& e_) : eng(e_), S(e_.S), g(e_.g), arr(e_.arr), slot(e_.slot), flags(e_.flags) {}

    // One pass of strength eps > 0 over the velocities as they are: out of place into three pool arrays, which become the
    // velocities (the kernel also does what set_bounds(1 / 2 / 3) would do afterwards).  One launch.
    int pass(const char* who, double eps)
    {
        if (S->comm.active()) return fail(FS_EINVAL, "%s: vorticity confinement needs a single GPU handle (its stencil reaches two planes into the other slabs)", who);
        int rc = eng.ensure_flags();
        if (rc) return rc;
        const int V[3] = { FS_VX, FS_VY, FS_VZ };
        for (int f : V)
            if ((rc = eng.unalias(f))) return rc;
        int res[3] = { -1, -1, -1 };
        for (int k = 0; k < 3; ++k)
            if ((res[k] = eng.acquire()) < 0) {
                for (int j = 0; j < k; ++j) eng.held[res[j]] = false;
                return fail(FS_ENOMEM, "array pool exhausted");
            }
        const double k = (double)S->dt * eps;
        {
            ScopedSpan sp(S, FAM_CONFINE);
            fs::launch_confine<T>(S->stream, g, arr[slot[FS_VX]], arr[slot[FS_VY]], arr[slot[FS_VZ]], flags, arr[res[0]], arr[res[1]],
                                  arr[res[2]], k);
        }
        for (int a = 0; a < 3; ++a) eng.adopt(V[a], res[a]);
        ++S->n_confine;
        return FS_OK;
    }
    int vorticity(double eps)
    {
        if (!(eps >= 0.0) || !std::isfinite(eps)) return fail(FS_EINVAL, "fs_confine_vorticity: epsilon must be finite and >= 0");
        if (S->comm.active()) return fail(FS_EINVAL, "fs_confine_vorticity: vorticity confinement needs a single GPU handle");
        if (eps == 0.0) return FS_OK;
        if (!eng.in_step) eng.vzmax_prev = -1.0;             // a call from outside step(): what is known about v_z is void
        return pass("fs_confine_vorticity", eps);
    }

private:
    Engine<T>& eng;
    fs_sim* const S;
    const fs::GridDesc& g;
    T* (&arr)[NPOOL_MAX];
    int (&slot)[NSLOT];
    uint8_t*& flags;
};

}  // namespace
