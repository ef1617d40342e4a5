// driver/vortex.h -- vortex identification (csrc/vortex.h; beyond the reference) and iso-surfaces of any field
#pragma once
#include "common.h"
#include "../vortex.h"

namespace {

template <class T>
struct Vortex {
    explicit Vortex(Engine<T>& e_) : eng(e_), S(e_.S), g(e_.g), sc(e_.sc), arr(e_.arr), slot(e_.slot), flags(e_.flags) {}

    // the private array the vortex kernel writes, allocated and zeroed at first need
    int ensure(const char* who)
    {
        if (vort) return FS_OK;
        const hipError_t e = base.alloc((size_t)g.n);
        if (e != hipSuccess) return fail(FS_ENOMEM, "%s: scratch array of %zu bytes: %s", who, (size_t)g.n * sizeof(T), hipGetErrorString(e));
        vort = base.get() + g.lead;
        HIP_TRY(hipMemsetAsync(base.get(), 0, (size_t)g.n * sizeof(T), S->stream));
        return FS_OK;
    }

    // One field into `vort`.  Collective on slab handles: the stencil reads one plane of each neighbour.
    int compute(const char* who, int which)
    {
        if (which < 0 || which >= FS_VORTEX_NFIELDS) return fail(FS_EINVAL, "%s: unknown vortex selector %d (0..%d)", who, which, FS_VORTEX_NFIELDS - 1);
        if (S->comm.active() && S->comm.null_transport)
            return fail(FS_EINVAL, "%s: vortex fields need the other slabs' planes; the FSNULL transport carries none", who);
        int rc = eng.ensure_flags();
        if (rc) return rc;
        for (int f : { FS_VX, FS_VY, FS_VZ })
            if ((rc = eng.halo(arr[slot[f]]))) return rc;
        if ((rc = ensure(who))) return rc;
        ScopedSpan sp(S, FAM_VORTEX);
        fs::launch_vortex<T>(S->stream, S->tune, g, sc, which, arr[slot[FS_VX]], arr[slot[FS_VY]], arr[slot[FS_VZ]], flags, vort);
        return FS_OK;
    }

    int fetch(int which, void* dst, size_t n, int elem)
    {
        if ((long)n != eng.dense_cells()) return fail(FS_EINVAL, "fs_vortex_field: expected %ld elements, got %zu", eng.dense_cells(), n);
        if (elem != 4 && elem != 8) return fail(FS_EINVAL, "fs_vortex_field: elem_size must be 4 or 8");
        int rc = compute("fs_vortex_field", which);
        if (rc) return rc;
        if ((rc = eng.need_dense(n * (size_t)elem))) return rc;
        if (elem == 4) fs::launch_pack<T, float>(S->stream, g, vort, (float*)eng.dense.get(), 0, g.D + 1);
        else fs::launch_pack<T, double>(S->stream, g, vort, (double*)eng.dense.get(), 0, g.D + 1);
        HIP_TRY(hipMemcpyAsync(dst, eng.dense.get(), n * elem, hipMemcpyDeviceToHost, S->stream));
        HIP_TRY(hipStreamSynchronize(S->stream));
        return FS_OK;
    }

    int dump(const char* dir)
    {
        static const char* const names[FS_VORTEX_NFIELDS] = { "vort_x.bin", "vort_y.bin", "vort_z.bin", "vort_sq.bin", "q.bin" };
        if (S->comm.active() && S->comm.null_transport)
            return fail(FS_EINVAL, "fs_vortex_dump: vortex fields need the other slabs' planes; the FSNULL transport carries none");
        int rc = FS_OK;
        // rank 0 truncates; the other slab ranks open the files for update once they exist (as fs_flow_stats_dump does)
        const bool lead = !S->comm.active() || S->comm.rank == 0;
        FILE* fp[FS_VORTEX_NFIELDS] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        bool ok = true;
        for (int pass = 0; pass < 2; ++pass) {
            if ((pass == 0) == lead)
                for (int k = 0; k < FS_VORTEX_NFIELDS; ++k) {
                    fp[k] = fopen((std::string(dir) + "/" + names[k]).c_str(), lead ? "wb" : "r+b");
                    if (!fp[k]) ok = false;
                }
            if (pass == 0 && S->comm.active()) {
                if (S->comm.shm && S->comm.shm_ready(g, S->D)) return fail(FS_ECOMM, "%s", S->comm.last_error());
                if ((rc = eng.slab_barrier())) return rc;
            }
        }
        // local planes written by this rank: its interior planes, plus the physical ghost planes
        const int zlo = sc.lo_wall ? 0 : 1, zhi = sc.hi_wall ? g.D + 1 : g.D;
        const size_t plane = (size_t)(g.W + 2) * (g.H + 2);
        std::vector<float> h((size_t)eng.dense_cells());
        for (int k = 0; k < FS_VORTEX_NFIELDS && !rc; ++k) {     // every rank computes all five (collective), whatever its files do
            rc = fetch(k, h.data(), h.size(), 4);
            if (rc || !ok || !fp[k]) continue;
            if (fseek(fp[k], (long)(plane * (size_t)(sc.zoff + zlo) * sizeof(float)), SEEK_SET) != 0 ||
                fwrite(h.data() + plane * (size_t)zlo, sizeof(float), plane * (size_t)(zhi - zlo + 1), fp[k]) != plane * (size_t)(zhi - zlo + 1))
                ok = false;
        }
        for (int k = 0; k < FS_VORTEX_NFIELDS; ++k)
            if (fp[k] && fclose(fp[k]) != 0) ok = false;
        if (S->comm.active() && !rc) rc = eng.slab_barrier();     // every rank's planes are in the files
        if (rc) return rc;
        if (!ok) return fail(FS_EIO, "fs_vortex_dump: cannot write the vortex frames under '%s'", dir);
        return FS_OK;
    }

    int isosurface(int source, double level)
    {
        S->iso_valid = false;
        if (S->comm.active()) return fail(FS_EINVAL, "fs_isosurface: iso-surfaces are extracted on a single-GPU handle");
        const T* field = nullptr;
        if (source >= 0 && source < FS_NFIELDS) {
            field = arr[slot[source]];
        } else if ((source & ~(FS_ISO_VORTEX - 1)) == FS_ISO_VORTEX && (source & (FS_ISO_VORTEX - 1)) < FS_VORTEX_NFIELDS) {
            int rc = compute("fs_isosurface", source & (FS_ISO_VORTEX - 1));
            if (rc) return rc;
            field = vort;
        } else if (source == FS_SOURCE_HEAT) {
            if (!eng.heat.on()) return fail(FS_EINVAL, "fs_isosurface: FS_SOURCE_HEAT while heat is off (fs_heat_params, mode 1 or 2)");
            field = arr[slot[F_THETA]];
        } else {
            return fail(FS_EINVAL, "fs_isosurface: unknown source %d (a field selector, FS_SOURCE_HEAT, or FS_ISO_VORTEX | FS_VORTEX_*)", source);
        }
        return eng.viewer.surface_into(field, (T)level, S->iso_verts, S->iso_tris, S->iso_valid);
    }

    const T* array() const { return vort; }   // what the last compute() left

private:
    Engine<T>& eng;
    fs_sim* const S;
    const fs::GridDesc& g;
    const fs::SlabCtx& sc;
    T* (&arr)[NPOOL_MAX];
    int (&slot)[NSLOT];
    uint8_t*& flags;
    // the one field a call computes, in the fields' layout (LEAD-shifted like them); allocated at the first call.  Only the
    // kernel writes it, and only cells of interior rows: its ghosts stay +0.0.
    DevBuf<T> base;
    T* vort = nullptr;
};

}  // namespace
