// driver/volume.h -- volume rendering (csrc/volume.h; the reference's 3-D viewer, GUI/gl_widget.py, renders no volume)
#pragma once
#include "common.h"
#include "../volume.h"

namespace {

template <class T>
struct Volume {
    explicit Volume(Engine<T>& e_) : eng(e_), S(e_.S), g(e_.g), arr(e_.arr), slot(e_.slot) {}

    // A slot's ray set: uploaded into a new array, then the old one goes (a queued frame may still read it: the stream is
    // synchronised first).  cols = rows = 0 frees the slot.  The arguments are checked by fs_volume_rays.
    int set_rays(int slot, const double* rays, int cols, int rows)
    {
        DevBuf<double> fresh;
        const size_t bytes = (size_t)cols * (size_t)rows * 6 * sizeof(double);
        if (bytes > 0) {
            const hipError_t e = fresh.alloc(bytes / sizeof(double));
            if (e != hipSuccess) return fail(FS_ENOMEM, "fs_volume_rays: %d x %d rays: %s", cols, rows, hipGetErrorString(e));
            hipError_t c = hipMemcpyAsync(fresh.get(), rays, bytes, hipMemcpyHostToDevice, S->stream);
            if (c == hipSuccess) c = hipStreamSynchronize(S->stream);   // `rays` may be freed by the caller
            HIP_TRY(c);
        }
        if (vol_rays[slot].get()) {
            HIP_TRY(hipStreamSynchronize(S->stream));
            HIP_TRY(vol_rays[slot].release());
        }
        vol_rays[slot] = std::move(fresh);
        return FS_OK;
    }

    // one view of the state as it is now: one launch.  The arguments are checked; rgb / acc are device arrays, either may be null.
    int launch(const char* who, int source, int cam, const double* par, uint8_t* rgb, double* acc)
    {
        fs::VolumeView vw = {};
        if (!fs::volume_params_ok(par, g.W, g.H, g.D, &vw.kmax)) return fail(FS_EINVAL, "%s: bad view parameters", who);
        for (int k = 0; k < fs::VOLUME_PARAMS; ++k) vw.par[k] = par[k];
        vw.n = eng.images.table_n();
        const T* field = nullptr;
        const double* stat = nullptr;
        const int rc = eng.sampling.resolve_source(who, source, field, stat);
        if (rc) return rc;
        const T* obs = arr[slot[FS_OBS]];
        const int cols = S->vol_cols[cam], rows = S->vol_rows[cam];
        if (stat) fs::launch_volume<double, T>(S->stream, g, vw, cols, rows, vol_rays[cam].get(), stat, obs, eng.images.table(), rgb, acc);
        else fs::launch_volume<T, T>(S->stream, g, vw, cols, rows, vol_rays[cam].get(), field, obs, eng.images.table(), rgb, acc);
        return FS_OK;
    }

    int render(int source, int slot, const double* par, uint8_t* rgb, size_t n_bytes, double* acc, size_t n_acc)
    {
        const size_t npix = (size_t)S->vol_cols[slot] * (size_t)S->vol_rows[slot];
        int rc = eng.images.ensure_scratch();                 // the colour table
        if (rc) return rc;
        hipError_t e = vol_acc.grow(npix * 4, S->stream);    // a queued render may still use what is freed here
        if (e == hipSuccess) e = vol_rgb.grow(npix * 3, S->stream);
        if (e != hipSuccess) {
            vol_acc.release();
            vol_rgb.release();
            return fail(FS_ENOMEM, "fs_volume_render: %zu pixels: %s", npix, hipGetErrorString(e));
        }
        {
            ScopedSpan sp(S, FAM_MISC);
            if ((rc = launch("fs_volume_render", source, slot, par, rgb ? vol_rgb.get() : nullptr, acc ? vol_acc.get() : nullptr))) return rc;
        }
        if (rgb) HIP_TRY(hipMemcpyAsync(rgb, vol_rgb.get(), n_bytes, hipMemcpyDeviceToHost, S->stream));
        if (acc) HIP_TRY(hipMemcpyAsync(acc, vol_acc.get(), n_acc * sizeof(double), hipMemcpyDeviceToHost, S->stream));
        HIP_TRY(hipStreamSynchronize(S->stream));
        return FS_OK;
    }

    int config() { return ensure_ring(); }

    // (re)allocate and clear the ring after fs_volume_views / fs_volume_rays / fs_set_option("volume_log"), and set up whatever a
    // view needs, so that a record in mid-step allocates nothing: the colour table, the vortex array, the staging of a
    // statistics source
    int ensure_ring()
    {
        if (vol_ring.gen == S->volume_gen) return vol_ring.on() ? eng.images.ensure_scratch() : FS_OK;   // a new colour table
        HIP_TRY(vol_ring.setup(S->stream, S->volume_gen));   // off, whatever fails below
        if (S->volume_views.empty() || S->volume_log <= 0) return FS_OK;
        if (S->comm.active()) return fail(FS_EINVAL, "the volume log needs a single-GPU handle");
        int rc = eng.images.ensure_scratch();
        if (rc) return rc;
        for (const VolumeLogView& v : S->volume_views) {
            if ((v.source & ~(FS_ISO_VORTEX - 1)) == FS_ISO_VORTEX && (rc = eng.vortex.ensure("fs_volume_views"))) return rc;
            if ((v.source & ~(FS_SAMPLE_STAT - 1)) == FS_SAMPLE_STAT && (rc = eng.need_dense(eng.flow_stats.bytes()))) return rc;
        }
        const size_t bytes = volume_frame_bytes(S, S->volume_views);
        const hipError_t e = vol_ring.setup(S->stream, S->volume_gen, S->volume_log, bytes);
        if (e != hipSuccess && !vol_ring.base.get()) return fail(FS_ENOMEM, "volume_log: %d frames of %zu bytes: %s", S->volume_log, bytes, hipGetErrorString(e));
        HIP_TRY(e);
        return FS_OK;
    }

    // one frame of the state as it is now into the next ring slot: one launch per view
    int record()
    {
        uint8_t* dst = (uint8_t*)vol_ring.slot(vol_ring.at.next());
        for (const VolumeLogView& v : S->volume_views) {
            ScopedSpan sp(S, FAM_VOLUME);
            const int rc = launch("the volume log", v.source, v.slot, v.par, dst, nullptr);
            if (rc) return rc;
            dst += 3 * (size_t)S->vol_cols[v.slot] * (size_t)S->vol_rows[v.slot];
        }
        vol_ring.at.commit(S->steps_total);
        return FS_OK;
    }

    int sample()
    {
        int rc = ensure_ring();
        if (rc) return rc;
        if (!vol_ring.on()) return fail(FS_EINVAL, "fs_volume_sample: no views are set (fs_volume_views), or option \"volume_log\" is 0");
        return record();
    }

    int log_fetch(uint8_t* frames, long* steps, long max_frames, long* n_frames, long* n_dropped)
    {
        int rc = ensure_ring();
        if (rc) return rc;
        rc = vol_ring.fetch_begin({"fs_volume_log", "frames", "frames = NULL"}, vol_ring.at.retained(), max_frames,
                                  frames != nullptr, n_frames, n_dropped);
        if (rc != LogRing::GO_ON) return rc;
        HIP_TRY(vol_ring.fetch_copy(S->stream, frames));
        vol_ring.fetch_end(steps);
        return FS_OK;
    }

    bool on() const { return vol_ring.on(); }

private:
    Engine<T>& eng;
    fs_sim* const S;
    const fs::GridDesc& g;
    T* (&arr)[NPOOL_MAX];
    int (&slot)[NSLOT];
    // the ray set of each camera slot, the staging images of fs_volume_render (grown on demand), and the per-step log, a device
    // ring of frames (the views' RGB images one after the other).  The colour table is the image entries' (driver/images.h).
    DevBuf<double> vol_rays[fs::VOLUME_CAMERAS_MAX];
    DevBuf<uint8_t> vol_rgb;
    DevBuf<double> vol_acc;
    LogRing vol_ring;                   // for S->volume_gen
};

}  // namespace
