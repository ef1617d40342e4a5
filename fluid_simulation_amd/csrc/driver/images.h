// driver/images.h -- slice and projection images (csrc/image.h; the reference's 2-D viewer does this on the host, gui.py:61-79, 257-295)
#pragma once
#include "common.h"
#include "../image.h"

namespace {

template <class T>
struct Images {
    explicit Images(Engine<T>& e_) : eng(e_), S(e_.S), g(e_.g), arr(e_.arr), slot(e_.slot), flags(e_.flags) {}

    long max_pixels() const
    {
        const long a = (long)(g.W + 2) * (g.H + 2), b = (long)(g.W + 2) * (g.D + 2), c = (long)(g.H + 2) * (g.D + 2);
        return std::max(a, std::max(b, c));
    }

    // the scratch images and the device copy of the colour table, at first need and after fs_image_colormap
    int ensure_scratch()
    {
        if (!img_val) {
            const size_t np = ((size_t)max_pixels() + 15) / 16 * 16;
            const hipError_t e = img_buf.alloc(np * 16 + 3 * (size_t)fs::IMG_TABLE_MAX);
            if (e != hipSuccess) return fail(FS_ENOMEM, "image scratch of %zu bytes: %s", np * 16 + 3 * (size_t)fs::IMG_TABLE_MAX, hipGetErrorString(e));
            uint8_t* const base = img_buf.get();
            img_val = (double*)base;
            img_flag = base + 8 * np;
            for (int a = 0; a < 3; ++a) img_sil[a] = base + (9 + (size_t)a) * np;
            img_rgb = base + 12 * np;
            img_table = base + 16 * np;
            img_sil_ok[0] = img_sil_ok[1] = img_sil_ok[2] = false;
            img_table_gen = -1;
        }
        if (img_table_gen != S->image_table_gen) {
            const bool own = !S->image_table.empty();
            img_table_n = own ? (int)(S->image_table.size() / 3) : fs::IMG_DEFAULT_N;
            HIP_TRY(hipMemcpyAsync(img_table, own ? S->image_table.data() : fs::IMG_DEFAULT_TABLE, 3 * (size_t)img_table_n,
                                   hipMemcpyHostToDevice, S->stream));
            HIP_TRY(hipStreamSynchronize(S->stream));    // the handle's table may be replaced by the caller
            img_table_gen = S->image_table_gen;
        }
        return FS_OK;
    }

    // One value image into img_val and its obstacle flags (-> flag): the kernels of one view.  The arguments are checked.
    int render(const char* who, int source, int kind, int axis, int index, const uint8_t*& flag)
    {
        int rc = eng.ensure_flags();                         // obs changed: the silhouettes are stale
        if (rc) return rc;
        const T* field = nullptr;
        const double* stat = nullptr;
        if ((rc = eng.sampling.resolve_source(who, source, field, stat))) return rc;
        const T* obs = arr[slot[FS_OBS]];
        if (kind == fs::IMG_SLICE) {
            if (stat) fs::launch_image_slice<double, T>(S->stream, g, axis, index, stat, obs, img_val, img_flag);
            else fs::launch_image_slice<T, T>(S->stream, g, axis, index, field, obs, img_val, img_flag);
            flag = img_flag;
            return FS_OK;
        }
        if (stat) fs::launch_image_project<double>(S->stream, g, kind, axis, stat, img_val, nullptr);
        else fs::launch_image_project<T>(S->stream, g, kind, axis, field, img_val, nullptr);
        if (!img_sil_ok[axis]) {                         // the silhouette depends on obs and the axis only
            fs::launch_image_project<T>(S->stream, g, fs::IMG_ANY, axis, obs, nullptr, img_sil[axis]);
            img_sil_ok[axis] = true;
        }
        flag = img_sil[axis];
        return FS_OK;
    }

    int args(const char* who, int kind, int axis, int index, int* cols, int* rows)
    {
        if (S->comm.active()) return fail(FS_EINVAL, "%s: images are taken on a single-GPU handle", who);
        if (kind < 0 || kind >= fs::IMG_NKINDS) return fail(FS_EINVAL, "%s: unknown kind %d (FS_IMG_SLICE | SUM | MAX | MIN)", who, kind);
        if (axis < 0 || axis > 2) return fail(FS_EINVAL, "%s: axis %d (0 = x, 1 = y, 2 = z)", who, axis);
        const int N = axis == 0 ? g.W : axis == 1 ? g.H : g.D;
        if (index < 0 || index > (kind == fs::IMG_SLICE ? N + 1 : 0))
            return fail(FS_EINVAL, "%s: index %d (a slice: 0 .. %d; a projection: 0)", who, index, N + 1);
        int c, r;
        fs::image_dims(axis, g.W, g.H, g.D, &c, &r);
        if (cols) *cols = c;
        if (rows) *rows = r;
        return FS_OK;
    }

    int values(int source, int kind, int axis, int index, double* out, size_t n, int* cols, int* rows)
    {
        int c, r;
        int rc = args("fs_image_values", kind, axis, index, &c, &r);
        if (rc) return rc;
        if (!image_source_ok(source)) return fail(FS_EINVAL, "fs_image_values: unknown source %d", source);
        if (cols) *cols = c;
        if (rows) *rows = r;
        if (!out) return FS_OK;
        if (n != (size_t)c * (size_t)r) return fail(FS_EINVAL, "fs_image_values: the image has %d x %d values, the call has room for %zu", c, r, n);
        if ((rc = ensure_scratch())) return rc;
        const uint8_t* flag = nullptr;
        {
            ScopedSpan sp(S, FAM_MISC);
            if ((rc = render("fs_image_values", source, kind, axis, index, flag))) return rc;
        }
        HIP_TRY(hipMemcpyAsync(out, img_val, n * sizeof(double), hipMemcpyDeviceToHost, S->stream));
        HIP_TRY(hipStreamSynchronize(S->stream));
        return FS_OK;
    }

    int rgb(int source, int kind, int axis, int index, double vmin, double vmax, double alpha, uint8_t* out, size_t n_bytes,
                  int* cols, int* rows)
    {
        int c, r;
        int rc = args("fs_image_rgb", kind, axis, index, &c, &r);
        if (rc) return rc;
        if (!image_source_ok(source)) return fail(FS_EINVAL, "fs_image_rgb: unknown source %d", source);
        if (!image_range_ok(vmin, vmax, alpha)) return fail(FS_EINVAL, "fs_image_rgb: vmin < vmax, both finite, and obstacle_alpha in [0, 1]");
        if (cols) *cols = c;
        if (rows) *rows = r;
        if (!out) return FS_OK;
        const size_t npix = (size_t)c * (size_t)r;
        if (n_bytes != 3 * npix) return fail(FS_EINVAL, "fs_image_rgb: the image has %d x %d x 3 bytes, the call has room for %zu", c, r, n_bytes);
        if ((rc = ensure_scratch())) return rc;
        const uint8_t* flag = nullptr;
        {
            ScopedSpan sp(S, FAM_MISC);
            if ((rc = render("fs_image_rgb", source, kind, axis, index, flag))) return rc;
            fs::launch_image_colour(S->stream, (long)npix, img_val, flag, vmin, vmax, alpha, img_table, img_table_n, img_rgb);
        }
        HIP_TRY(hipMemcpyAsync(out, img_rgb, n_bytes, hipMemcpyDeviceToHost, S->stream));
        HIP_TRY(hipStreamSynchronize(S->stream));
        return FS_OK;
    }

    int config() { return ensure_ring(); }

    // (re)allocate and clear the ring after fs_image_views / fs_set_option("image_log"), and set up whatever a view needs, so
    // that a record in mid-step allocates nothing: the scratch images, the vortex array, the staging of a statistics source
    int ensure_ring()
    {
        if (img_ring.gen == S->image_gen) return img_ring.on() ? ensure_scratch() : FS_OK;   // a new colour table
        HIP_TRY(img_ring.setup(S->stream, S->image_gen));   // off, whatever fails below
        if (S->image_views.empty() || S->image_log <= 0) return FS_OK;
        if (S->comm.active()) return fail(FS_EINVAL, "the image log needs a single-GPU handle");
        int rc = ensure_scratch();
        if (rc) return rc;
        size_t bytes = 0;
        for (const ImageView& v : S->image_views) {
            int c, r;
            fs::image_dims(v.axis, g.W, g.H, g.D, &c, &r);
            bytes += 3 * (size_t)c * (size_t)r;
            if ((v.source & ~(FS_ISO_VORTEX - 1)) == FS_ISO_VORTEX && (rc = eng.vortex.ensure("fs_image_views"))) return rc;
            if ((v.source & ~(FS_SAMPLE_STAT - 1)) == FS_SAMPLE_STAT && (rc = eng.need_dense(eng.flow_stats.bytes()))) return rc;
        }
        const hipError_t e = img_ring.setup(S->stream, S->image_gen, S->image_log, bytes);
        if (e != hipSuccess && !img_ring.base.get()) return fail(FS_ENOMEM, "image_log: %d frames of %zu bytes: %s", S->image_log, bytes, hipGetErrorString(e));
        HIP_TRY(e);
        return FS_OK;
    }

    // one frame of the state as it is now into the next ring slot: every view's kernels, then its colouring
    int record()
    {
        uint8_t* dst = (uint8_t*)img_ring.slot(img_ring.at.next());
        for (const ImageView& v : S->image_views) {
            int c, r;
            fs::image_dims(v.axis, g.W, g.H, g.D, &c, &r);
            const uint8_t* flag = nullptr;
            ScopedSpan sp(S, FAM_IMAGES);
            const int rc = render("the image log", v.source, v.kind, v.axis, v.index, flag);
            if (rc) return rc;
            fs::launch_image_colour(S->stream, (long)c * r, img_val, flag, v.vmin, v.vmax, v.alpha, img_table, img_table_n, dst);
            dst += 3 * (size_t)c * (size_t)r;
        }
        img_ring.at.commit(S->steps_total);
        return FS_OK;
    }

    int sample()
    {
        int rc = ensure_ring();
        if (rc) return rc;
        if (!img_ring.on()) return fail(FS_EINVAL, "fs_image_sample: no views are set (fs_image_views), or option \"image_log\" is 0");
        return record();
    }

    int log_fetch(uint8_t* frames, long* steps, long max_frames, long* n_frames, long* n_dropped)
    {
        int rc = ensure_ring();
        if (rc) return rc;
        rc = img_ring.fetch_begin({"fs_image_log", "frames", "frames = NULL"}, img_ring.at.retained(), max_frames,
                                  frames != nullptr, n_frames, n_dropped);
        if (rc != LogRing::GO_ON) return rc;
        HIP_TRY(img_ring.fetch_copy(S->stream, frames));
        img_ring.fetch_end(steps);
        return FS_OK;
    }

    bool on() const { return img_ring.on(); }
    void obs_changed() { img_sil_ok[0] = img_sil_ok[1] = img_sil_ok[2] = false; }   // the silhouettes are stale
    // the colour table on the device (after ensure_scratch): the volume renderer uses it too
    const uint8_t* table() const { return img_table; }
    int table_n() const { return img_table_n; }

private:
    Engine<T>& eng;
    fs_sim* const S;
    const fs::GridDesc& g;
    T* (&arr)[NPOOL_MAX];
    int (&slot)[NSLOT];
    uint8_t*& flags;
    // one allocation holds the value image, the flag image of a slice, the obstacle silhouette of each axis (valid until obs
    // changes), an RGB staging image and the colour table; the per-step log is a device ring of frames (the views' RGB images
    // one after the other)
    DevBuf<uint8_t> img_buf;            // the allocation; the pointers below are views into it
    double* img_val = nullptr;          // its base
    uint8_t* img_flag = nullptr;
    uint8_t* img_sil[3] = {nullptr, nullptr, nullptr};
    bool img_sil_ok[3] = {false, false, false};
    uint8_t* img_rgb = nullptr;
    uint8_t* img_table = nullptr;
    int img_table_n = 0;
    long img_table_gen = -1;            // S->image_table_gen the device table holds
    LogRing img_ring;                   // for S->image_gen
};

}  // namespace
