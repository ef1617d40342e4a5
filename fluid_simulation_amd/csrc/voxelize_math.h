// voxelize_math.h -- everything of the STL voxelizer (voxelize.hip) that needs no HIP runtime: the mesh parser, the Euler
// rotation, the setup that turns triangles and arguments into VoxParams and the 64^3 occupancy grid (host), and the
// per-sample functions the kernels call (host and device).  Plain C++17, so that tests/test_voxelize_cpu.py compiles exactly
// what the kernels run.  Every written operation is rounded once, in the order written (the library and the test driver
// are built with -ffp-contract=off).  Line numbers refer to the reference's object_loader.cpp.  Internal to libfluidsim.so.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define FS_VOX_HD __host__ __device__
#else
#define FS_VOX_HD
#endif

namespace fs {
namespace vox {

struct P3 { float x, y, z; };
struct Tri { P3 a, b, c; };

struct VoxParams {
    int ns;
    float lo, res, cell;
    float gscale, cx, cy, cz, tx, ty, tz;
    int W, H, D;
    unsigned seed;
    int ntri;
};

constexpr int GRID = 64;                 // object_loader.cpp:382
constexpr unsigned LCG_A = 48271u;       // std::minstd_rand
constexpr unsigned LCG_M = 2147483647u;

// ---------------------------------------------------------------------------- host: parser, rotation, setup

inline std::string strip(const std::string& s)
{
    size_t a = s.find_first_not_of(" \t\n\r");
    if (a == std::string::npos) return "";
    size_t b = s.find_last_not_of(" \t\n\r");
    return s.substr(a, b - a + 1);
}

// object_loader.cpp:98-174.  false: the file cannot be opened.  The rules for files that are not clean:
//   * a file whose first line, stripped, starts with "solid" is ASCII, whatever follows (:107);
//   * a binary file keeps the complete 50-byte records it holds: reading stops at the first short record, and at the count
//     field's number if that comes first;
//   * nothing is sized by the count field (a corrupt one names up to 2^32 - 1 records);
//   * an ASCII facet counts when exactly three vertex lines parsed since its "outer loop": a fourth wraps the counter to 0.
inline bool read_stl(const char* path, std::vector<Tri>& out)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    std::string line;
    std::getline(f, line);
    const bool binary = (strip(line).find("solid") != 0);      // :107
    f.close();
    if (binary) {
        f.open(path, std::ios::binary);
        if (!f) return false;
        f.seekg(80);
        uint32_t n = 0;
        f.read(reinterpret_cast<char*>(&n), 4);
        if (!f) return true;
        for (uint32_t i = 0; i < n; ++i) {
            float rec[12];
            uint16_t attr;
            f.read(reinterpret_cast<char*>(rec), sizeof rec);
            f.read(reinterpret_cast<char*>(&attr), 2);
            if (!f) break;                                       // truncated file: keep what is complete
            Tri t;
            t.a = { rec[3], rec[4], rec[5] };
            t.b = { rec[6], rec[7], rec[8] };
            t.c = { rec[9], rec[10], rec[11] };
            out.push_back(t);
        }
    } else {
        f.open(path);
        if (!f) return false;
        Tri cur{};
        int vi = 0;
        while (std::getline(f, line)) {
            line = strip(line);
            if (line == "outer loop") { vi = 0; continue; }
            if (line == "endloop") continue;
            if (line == "endfacet") { if (vi == 3) out.push_back(cur); continue; }
            if (line.compare(0, 6, "vertex") == 0) {
                std::istringstream iss(line.substr(6));
                float x, y, z;
                if (iss >> x >> y >> z) {
                    P3 v = { x, y, z };
                    if (vi == 0) cur.a = v; else if (vi == 1) cur.b = v; else if (vi == 2) cur.c = v;
                    vi = (vi + 1) % 4;                           // :166
                }
            }
        }
    }
    return true;
}

// object_loader.cpp:177-202
inline P3 rotate(const P3& p, float dx, float dy, float dz)
{
    const float rx = dx * M_PI / 180.0f, ry = dy * M_PI / 180.0f, rz = dz * M_PI / 180.0f;
    const float cx = cosf(rx), sx = sinf(rx), cy = cosf(ry), sy = sinf(ry), cz = cosf(rz), sz = sinf(rz);
    P3 o;
    o.x = (cy * cz) * p.x + (-cy * sz) * p.y + (sy) * p.z;
    o.y = (sx * sy * cz + cx * sz) * p.x + (-sx * sy * sz + cx * cz) * p.y + (-sx * cy) * p.z;
    o.z = (-cx * sy * cz + sx * sz) * p.x + (cx * sy * sz + sx * cz) * p.y + (cx * cy) * p.z;
    return o;
}

// What the kernels need of one mesh and one set of arguments: the rotated triangles (9 floats each), the coarse occupancy
// grid and the parameters.  raw must not be empty.
struct VoxSetup {
    VoxParams q;
    std::vector<float> rt;
    std::vector<uint8_t> occ;
};

inline void setup(const std::vector<Tri>& raw, int W, int H, int D, float scale, float rot_x, float rot_y, float rot_z,
                  float tr_x, float tr_y, float tr_z, unsigned seed, VoxSetup& s)
{
    // objCenter is the origin: orig_min/orig_max are never updated (:288-296)
    std::vector<float>& rt = s.rt;
    rt.assign(raw.size() * 9, 0.0f);
    float r2 = 0.0f;
    for (size_t i = 0; i < raw.size(); ++i) {
        const P3 v[3] = { raw[i].a, raw[i].b, raw[i].c };
        for (int k = 0; k < 3; ++k) {
            P3 r = rotate(v[k], rot_x, rot_y, rot_z);                        // :302-316
            rt[i * 9 + k * 3 + 0] = r.x; rt[i * 9 + k * 3 + 1] = r.y; rt[i * 9 + k * 3 + 2] = r.z;
            float d2 = v[k].x * v[k].x + v[k].y * v[k].y + v[k].z * v[k].z;  // unrotated, :328-333
            if (d2 > r2) r2 = d2;
        }
    }
    const float radius = std::sqrt(r2);
    const float pad = radius * 0.05f;                                        // :349
    const float lo = (0.0f - radius) - pad, hi = (0.0f + radius) + pad;
    const float span = hi - lo;                                              // objSize
    float res = span / 200.0f;                                               // :368
    if (res < 0.02f) res = 0.02f;
    const int ns = (int)(span / res);                                        // :370-372

    // coarse occupancy grid: triangle AABBs rasterised with (int) truncation (:54-77, :380-389)
    const float cell = res * 5.0f;
    std::vector<uint8_t>& occ = s.occ;
    occ.assign((size_t)GRID * GRID * GRID, 0);
    for (size_t i = 0; i < raw.size(); ++i) {
        const float* t = &rt[i * 9];
        float mn[3], mx[3];
        for (int a = 0; a < 3; ++a) {
            mn[a] = std::min(std::min(t[a], t[3 + a]), t[6 + a]);
            mx[a] = std::max(std::max(t[a], t[3 + a]), t[6 + a]);
        }
        int c0[3], c1[3];
        for (int a = 0; a < 3; ++a) {
            c0[a] = std::max(0, (int)((mn[a] - lo) / cell));
            c1[a] = std::min(GRID - 1, (int)((mx[a] - lo) / cell));
        }
        for (int z = c0[2]; z <= c1[2]; ++z)
            for (int y = c0[1]; y <= c1[1]; ++y)
                for (int x = c0[0]; x <= c1[0]; ++x) occ[x + y * GRID + z * GRID * GRID] = 1;
    }

    VoxParams& q = s.q;
    q.ns = ns; q.lo = lo; q.res = res; q.cell = cell;
    q.gscale = scale * std::min(std::min((float)W, (float)H), (float)D) / span;   // :429
    q.cx = (float)W / 2; q.cy = (float)H / 2; q.cz = (float)D / 2;                // :430
    q.tx = tr_x; q.ty = tr_y; q.tz = tr_z;
    q.W = W; q.H = H; q.D = D; q.seed = seed; q.ntri = (int)raw.size();
}

// ---------------------------------------------------------------------------- host and device: one sample

FS_VOX_HD inline unsigned mulmod(unsigned a, unsigned b)
{
    return (unsigned)(((unsigned long long)a * b) % LCG_M);
}
FS_VOX_HD inline unsigned powmod(unsigned base, unsigned long long e)
{
    unsigned r = 1u;
    while (e) {
        if (e & 1ull) r = mulmod(r, base);
        base = mulmod(base, base);
        e >>= 1;
    }
    return r;
}

// sample n = (i*ns + j)*ns + k, the reference's loop order (object_loader.cpp:403-405)
FS_VOX_HD inline void sample_point(const VoxParams& q, long n, float& x, float& y, float& z)
{
    const int k = (int)(n % q.ns), j = (int)((n / q.ns) % q.ns), i = (int)(n / ((long)q.ns * q.ns));
    x = q.lo + i * q.res;                                        // :407-409
    y = q.lo + j * q.res;
    z = q.lo + k * q.res;
}

// VoxelGrid::contains, object_loader.cpp:79-87: does sample n survive the coarse-grid rejection
FS_VOX_HD inline uint8_t sample_kept(const VoxParams& q, const uint8_t* occ, long n)
{
    float x, y, z;
    sample_point(q, n, x, y, z);
    uint8_t k = 0;
    if (!(x < q.lo || y < q.lo || z < q.lo)) {
        int ix = (int)((x - q.lo) / q.cell), iy = (int)((y - q.lo) / q.cell), iz = (int)((z - q.lo) / q.cell);
        if (ix >= 0 && ix < GRID && iy >= 0 && iy < GRID && iz >= 0 && iz < GRID)
            k = occ[ix + iy * GRID + iz * GRID * GRID];
    }
    return k;
}

// Moeller-Trumbore exactly as object_loader.cpp:205-233
FS_VOX_HD inline bool ray_hits(float ox, float oy, float oz, float dx, float dy, float dz, const float* t)
{
    const float EPS = 1e-6f;
    const float e1x = t[3] - t[0], e1y = t[4] - t[1], e1z = t[5] - t[2];
    const float e2x = t[6] - t[0], e2y = t[7] - t[1], e2z = t[8] - t[2];
    const float hx = dy * e2z - dz * e2y, hy = dz * e2x - dx * e2z, hz = dx * e2y - dy * e2x;
    const float det = e1x * hx + e1y * hy + e1z * hz;
    if (fabsf(det) < EPS) return false;
    const float f = 1.0f / det;
    const float sx = ox - t[0], sy = oy - t[1], sz = oz - t[2];
    const float u = f * (sx * hx + sy * hy + sz * hz);
    if (u < 0.0f || u > 1.0f) return false;
    const float qx = sy * e1z - sz * e1y, qy = sz * e1x - sx * e1z, qz = sx * e1y - sy * e1x;
    const float v = f * (dx * qx + dy * qy + dz * qz);
    if (v < 0.0f || u + v > 1.0f) return false;
    const float tt = f * (e2x * qx + e2y * qy + e2z * qz);
    return tt > 1e-3f;
}

FS_VOX_HD inline unsigned lcg_step(unsigned& st)
{
    st = mulmod(st, LCG_A);
    return st;
}
// The generator's state in front of the six draws of the surviving sample of rank r: the sequential stream jumped ahead by
// 6r draws, x_n = x_0 * a^n mod m.
FS_VOX_HD inline unsigned lcg_jump(unsigned seed, unsigned long long r)
{
    unsigned s0 = seed % LCG_M;                                  // minstd_rand(seed): 0 maps to 1
    if (s0 == 0) s0 = 1;
    return mulmod(s0, powmod(LCG_A, 6ull * r));
}
// the jitter of one coordinate, :417-419
FS_VOX_HD inline float lcg_jitter(unsigned& st)
{
    return (float)(unsigned long long)(lcg_step(st) % 1000u) * 1e-6f - 5e-4f;
}
// std::uniform_real_distribution<float>(0.1f, 1.0f) on minstd_rand (libstdc++): one draw,
// generate_canonical = float(x - min) / float(range) with range 2^31-2 rounding to 2^31.
FS_VOX_HD inline float lcg_unit(unsigned& st)
{
    float r = (float)(unsigned long long)(lcg_step(st) - 1u) / 2147483648.0f;
    if (r >= 1.0f) r = 0.99999994f;                              // nextafter(1.0f, 0.0f)
    return r * (1.0f - 0.1f) + 0.1f;
}

// The solver cell of an odd-parity sample, :432-434 (truncation toward zero): false when it lies outside the grid, else
// id = the packed global cell x + y*(W+2) + z*(W+2)*(H+2).
FS_VOX_HD inline bool sample_cell(const VoxParams& q, float px, float py, float pz, int& id)
{
    const int gx = (int)((px - 0.0f) * q.gscale + q.cx + q.tx);
    const int gy = (int)((py - 0.0f) * q.gscale + q.cy + q.ty);
    const int gz = (int)((pz - 0.0f) * q.gscale + q.cz + q.tz);
    if (!(gx >= 1 && gx <= q.W && gy >= 1 && gy <= q.H && gz >= 1 && gz <= q.D)) return false;
    id = gx + gy * (q.W + 2) + gz * (q.W + 2) * (q.H + 2);
    return true;
}

}  // namespace vox
}  // namespace fs
