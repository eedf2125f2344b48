// ffgpu_warp_host.hpp -- the host side of the warp surfaces (include/ffcnn_hip.h: ffgpu_warp_spec_check, ffgpu_warp_mesh_size, ffgpu_warp_mesh_orient,
// ffgpu_warp_mesh_homography, ffgpu_warp_mesh_lens, ffgpu_warp_point, ffgpu_warp_tile, ffgpu_warp_bgr_dev / _nv12_dev) before anything reaches the
// device: the spec's check, the mesh builders, the interpolation rule for one pixel, the argument checks, and the planes of a call as the jobs the
// launches take.  Plain C++17 with no HIP in it: every function reports through ffgpu_set_error and touches no device, so san/warp_driver.cc runs
// the same lines on the CPU under ASan + UBSan (tests/test_warp_abi.py).  The frame descriptors' checks are ffgpu_args.hpp's.
#pragma once
#include <math.h>
#include <limits.h>
#include <type_traits>
#include <utility>
#include "ffgpu_args.hpp"

static_assert(sizeof(ffgpu_warp_mesh) == 24 && sizeof(ffgpu_warp_spec) == 16 && sizeof(ffgpu_warp_lens) == 120, "include/ffcnn_hip.h states these sizes");
#define WARP_TW        64                             // a workgroup's tile of destination pixels: columns,
#define WARP_TH        16                             //   rows
#define WARP_ARG_JOBS  64                             // jobs per launch
#define WARP_STAGED_CH 3                              // the planes that have a staged form: BGR (the Y and the U V plane are always read directly)
#define WARP_LDS_BYTES 16384                         // what the staged form may fill: a tile whose clipped source box needs more reads global memory directly

static const FrameRole FRAME_WARP_SRC = { "source", false, "read", 0x3fffffff }, FRAME_WARP_DST = { "destination", false, "written", 0x3fffffff };

// One plane of one job as the kernel reads it: CH interleaved channels (BGR: 3; NV12: the Y plane 1, the U V plane 2), sizes in SAMPLES of the plane.
// half = 1 (the U V plane): destination sample (i, j) takes the mesh at luma pixel (2 i, 2 j) and halves the position.
struct WarpJob {
    const unsigned char *src;     // row 0 of the source plane
    unsigned char *dst;           // row 0 of the destination plane
    const int *xy;                // the mesh, rows of mw (x, y) pairs
    int spitch, dpitch;           // bytes from one row to the next
    int sw, sh;                   // the source plane: no load reaches outside its sw x sh samples
    int dw, dh;                   // the destination plane
    int mw;                       // points in a mesh row
    int shift;                    // s, the cell's log2, in bits 0..7; half in bit 8
};
static_assert(sizeof(WarpJob) == 56, "WarpJob: WARP_ARG_JOBS of them travel by value as k_warp's argument");

inline int ffgpu_warp_spec_check_host(const char *what, const ffgpu_warp_spec *sp)
{
    if (!sp) { ffgpu_set_error("%s: NULL spec", what); return -1; }
    if (sp->filter != FFGPU_WARP_BILINEAR && sp->filter != FFGPU_WARP_NEAREST) { ffgpu_set_error("%s: filter %d is neither FFGPU_WARP_BILINEAR nor FFGPU_WARP_NEAREST", what, sp->filter); return -1; }
    if (sp->border != FFGPU_WARP_FILL && sp->border != FFGPU_WARP_CLAMP) { ffgpu_set_error("%s: border %d is neither FFGPU_WARP_FILL nor FFGPU_WARP_CLAMP", what, sp->border); return -1; }
    if (sp->fill[3] != 0) { ffgpu_set_error("%s: fill[3] must be 0", what); return -1; }
    if (sp->reserved != 0) { ffgpu_set_error("%s: spec: reserved must be 0", what); return -1; }
    return 0;
}

// s of a cell c = 1 << s, or -1
inline int ffgpu_warp_cell_log2(int cell) { return cell == 8 ? 3 : cell == 16 ? 4 : cell == 32 ? 5 : cell == 64 ? 6 : -1; }

inline int ffgpu_warp_mesh_size_host(const char *what, int dst_w, int dst_h, int cell, int out[2])
{
    if (!out) { ffgpu_set_error("%s: NULL out", what); return -1; }
    if (dst_w < 1 || dst_h < 1 || dst_w > FFGPU_WARP_MAX_SIDE || dst_h > FFGPU_WARP_MAX_SIDE) {
        ffgpu_set_error("%s: a destination of %d x %d (1..%d each)", what, dst_w, dst_h, FFGPU_WARP_MAX_SIDE);
        return -1;
    }
    if (ffgpu_warp_cell_log2(cell) < 0) { ffgpu_set_error("%s: cell %d is none of 8, 16, 32, 64", what, cell); return -1; }
    out[0] = (dst_w - 1) / cell + 2; out[1] = (dst_h - 1) / cell + 2;
    return 0;
}

// floor(v * 256 + 0.5) saturated to int32; INT32_MIN for a value that is not finite
inline int ffgpu_warp_fix(double v)
{
    if (!isfinite(v)) return INT_MIN;
    const double t = floor(v * 256.0 + 0.5);
    return t <= -2147483648.0 ? INT_MIN : t >= 2147483647.0 ? INT_MAX : (int)t;
}

inline int ffgpu_warp_mesh_orient_host(const char *what, int src_w, int src_h, int orient, int cell, int out_dst_wh[2], int *xy)
{
    if (!out_dst_wh) { ffgpu_set_error("%s: NULL out_dst_wh", what); return -1; }
    if (src_w < 1 || src_h < 1 || src_w > FFGPU_WARP_MAX_SIDE || src_h > FFGPU_WARP_MAX_SIDE) {
        ffgpu_set_error("%s: a source of %d x %d (1..%d each)", what, src_w, src_h, FFGPU_WARP_MAX_SIDE);
        return -1;
    }
    if (orient < 0 || orient > 7) { ffgpu_set_error("%s: orient %d (0..7)", what, orient); return -1; }
    const int dw = (orient & 1) ? src_h : src_w, dh = (orient & 1) ? src_w : src_h;
    int m[2];
    if (ffgpu_warp_mesh_size_host(what, dw, dh, cell, m)) return -1;
    out_dst_wh[0] = dw; out_dst_wh[1] = dh;
    if (!xy) return 0;
    // x = ax i + bx j + cx, y = ay i + by j + cy: the table of include/ffcnn_hip.h
    const int W1 = src_w - 1, H1 = src_h - 1;
    static const signed char T[8][6] = { // ax bx cx(W1)  ay by cy(H1)
        { 1, 0, 0, 0, 1, 0 }, { 0, 1, 0, -1, 0, 1 }, { -1, 0, 1, 0, -1, 1 }, { 0, -1, 1, 1, 0, 0 },
        { -1, 0, 1, 0, 1, 0 }, { 0, -1, 1, -1, 0, 1 }, { 1, 0, 0, 0, -1, 1 }, { 0, 1, 0, 1, 0, 0 } };
    const signed char *t = T[orient];
    for (int cj = 0; cj < m[1]; cj++)
        for (int ci = 0; ci < m[0]; ci++) {
            const int i = ci * cell, j = cj * cell;                                    // (at most 8192 + 63: the products below stay far inside int32)
            int *p = xy + 2 * ((size_t)cj * (size_t)m[0] + (size_t)ci);
            p[0] = FFGPU_WARP_MESH_ONE * (t[0] * i + t[1] * j + t[2] * W1);
            p[1] = FFGPU_WARP_MESH_ONE * (t[3] * i + t[4] * j + t[5] * H1);
        }
    return 0;
}

// (doubles in the order written: no contraction into fused multiply-adds, where the compiler knows the pragma)
inline int ffgpu_warp_mesh_homography_host(const char *what, int dst_w, int dst_h, int cell, const double h[9], int *xy)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    int m[2];
    if (ffgpu_warp_mesh_size_host(what, dst_w, dst_h, cell, m)) return -1;
    if (!h) { ffgpu_set_error("%s: NULL h", what); return -1; }
    if (!xy) { ffgpu_set_error("%s: NULL xy", what); return -1; }
    for (int cj = 0; cj < m[1]; cj++)
        for (int ci = 0; ci < m[0]; ci++) {
            const double i = (double)(ci * cell), j = (double)(cj * cell);
            const double den = (h[6] * i + h[7] * j) + h[8];
            int *p = xy + 2 * ((size_t)cj * (size_t)m[0] + (size_t)ci);
            if (!(den > 0.0)) { p[0] = p[1] = INT_MIN; continue; }
            p[0] = ffgpu_warp_fix(((h[0] * i + h[1] * j) + h[2]) / den);
            p[1] = ffgpu_warp_fix(((h[3] * i + h[4] * j) + h[5]) / den);
        }
    return 0;
}

inline int ffgpu_warp_mesh_lens_host(const char *what, int dst_w, int dst_h, int cell, const ffgpu_warp_lens *lens, int *xy)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    int m[2];
    if (ffgpu_warp_mesh_size_host(what, dst_w, dst_h, cell, m)) return -1;
    if (!lens) { ffgpu_set_error("%s: NULL lens", what); return -1; }
    if (!xy) { ffgpu_set_error("%s: NULL xy", what); return -1; }
    if (lens->model != FFGPU_WARP_LENS_BROWN && lens->model != FFGPU_WARP_LENS_EQUIDISTANT) {
        ffgpu_set_error("%s: model %d is neither FFGPU_WARP_LENS_BROWN nor FFGPU_WARP_LENS_EQUIDISTANT", what, lens->model);
        return -1;
    }
    if (lens->reserved != 0) { ffgpu_set_error("%s: lens: reserved must be 0", what); return -1; }
    if (!(isfinite(lens->dst[0]) && isfinite(lens->dst[1]) && lens->dst[0] > 0.0 && lens->dst[1] > 0.0)) {
        ffgpu_set_error("%s: the destination's fx %g and fy %g must be finite and above 0", what, lens->dst[0], lens->dst[1]);
        return -1;
    }
    const double *k = lens->k, *pt = lens->p;
    for (int cj = 0; cj < m[1]; cj++)
        for (int ci = 0; ci < m[0]; ci++) {
            const double i = (double)(ci * cell), j = (double)(cj * cell);
            const double xn = (i - lens->dst[2]) / lens->dst[0], yn = (j - lens->dst[3]) / lens->dst[1];
            const double r2 = xn * xn + yn * yn;
            double xd, yd;
            if (lens->model == FFGPU_WARP_LENS_BROWN) {
                const double rad = 1.0 + ((k[2] * r2 + k[1]) * r2 + k[0]) * r2;
                xd = xn * rad + ((2.0 * pt[0]) * (xn * yn) + pt[1] * (r2 + (2.0 * xn) * xn));
                yd = yn * rad + (pt[0] * (r2 + (2.0 * yn) * yn) + (2.0 * pt[1]) * (xn * yn));
            } else {
                const double r = sqrt(r2), theta = atan(r), t2 = theta * theta;
                const double theta_d = theta * (1.0 + ((((k[3] * t2 + k[2]) * t2 + k[1]) * t2 + k[0]) * t2));
                const double scale = r > 0.0 ? theta_d / r : 1.0;
                xd = xn * scale; yd = yn * scale;
            }
            int *p = xy + 2 * ((size_t)cj * (size_t)m[0] + (size_t)ci);
            p[0] = ffgpu_warp_fix(lens->src[0] * xd + lens->src[2]);
            p[1] = ffgpu_warp_fix(lens->src[1] * yd + lens->src[3]);
        }
    return 0;
}

// The interpolation rule of the contract for one coordinate: the four points' values, a and b inside a cell of 1 << s.  The four weights are
// (c - a)(c - b), a (c - b), (c - a) b, a b: the same sum as the contract's nested form, in exact 64-bit integers (below 2^43).
inline long long ffgpu_warp_interp(int p00, int p10, int p01, int p11, int a, int b, int s)
{
    const long long c = 1LL << s;
    const long long S = (c - b) * ((c - a) * (long long)p00 + a * (long long)p10) + b * ((c - a) * (long long)p01 + a * (long long)p11);
    return (S + (1LL << (2 * s - 1))) >> (2 * s);
}

// a mesh descriptor against its destination; job k of the call in the message
inline int ffgpu_warp_mesh_check(const char *what, int k, const ffgpu_warp_mesh &m, int dst_w, int dst_h)
{
    if (m.reserved != 0) { ffgpu_set_error("%s: job %d: mesh: reserved must be 0", what, k); return -1; }
    if (ffgpu_warp_cell_log2(m.cell) < 0) { ffgpu_set_error("%s: job %d: mesh: cell %d is none of 8, 16, 32, 64", what, k, m.cell); return -1; }
    if (!m.xy) { ffgpu_set_error("%s: job %d: mesh: NULL xy", what, k); return -1; }
    if (reinterpret_cast<uintptr_t>(m.xy) & 7) { ffgpu_set_error("%s: job %d: mesh: xy %p is not 8-byte aligned", what, k, (const void *)m.xy); return -1; }
    const int mw = (dst_w - 1) / m.cell + 2, mh = (dst_h - 1) / m.cell + 2;
    if (m.mw != mw || m.mh != mh) {
        ffgpu_set_error("%s: job %d: mesh: %d x %d points, a destination of %d x %d with cells of %d has %d x %d", what, k, m.mw, m.mh, dst_w, dst_h, m.cell, mw, mh);
        return -1;
    }
    return 0;
}

inline int ffgpu_warp_point_host(const char *what, const ffgpu_warp_mesh *mesh, int dst_w, int dst_h, int i, int j, int out[2])
{
    if (!mesh) { ffgpu_set_error("%s: NULL mesh", what); return -1; }
    if (!out) { ffgpu_set_error("%s: NULL out", what); return -1; }
    if (dst_w < 1 || dst_h < 1 || dst_w > FFGPU_WARP_MAX_SIDE || dst_h > FFGPU_WARP_MAX_SIDE) {
        ffgpu_set_error("%s: a destination of %d x %d (1..%d each)", what, dst_w, dst_h, FFGPU_WARP_MAX_SIDE);
        return -1;
    }
    if (ffgpu_warp_mesh_check(what, 0, *mesh, dst_w, dst_h)) return -1;
    if (i < 0 || j < 0 || i >= dst_w || j >= dst_h) { ffgpu_set_error("%s: pixel (%d, %d) is outside the destination of %d x %d", what, i, j, dst_w, dst_h); return -1; }
    const int s = ffgpu_warp_cell_log2(mesh->cell), c = mesh->cell;
    const int *p = mesh->xy + 2 * ((size_t)(j >> s) * (size_t)mesh->mw + (size_t)(i >> s)), *q = p + 2 * (size_t)mesh->mw;
    out[0] = (int)ffgpu_warp_interp(p[0], p[2], q[0], q[2], i & (c - 1), j & (c - 1), s);
    out[1] = (int)ffgpu_warp_interp(p[1], p[3], q[1], q[3], i & (c - 1), j & (c - 1), s);
    return 0;
}

// The arguments of a call into the jobs of its planes: jobs[0] the BGR planes or the Y planes, jobs[1] the U V planes, skipped jobs left out, in
// job order.  -1 with the job's index in the message.
template <class Frame>
int ffgpu_warp_args_check(const char *what, const Frame *srcs, const Frame *dsts, const ffgpu_warp_mesh *meshes, int njobs, const ffgpu_warp_spec *spec,
                          std::vector<WarpJob> (&jobs)[2])
{
    const bool nv12 = std::is_same<Frame, ffgpu_nv12_frame>::value;
    if (!srcs) { ffgpu_set_error("%s: NULL srcs", what); return -1; }
    if (!dsts) { ffgpu_set_error("%s: NULL dsts", what); return -1; }
    if (!meshes) { ffgpu_set_error("%s: NULL meshes", what); return -1; }
    if (ffgpu_warp_spec_check_host(what, spec)) return -1;
    if (njobs < 1 || njobs > FFGPU_WARP_MAX_JOBS) { ffgpu_set_error("%s: %d jobs (1..%d)", what, njobs, FFGPU_WARP_MAX_JOBS); return -1; }
    std::vector<DrawTarget> st, dt;
    if (ffgpu_frame_table(what, FRAME_WARP_SRC, srcs, njobs, st) || ffgpu_frame_table(what, FRAME_WARP_DST, dsts, njobs, dt)) return -1;
    jobs[0].clear(); jobs[1].clear();
    std::vector<std::pair<const unsigned char *, int>> written;
    for (int k = 0; k < njobs; k++) {
        const DrawTarget &s = st[(size_t)k], &d = dt[(size_t)k];
        if (!s.p0 || !d.p0) continue;                                                 // a skipped job: its sizes and its mesh are not looked at
        if (s.w > FFGPU_WARP_MAX_SIDE || s.h > FFGPU_WARP_MAX_SIDE) { ffgpu_set_error("%s: job %d: a source of %d x %d (1..%d each)", what, k, s.w, s.h, FFGPU_WARP_MAX_SIDE); return -1; }
        if (d.w > FFGPU_WARP_MAX_SIDE || d.h > FFGPU_WARP_MAX_SIDE) { ffgpu_set_error("%s: job %d: a destination of %d x %d (1..%d each)", what, k, d.w, d.h, FFGPU_WARP_MAX_SIDE); return -1; }
        if (ffgpu_warp_mesh_check(what, k, meshes[k], d.w, d.h)) return -1;
        if (s.p0 == d.p0) { ffgpu_set_error("%s: job %d: the source and the destination are the same pixels", what, k); return -1; }
        written.push_back(std::make_pair((const unsigned char *)d.p0, k));
        WarpJob j;
        memset(&j, 0, sizeof j);
        j.xy = meshes[k].xy; j.mw = meshes[k].mw; j.shift = ffgpu_warp_cell_log2(meshes[k].cell);
        j.src = s.p0; j.dst = d.p0; j.spitch = s.pitch; j.dpitch = d.pitch; j.sw = s.w; j.sh = s.h; j.dw = d.w; j.dh = d.h;
        jobs[0].push_back(j);
        if (!nv12) continue;
        // the U V plane: two channels at half the size; chroma sample (i, j) takes the mesh at luma pixel (2 i, 2 j)
        j.src = s.p1; j.dst = d.p1; j.spitch = s.pitch_uv; j.dpitch = d.pitch_uv; j.sw = (s.w + 1) / 2; j.sh = (s.h + 1) / 2; j.dw = (d.w + 1) / 2; j.dh = (d.h + 1) / 2;
        j.shift |= 1 << 8;
        jobs[1].push_back(j);
    }
    std::sort(written.begin(), written.end());
    for (size_t n = 1; n < written.size(); n++)
        if (written[n].first == written[n - 1].first) {
            ffgpu_set_error("%s: jobs %d and %d have the same destination", what, written[n - 1].second, written[n].second);
            return -1;
        }
    return 0;
}

// the tiles of the job with the most of them: the launch's grid
inline unsigned ffgpu_warp_tiles(const WarpJob *j, int n)
{
    unsigned most = 1;
    for (int i = 0; i < n; i++) most = std::max(most, (unsigned)(((j[i].dw + WARP_TW - 1) / WARP_TW) * ((j[i].dh + WARP_TH - 1) / WARP_TH)));
    return most;
}
