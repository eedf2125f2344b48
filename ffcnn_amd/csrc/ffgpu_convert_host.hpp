// ffgpu_convert_host.hpp -- the host side of the convert surfaces (include/ffcnn_hip.h: ffgpu_convert_check, ffgpu_convert_tile,
// ffgpu_convert_bgr_dev / _nv12_dev) before anything reaches the device: a source surface checked and its planes resolved, the argument checks, and
// the jobs of a call by source class as the launches take them, each with the form (aligned or general) it runs in.  Plain C++17 with no HIP in it:
// every function reports through ffgpu_set_error and touches no device, so san/convert_driver.cc runs the same lines on the CPU under ASan + UBSan
// (tests/test_convert_abi.py).  The destination descriptors' checks are ffgpu_args.hpp's.
#pragma once
#include <type_traits>
#include <utility>
#include "ffgpu_args.hpp"

static_assert(sizeof(ffgpu_surface) == 56, "include/ffcnn_hip.h states this size");
#define CONVERT_TW        256                         // a workgroup's tile of destination pixels: columns (a wave: 64 lanes of 4 pixels),
#define CONVERT_TH        8                           //   rows (four waves of a row pair)
#define CONVERT_ARG_JOBS  48                          // jobs per launch
// RGB -> YUV by FFGPU_YUV_*: { yoff, yr, yg, yb, ur, ug, ub, vr, vg, vb } (the table of include/ffcnn_hip.h)
#define FFGPU_RGB2YUV_MATRICES { { 16, 66, 129, 25, -38, -74, 112, 112, -94, -18 }, { 0, 77, 150, 29, -43, -85, 128, 128, -107, -21 }, \
                                 { 16, 47, 157, 16, -26, -86, 112, 112, -102, -10 }, { 0, 54, 183, 19, -29, -99, 128, 128, -116, -12 } }

// the source classes k_convert is instantiated for
enum { CONVERT_RGB, CONVERT_GRAY, CONVERT_PLANAR, CONVERT_PAIR, CONVERT_PAIR16, CONVERT_PACKED422, CONVERT_NSRC };
#define CONVERT_SWAP  1                               // ConvertJob::sel: R before B / V before U / U Y0 V Y1
#define CONVERT_BPP4  2                               //   packed RGB of 4 bytes a pixel

// One job as the kernel reads it.  s[1] is the U plane (or the pair plane), s[2] the V plane, whatever the order of the surface's planes.
struct ConvertJob {
    const unsigned char *s[3];    // row 0 of the source planes
    unsigned char *d[2];          // row 0 of the BGR pixels / of the Y plane, and of the U V plane
    int sp[3], dp[2];             // bytes from one row to the next
    int w, h;
    int sel;                      // CONVERT_SWAP | CONVERT_BPP4
    int fmt;                      // 1 + FFGPU_YUV_* of the source (FrameDesc::fmt)
    int aligned;                  // every address and pitch above is a multiple of 4: the aligned form
};
static_assert(sizeof(ConvertJob) == 80, "ConvertJob: CONVERT_ARG_JOBS of them travel by value as k_convert's argument");

struct ConvertFormat { int cls, sel, planes, bytes0; bool pairs0; };    // bytes0: of p[0] per pixel (4:2:2: per pixel pair); pairs0: p[0] holds 16-bit samples
inline const ConvertFormat *ffgpu_convert_format(int format)
{
    static const ConvertFormat F[12] = {
        { CONVERT_RGB, 0, 1, 3, false }, { CONVERT_RGB, CONVERT_SWAP, 1, 3, false }, { CONVERT_RGB, CONVERT_BPP4, 1, 4, false },
        { CONVERT_RGB, CONVERT_SWAP | CONVERT_BPP4, 1, 4, false }, { CONVERT_GRAY, 0, 1, 1, false }, { CONVERT_PAIR, 0, 2, 1, false },
        { CONVERT_PAIR, CONVERT_SWAP, 2, 1, false }, { CONVERT_PLANAR, 0, 3, 1, false }, { CONVERT_PLANAR, CONVERT_SWAP, 3, 1, false },
        { CONVERT_PACKED422, 0, 1, 4, false }, { CONVERT_PACKED422, CONVERT_SWAP, 1, 4, false }, { CONVERT_PAIR16, 0, 2, 2, true } };
    return format >= 0 && format < 12 ? &F[format] : nullptr;
}

// One source surface, job k of the call, for a destination of dw x dh: its fields checked, its defaults resolved into j.s / j.sp / j.w / j.h / j.sel /
// j.fmt.  With a NULL p[0] the addresses are left out (ffgpu_convert_check's form; the operators skip such a job before they come here).
inline int ffgpu_surface_check(const char *what, int k, const ffgpu_surface &s, int dw, int dh, ConvertJob &j)
{
    const ConvertFormat *f = ffgpu_convert_format(s.format);
    if (!f) { ffgpu_set_error("%s: job %d: format %d is none of FFGPU_PIX_* (0..11)", what, k, s.format); return -1; }
    if (s.matrix < 0 || s.matrix > 3) { ffgpu_set_error("%s: job %d: matrix %d is none of FFGPU_YUV_* (0..3)", what, k, s.matrix); return -1; }
    if (s.reserved != 0) { ffgpu_set_error("%s: job %d: surface: reserved must be 0", what, k); return -1; }
    if (s.w < 1 || s.h < 1 || s.w > FFGPU_CONVERT_MAX_SIDE || s.h > FFGPU_CONVERT_MAX_SIDE) {
        ffgpu_set_error("%s: job %d: a source of %d x %d (1..%d each)", what, k, s.w, s.h, FFGPU_CONVERT_MAX_SIDE);
        return -1;
    }
    if (s.w != dw || s.h != dh) { ffgpu_set_error("%s: job %d: a source of %d x %d for a destination of %d x %d", what, k, s.w, s.h, dw, dh); return -1; }
    const int cw = (s.w + 1) / 2, ch = (s.h + 1) / 2;
    // plane n: its least pitch, its rows, and whether it is read as aligned 16-bit values
    const int least[3] = { f->cls == CONVERT_PACKED422 ? 4 * cw : f->bytes0 * s.w, f->cls == CONVERT_PLANAR ? cw : f->cls == CONVERT_PAIR16 ? 4 * cw : 2 * cw, cw };
    const int rows[3] = { s.h, ch, ch };
    const bool pairs[3] = { f->pairs0, f->cls != CONVERT_PLANAR, false };
    const unsigned char *behind = nullptr;
    for (int n = 0; n < 3; n++) {
        if (n >= f->planes) {
            if (s.p[n]) { ffgpu_set_error("%s: job %d: p[%d] must be NULL: format %d has %d plane%s", what, k, n, s.format, f->planes, f->planes > 1 ? "s" : ""); return -1; }
            continue;
        }
        const int pitch = s.pitch[n] ? s.pitch[n] : least[n];
        if (pitch < least[n]) { ffgpu_set_error("%s: job %d: pitch[%d] %d is below %d", what, k, n, s.pitch[n], least[n]); return -1; }
        if (pairs[n] && (pitch & 1)) { ffgpu_set_error("%s: job %d: pitch[%d] %d is odd (plane %d is read as aligned 16-bit values)", what, k, n, s.pitch[n], n); return -1; }
        // (YV12: p[1] is the V plane; the kernel's s[1] is always U)
        const int to = f->cls == CONVERT_PLANAR && (f->sel & CONVERT_SWAP) && n ? 3 - n : n;
        j.sp[to] = pitch;
        if (!s.p[0]) continue;
        const unsigned char *p = s.p[n] ? s.p[n] : behind;
        if (pairs[n] && (reinterpret_cast<uintptr_t>(p) & 1)) {
            ffgpu_set_error("%s: job %d: plane %d's address %p is odd (it is read as aligned 16-bit values)", what, k, n, (const void *)p);
            return -1;
        }
        j.s[to] = p;
        behind = p + (size_t)pitch * (size_t)rows[n];
    }
    j.w = s.w; j.h = s.h; j.fmt = 1 + s.matrix;
    j.sel = f->cls == CONVERT_PLANAR ? 0 : f->sel;
    return 0;
}

inline int ffgpu_convert_check_host(const char *what, const ffgpu_surface *src, int dst_w, int dst_h)
{
    if (!src) { ffgpu_set_error("%s: NULL src", what); return -1; }
    ConvertJob j;
    memset(&j, 0, sizeof j);
    return ffgpu_surface_check(what, 0, *src, dst_w, dst_h, j);
}

// The arguments of a call into its jobs by source class, skipped jobs left out, in job order.  -1 with the job's index in the message.
template <class Frame>
int ffgpu_convert_args_check(const char *what, const ffgpu_surface *srcs, const Frame *dsts, int njobs, std::vector<ConvertJob> (&jobs)[CONVERT_NSRC])
{
    if (!srcs) { ffgpu_set_error("%s: NULL srcs", what); return -1; }
    if (!dsts) { ffgpu_set_error("%s: NULL dsts", what); return -1; }
    if (njobs < 1 || njobs > FFGPU_CONVERT_MAX_JOBS) { ffgpu_set_error("%s: %d jobs (1..%d)", what, njobs, FFGPU_CONVERT_MAX_JOBS); return -1; }
    std::vector<DrawTarget> dt;
    if (ffgpu_frame_table(what, FRAME_DRAW, dsts, njobs, dt)) return -1;
    for (auto &v : jobs) v.clear();
    std::vector<std::pair<const unsigned char *, int>> written;
    for (int k = 0; k < njobs; k++) {
        const DrawTarget &d = dt[(size_t)k];
        if (!srcs[k].p[0] || !d.p0) continue;                                         // a skipped job: its surface is not looked at
        ConvertJob j;
        memset(&j, 0, sizeof j);
        if (ffgpu_surface_check(what, k, srcs[k], d.w, d.h, j)) return -1;
        j.d[0] = d.p0; j.d[1] = d.p1; j.dp[0] = d.pitch; j.dp[1] = d.pitch_uv;
        uintptr_t bits = 0;
        for (int n = 0; n < 3; n++) {
            if (!j.s[n]) continue;
            if (j.s[n] == j.d[0] || j.s[n] == j.d[1]) { ffgpu_set_error("%s: job %d: a source plane and a destination plane are the same address %p", what, k, (const void *)j.s[n]); return -1; }
            bits |= reinterpret_cast<uintptr_t>(j.s[n]) | (uintptr_t)j.sp[n];
        }
        for (int n = 0; n < 2; n++) if (j.d[n]) bits |= reinterpret_cast<uintptr_t>(j.d[n]) | (uintptr_t)j.dp[n];
        j.aligned = (bits & 3) == 0;
        written.push_back(std::make_pair((const unsigned char *)d.p0, k));
        jobs[ffgpu_convert_format(srcs[k].format)->cls].push_back(j);
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
inline unsigned ffgpu_convert_tiles(const ConvertJob *j, int n) { return ffgpu_most_tiles(j, n, CONVERT_TW, CONVERT_TH, &ConvertJob::w, &ConvertJob::h); }
