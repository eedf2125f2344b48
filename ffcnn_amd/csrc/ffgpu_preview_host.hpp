// ffgpu_preview_host.hpp -- the host side of the preview surfaces (include/ffcnn_hip.h: ffgpu_preview_spec_check, ffgpu_preview_rect,
// ffgpu_preview_grid, ffgpu_preview_tile, ffgpu_preview_bgr_dev / _nv12_dev) before anything reaches the device: the spec's check, a pane resolved
// into its source region, image and bars, the wall's layout, the argument checks with the overlap test, and the planes of a call as the jobs the
// launches take.  Plain C++17 with no HIP in it: every function reports through ffgpu_set_error and touches no device, so san/preview_driver.cc runs
// the same lines on the CPU under ASan + UBSan (tests/test_preview_abi.py).  The frame descriptors' checks are ffgpu_args.hpp's.
#pragma once
#include <type_traits>
#include "ffgpu_args.hpp"

static_assert(sizeof(ffgpu_preview_pane) == 32 && sizeof(ffgpu_preview_spec) == 16, "include/ffcnn_hip.h states these sizes");
#define PREVIEW_TW        64                          // a workgroup's tile of destination samples: columns,
#define PREVIEW_TH        16                          //   rows
#define PREVIEW_ARG_JOBS  32                          // planes per launch

static const FrameRole FRAME_PREVIEW_SRC = { "source", false, "read", 0x3fffffff }, FRAME_PREVIEW_DST = { "destination", false, "written", 0x3fffffff };

// One plane of one pane as the kernel reads it: CH interleaved channels (BGR: 3; NV12: the Y plane 1, the U V plane 2), every number in SAMPLES of the
// plane.  The image is ow x oh samples at (ix, iy) of the destination plane, the pane pw x ph at (px, py) around it.
struct PreviewJob {
    const unsigned char *src;     // row 0 of the source plane
    unsigned char *dst;           // row 0 of the destination plane
    int spitch, dpitch;           // bytes from one row to the next
    int srow;                     // bytes of a source row that belong to the frame: no load reaches outside them
    int sx, sy, sw, sh;           // the source region
    int px, py, pw, ph;           // the pane
    int ix, iy, ow, oh;           // the image
    unsigned fill;                // the bars' sample: channel c in bits 8 c .. 8 c + 7
    int keep;                     // the bars are not written
    int pane;                     // the pane's index in the call
};
static_assert(sizeof(PreviewJob) == 88, "PreviewJob: PREVIEW_ARG_JOBS of them travel by value as k_preview's argument");

inline int ffgpu_preview_spec_check_host(const char *what, const ffgpu_preview_spec *sp)
{
    if (!sp) { ffgpu_set_error("%s: NULL spec", what); return -1; }
    if (sp->fit != FFGPU_PREVIEW_STRETCH && sp->fit != FFGPU_PREVIEW_FIT) { ffgpu_set_error("%s: fit %d is neither FFGPU_PREVIEW_STRETCH nor FFGPU_PREVIEW_FIT", what, sp->fit); return -1; }
    if (sp->flags & ~FFGPU_PREVIEW_KEEP_BARS) { ffgpu_set_error("%s: unknown flags 0x%x", what, (unsigned)sp->flags); return -1; }
    if (sp->fill[3] != 0) { ffgpu_set_error("%s: fill[3] must be 0", what); return -1; }
    if (sp->reserved != 0) { ffgpu_set_error("%s: spec: reserved must be 0", what); return -1; }
    return 0;
}

// RESOLVE of the contract: out = { sx, sy, sw, sh, X0, Y0, ow, oh }; pane k of the call in the message
inline int ffgpu_preview_resolve(const char *what, int k, int src_w, int src_h, int dst_w, int dst_h, const ffgpu_preview_pane &p, int fit, bool nv12, int out[8])
{
    int sx = p.sx, sy = p.sy, sw = p.sw, sh = p.sh, dx = p.dx, dy = p.dy, dw = p.dw, dh = p.dh;
    if ((sw == 0) != (sh == 0)) { ffgpu_set_error("%s: pane %d: a source region of %d x %d (both 0 for the whole frame, or neither)", what, k, sw, sh); return -1; }
    if ((dw == 0) != (dh == 0)) { ffgpu_set_error("%s: pane %d: a pane of %d x %d (both 0 for the whole surface, or neither)", what, k, dw, dh); return -1; }
    if (sw == 0) {
        if (sx != 0 || sy != 0) { ffgpu_set_error("%s: pane %d: the whole frame as the source region wants sx = sy = 0, not (%d, %d)", what, k, sx, sy); return -1; }
        sw = src_w; sh = src_h;
    }
    if (dw == 0) {
        if (dx != 0 || dy != 0) { ffgpu_set_error("%s: pane %d: the whole surface as the pane wants dx = dy = 0, not (%d, %d)", what, k, dx, dy); return -1; }
        dw = dst_w; dh = dst_h;
    }
    if (sw < 1 || sh < 1 || sw > FFGPU_PREVIEW_MAX_SIDE || sh > FFGPU_PREVIEW_MAX_SIDE) {
        ffgpu_set_error("%s: pane %d: a source region of %d x %d (1..%d each)", what, k, sw, sh, FFGPU_PREVIEW_MAX_SIDE);
        return -1;
    }
    if (dw < 1 || dh < 1 || dw > FFGPU_PREVIEW_MAX_SIDE || dh > FFGPU_PREVIEW_MAX_SIDE) {
        ffgpu_set_error("%s: pane %d: a pane of %d x %d (1..%d each)", what, k, dw, dh, FFGPU_PREVIEW_MAX_SIDE);
        return -1;
    }
    if (sx < 0 || sy < 0 || (long long)sx + sw > src_w || (long long)sy + sh > src_h) {
        ffgpu_set_error("%s: pane %d: the source region %d x %d at (%d, %d) is outside the frame of %d x %d", what, k, sw, sh, sx, sy, src_w, src_h);
        return -1;
    }
    if (dx < 0 || dy < 0 || (long long)dx + dw > dst_w || (long long)dy + dh > dst_h) {
        ffgpu_set_error("%s: pane %d: the pane %d x %d at (%d, %d) is outside the surface of %d x %d", what, k, dw, dh, dx, dy, dst_w, dst_h);
        return -1;
    }
    if (nv12 && ((sx | sy | dx | dy) & 1)) { ffgpu_set_error("%s: pane %d: NV12 wants even sx, sy, dx, dy, not (%d, %d) and (%d, %d)", what, k, sx, sy, dx, dy); return -1; }
    int ow = dw, oh = dh;
    if (fit == FFGPU_PREVIEW_FIT) {
        const long long SW = sw, SH = sh, DW = dw, DH = dh;
        if (SW * DH >= SH * DW) oh = (int)std::min<long long>(std::max<long long>((2 * SH * DW + SW) / (2 * SW), 1), DH);
        else                    ow = (int)std::min<long long>(std::max<long long>((2 * SW * DH + SH) / (2 * SH), 1), DW);
    }
    int ox = (dw - ow) >> 1, oy = (dh - oh) >> 1;
    if (nv12) { ox &= ~1; oy &= ~1; }
    out[0] = sx; out[1] = sy; out[2] = sw; out[3] = sh; out[4] = dx + ox; out[5] = dy + oy; out[6] = ow; out[7] = oh;
    return 0;
}

inline int ffgpu_preview_rect_host(const char *what, int src_w, int src_h, int dst_w, int dst_h, const ffgpu_preview_pane *pane, const ffgpu_preview_spec *spec, int nv12, int out[8])
{
    if (!pane) { ffgpu_set_error("%s: NULL pane", what); return -1; }
    if (!out) { ffgpu_set_error("%s: NULL out", what); return -1; }
    if (ffgpu_preview_spec_check_host(what, spec)) return -1;
    if (src_w < 1 || src_h < 1 || dst_w < 1 || dst_h < 1) { ffgpu_set_error("%s: a frame of %d x %d into a surface of %d x %d", what, src_w, src_h, dst_w, dst_h); return -1; }
    return ffgpu_preview_resolve(what, 0, src_w, src_h, dst_w, dst_h, *pane, spec->fit, nv12 != 0, out);
}

inline int ffgpu_preview_grid_host(const char *what, int npanes, int cols, int dst_w, int dst_h, int gap, int nv12, ffgpu_preview_pane *out)
{
    if (!out) { ffgpu_set_error("%s: NULL out", what); return -1; }
    if (npanes < 1 || cols < 1 || cols > npanes) { ffgpu_set_error("%s: %d panes in %d columns (both from 1, cols <= npanes)", what, npanes, cols); return -1; }
    if (gap < 0 || (nv12 && (gap & 1))) { ffgpu_set_error("%s: gap %d (from 0%s)", what, gap, nv12 ? ", even for NV12" : ""); return -1; }
    const long long rows = ((long long)npanes + cols - 1) / cols;
    long long cw = ((long long)dst_w - ((long long)cols + 1) * gap) / cols, ch = ((long long)dst_h - (rows + 1) * gap) / rows;
    if (nv12) { cw &= ~1LL; ch &= ~1LL; }
    if (cw < 1 || ch < 1) { ffgpu_set_error("%s: %d x %lld panes with gap %d leave no room in %d x %d", what, cols, rows, gap, dst_w, dst_h); return -1; }
    for (int k = 0; k < npanes; k++) {
        memset(&out[k], 0, sizeof out[k]);
        out[k].dx = (int)(gap + (k % cols) * (cw + gap)); out[k].dy = (int)(gap + (k / cols) * (ch + gap)); out[k].dw = (int)cw; out[k].dh = (int)ch;
    }
    return 0;
}

// The arguments of a call into the jobs of its planes: jobs[0] the BGR planes or the Y planes, jobs[1] the U V planes, skipped panes left out, in
// pane order.  -1 with the pane's index in the message.
template <class Frame>
int ffgpu_preview_args_check(const char *what, const Frame *srcs, const Frame *dsts, const ffgpu_preview_pane *panes, int npanes, const ffgpu_preview_spec *spec,
                             std::vector<PreviewJob> (&jobs)[2])
{
    const bool nv12 = std::is_same<Frame, ffgpu_nv12_frame>::value;
    if (!srcs) { ffgpu_set_error("%s: NULL srcs", what); return -1; }
    if (!dsts) { ffgpu_set_error("%s: NULL dsts", what); return -1; }
    if (!panes) { ffgpu_set_error("%s: NULL panes", what); return -1; }
    if (ffgpu_preview_spec_check_host(what, spec)) return -1;
    if (npanes < 1 || npanes > FFGPU_PREVIEW_MAX_PANES) { ffgpu_set_error("%s: %d panes (1..%d)", what, npanes, FFGPU_PREVIEW_MAX_PANES); return -1; }
    std::vector<DrawTarget> st, dt;
    if (ffgpu_frame_table(what, FRAME_PREVIEW_SRC, srcs, npanes, st) || ffgpu_frame_table(what, FRAME_PREVIEW_DST, dsts, npanes, dt)) return -1;
    jobs[0].clear(); jobs[1].clear();
    struct Rect { const unsigned char *p; int k, x0, y0, x1, y1; };
    std::vector<Rect> rects;
    const int keep = (spec->flags & FFGPU_PREVIEW_KEEP_BARS) != 0;
    for (int k = 0; k < npanes; k++) {
        const DrawTarget &s = st[(size_t)k], &d = dt[(size_t)k];
        if (!s.p0 || !d.p0) continue;                                                 // a skipped pane: its sizes are not looked at
        if (s.p0 == d.p0) { ffgpu_set_error("%s: pane %d: the source and the destination are the same pixels", what, k); return -1; }
        int r[8];
        if (ffgpu_preview_resolve(what, k, s.w, s.h, d.w, d.h, panes[k], spec->fit, nv12, r)) return -1;
        const int dw = panes[k].dw ? panes[k].dw : d.w, dh = panes[k].dh ? panes[k].dh : d.h, dx = panes[k].dx, dy = panes[k].dy;
        for (const Rect &o : rects)
            if (o.p == d.p0 && dx < o.x1 && o.x0 < dx + dw && dy < o.y1 && o.y0 < dy + dh) {
                ffgpu_set_error("%s: panes %d and %d overlap in one destination surface", what, o.k, k);
                return -1;
            }
        rects.push_back(Rect{ d.p0, k, dx, dy, dx + dw, dy + dh });
        PreviewJob j;
        memset(&j, 0, sizeof j);
        j.keep = keep; j.pane = k;
        if (!nv12) {
            j.src = s.p0; j.dst = d.p0; j.spitch = s.pitch; j.dpitch = d.pitch; j.srow = 3 * s.w;
            j.sx = r[0]; j.sy = r[1]; j.sw = r[2]; j.sh = r[3]; j.px = dx; j.py = dy; j.pw = dw; j.ph = dh; j.ix = r[4]; j.iy = r[5]; j.ow = r[6]; j.oh = r[7];
            j.fill = ffgpu_pack_colour(spec->fill);
            jobs[0].push_back(j);
            continue;
        }
        j.src = s.p0; j.dst = d.p0; j.spitch = s.pitch; j.dpitch = d.pitch; j.srow = s.w;
        j.sx = r[0]; j.sy = r[1]; j.sw = r[2]; j.sh = r[3]; j.px = dx; j.py = dy; j.pw = dw; j.ph = dh; j.ix = r[4]; j.iy = r[5]; j.ow = r[6]; j.oh = r[7];
        j.fill = spec->fill[0];
        jobs[0].push_back(j);
        // the U V plane: two channels at half the size; chroma sample (i, j) belongs to the pane, and to its image, that holds luma pixel (2 i, 2 j)
        j.src = s.p1; j.dst = d.p1; j.spitch = s.pitch_uv; j.dpitch = d.pitch_uv; j.srow = 2 * ((s.w + 1) / 2);
        j.sx = r[0] / 2; j.sy = r[1] / 2; j.sw = (r[2] + 1) / 2; j.sh = (r[3] + 1) / 2; j.px = dx / 2; j.py = dy / 2; j.pw = (dw + 1) / 2; j.ph = (dh + 1) / 2;
        j.ix = r[4] / 2; j.iy = r[5] / 2; j.ow = (r[6] + 1) / 2; j.oh = (r[7] + 1) / 2;
        j.fill = (unsigned)spec->fill[1] | (unsigned)spec->fill[2] << 8;
        jobs[1].push_back(j);
    }
    return 0;
}

// the tiles of the job with the most of them: the launch's grid
inline unsigned ffgpu_preview_tiles(const PreviewJob *j, int n)
{
    unsigned most = 1;
    for (int i = 0; i < n; i++) most = std::max(most, (unsigned)(((j[i].pw + PREVIEW_TW - 1) / PREVIEW_TW) * ((j[i].ph + PREVIEW_TH - 1) / PREVIEW_TH)));
    return most;
}
