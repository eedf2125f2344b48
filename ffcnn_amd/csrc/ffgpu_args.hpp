// ffgpu_args.hpp -- what the entry points of include/ffcnn_hip.h make of their arguments before anything reaches the device: the caller's frame
// descriptors checked and their defaults resolved, and where a post-pass finds its boxes.  Plain C++17 with no HIP in it: every function reports
// through ffgpu_set_error and touches no device, so san/args_driver.cc runs the same lines on the CPU under ASan + UBSan (tests/test_args_host.py).
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "ffcnn_hip.h"

extern "C" void ffgpu_set_error(const char *fmt, ...);

// -------------------------------------------------------------------------- frames
// One frame of ffgpu_exec_forward_bgr_frames_dev / ffgpu_exec_forward_nv12_frames_dev as the kernels read it: the caller's descriptor plus
// net_input's letterbox arithmetic (ffcnn.c:267-273), computed once on the host.  The executor keeps a device table of `batch` of them.
// fmt tells the two kinds of table apart (a BGR table never compares equal to an NV12 one: the executor's "table already sent" shortcut).
struct FrameDesc {
    const unsigned char *bgr;     // row 0 of the frame (any byte alignment); NV12: row 0 of the Y plane
    int w, h, pitch;              // pitch: bytes from one row to the next (>= 3 w; NV12: of the Y plane, >= w)
    int sw, sh, s1, s2;           // the frame fills the top-left sw x sh of the net's plane; source pixel of (x, y) = (x s1 / s2, y s1 / s2)
    int fmt;                      // 0: u8 BGR; 1 + FFGPU_YUV_*: NV12 converted with that matrix
    const unsigned char *uv;      // NV12: row 0 of the interleaved U V plane (2-byte aligned, never NULL here); BGR: NULL
    int pitch_uv;                 // NV12: bytes from one U V row to the next (even)
    int pad_;
};
static_assert(sizeof(FrameDesc) == 56, "FrameDesc: 64 of them travel by value as k_set_frames' argument");

// the detections drawn into the frames (ffgpu_draw.inc) or redacted in them (ffgpu_redact.inc).  One target as the kernel reads it: the caller's descriptor with its defaults resolved, and
// the first box of its list (in boxes from the lists' base; unused when the records' own boxes are drawn).  p0 == NULL: a skipped target.
struct DrawTarget {
    unsigned char *p0;            // row 0 of the BGR pixels / of the Y plane
    unsigned char *p1;            // NV12: row 0 of the interleaved U V plane (2-byte aligned); BGR: NULL
    long long first;
    int w, h, pitch, pitch_uv;
};

// the detections cut out of the frames (ffgpu_crop.inc).  One source as the kernels read it: a DrawTarget that is only read, with the NV12 matrix
// (fmt as FrameDesc::fmt).
struct CropSrc {
    const unsigned char *p0;      // row 0 of the BGR pixels / of the Y plane; NULL: a skipped source
    const unsigned char *p1;      // NV12: row 0 of the interleaved U V plane (2-byte aligned); BGR: NULL
    long long first;
    int w, h, pitch, pitch_uv;
    int fmt, pad_;
};

// What a checked descriptor resolves to, whichever of the three structs above it fills.  p0 == NULL: a skipped target (FRAME_DRAW only).
struct FrameArgs {
    const unsigned char *p0, *p1;
    int w, h, pitch, pitch_uv, fmt;
};
// The two ways a descriptor is used, and all that differs between them.  The forward reads its frames: every one must be there, and k_front /
// k_input4 take a BGR frame of any height.  The draw writes its targets, and the crop reads its sources by the draw's contract: a NULL address
// skips the target, and the kernels' coordinates want h <= 0x3fffffff.
struct FrameRole {
    const char *noun;             // the descriptor in a message
    bool need_all;                // a NULL address is an error, reported before any other field
    const char *uv_access;        // what an odd uv address would break
    int bgr_max_h;
};
static const FrameRole FRAME_FORWARD = { "frame", true, "read", 0x7fffffff }, FRAME_DRAW = { "target", false, "written", 0x3fffffff };
static const FrameRole FRAME_SCRATCH = { "scratch", false, "written", 0x3fffffff };     // the blur's second surface per target: a FRAME_DRAW by another name

inline int ffgpu_frame_check(const char *what, const FrameRole &role, int k, const ffgpu_bgr_frame &f, FrameArgs &a)
{
    const char *const noun = role.noun;
    if (role.need_all && !f.bgr) { ffgpu_set_error("%s: %s %d: NULL bgr", what, noun, k); return -1; }
    if (f.w <= 0 || f.h <= 0 || 3L * f.w > 0x7fffffffL || f.h > role.bgr_max_h) { ffgpu_set_error("%s: %s %d: bad size %d x %d", what, noun, k, f.w, f.h); return -1; }
    if (f.reserved != 0) { ffgpu_set_error("%s: %s %d: reserved must be 0", what, noun, k); return -1; }
    const long pitch = f.pitch ? (long)f.pitch : ((3L * f.w + 3) & ~3L);
    if (pitch < 3L * f.w || pitch > 0x7fffffffL) { ffgpu_set_error("%s: %s %d: pitch %d is below 3 w = %ld", what, noun, k, f.pitch, 3L * f.w); return -1; }
    a = FrameArgs{ f.bgr, nullptr, f.w, f.h, (int)pitch, 0, 0 };
    return 0;
}

inline int ffgpu_frame_check(const char *what, const FrameRole &role, int k, const ffgpu_nv12_frame &f, FrameArgs &a)
{
    const char *const noun = role.noun;
    if (role.need_all && !f.y) { ffgpu_set_error("%s: %s %d: NULL y", what, noun, k); return -1; }
    if (f.w <= 0 || f.h <= 0 || f.w > 0x3fffffff || f.h > 0x3fffffff) { ffgpu_set_error("%s: %s %d: bad size %d x %d", what, noun, k, f.w, f.h); return -1; }
    if (f.reserved != 0) { ffgpu_set_error("%s: %s %d: reserved must be 0", what, noun, k); return -1; }
    if (f.matrix < 0 || f.matrix > 3) { ffgpu_set_error("%s: %s %d: matrix %d is none of FFGPU_YUV_* (0..3)", what, noun, k, f.matrix); return -1; }
    const int pitch_y = f.pitch_y ? f.pitch_y : f.w, min_uv = 2 * ((f.w + 1) / 2), pitch_uv = f.pitch_uv ? f.pitch_uv : min_uv;
    if (pitch_y < f.w) { ffgpu_set_error("%s: %s %d: pitch_y %d is below w = %d", what, noun, k, f.pitch_y, f.w); return -1; }
    if (pitch_uv < min_uv || (pitch_uv & 1)) { ffgpu_set_error("%s: %s %d: pitch_uv %d is odd or below 2 ((w + 1) / 2) = %d", what, noun, k, f.pitch_uv, min_uv); return -1; }
    a = FrameArgs{ nullptr, nullptr, f.w, f.h, pitch_y, pitch_uv, 1 + f.matrix };
    if (!f.y) return 0;
    const unsigned char *uv = f.uv ? f.uv : f.y + (size_t)pitch_y * f.h;
    if (reinterpret_cast<uintptr_t>(uv) & 1) {
        ffgpu_set_error("%s: %s %d: the uv plane's address %p is odd (U V pairs are %s as aligned 16-bit values)", what, noun, k, (const void *)uv, role.uv_access);
        return -1;
    }
    a.p0 = f.y; a.p1 = uv;
    return 0;
}

inline void ffgpu_frame_fill(FrameDesc &d, const FrameArgs &a) { d.bgr = a.p0; d.uv = a.p1; d.w = a.w; d.h = a.h; d.pitch = a.pitch; d.pitch_uv = a.pitch_uv; d.fmt = a.fmt; }
inline void ffgpu_frame_fill(DrawTarget &d, const FrameArgs &a)
{
    d.p0 = const_cast<unsigned char *>(a.p0); d.p1 = const_cast<unsigned char *>(a.p1); d.w = a.w; d.h = a.h; d.pitch = a.pitch; d.pitch_uv = a.pitch_uv;
}
inline void ffgpu_frame_fill(CropSrc &d, const FrameArgs &a) { d.p0 = a.p0; d.p1 = a.p1; d.w = a.w; d.h = a.h; d.pitch = a.pitch; d.pitch_uv = a.pitch_uv; d.fmt = a.fmt; }

// n descriptors (ffgpu_bgr_frame or ffgpu_nv12_frame) checked in order into a table of FrameDesc, DrawTarget or CropSrc, every other byte of a row
// zero; -1 with the first bad descriptor's index in the message
template <class Row, class Frame>
int ffgpu_frame_table(const char *what, const FrameRole &role, const Frame *f, int n, std::vector<Row> &out)
{
    out.resize((size_t)n);
    if (n > 0) memset(out.data(), 0, sizeof(Row) * (size_t)n);
    for (int k = 0; k < n; k++) {
        FrameArgs a;
        if (ffgpu_frame_check(what, role, k, f[k], a)) return -1;
        ffgpu_frame_fill(out[k], a);
    }
    return 0;
}

// -------------------------------------------------------------------------- colours and class tables
// a colour of a spec (B G R or Y U V, a fourth byte ignored) as the kernels carry it: byte k in bits 8 k .. 8 k + 7
inline unsigned ffgpu_pack_colour(const unsigned char *c) { return (unsigned)c[0] | (unsigned)c[1] << 8 | (unsigned)c[2] << 16; }

// a spec's palette (npalette entries of 4 bytes), or without one its single `color`, packed into pal[256]: npal entries, the rest zero
inline int ffgpu_palette_plan(const char *what, const unsigned char *palette, int npalette, const unsigned char *color, unsigned pal[256], int *npal)
{
    if (palette ? (npalette < 1 || npalette > 256) : npalette != 0) {
        ffgpu_set_error("%s: npalette %d (0 with a NULL palette, else 1..256)", what, npalette);
        return -1;
    }
    memset(pal, 0, sizeof(unsigned) * 256);
    const unsigned char *src = palette ? palette : color;
    *npal = palette ? npalette : 1;
    for (int k = 0; k < *npal; k++) pal[k] = ffgpu_pack_colour(src + 4 * k);
    return 0;
}

// a spec's class table: nclasses flags, or none
inline int ffgpu_class_table_check(const char *what, const unsigned char *classes, int nclasses)
{
    if (classes ? (nclasses < 1 || nclasses > 256) : nclasses != 0) {
        ffgpu_set_error("%s: nclasses %d (0 with NULL classes, else 1..256)", what, nclasses);
        return -1;
    }
    return 0;
}

// -------------------------------------------------------------------------- where a post-pass finds its boxes
// A post-pass runs behind a forward or a merge and reads one record per target, and either the record's own box[] or a full list.  Where those are is
// this value: the operator forms build it from the caller's buffers (ffgpu_source_dev), the executor forms from the executor's (ffgpu_source_exec),
// and the launches take it.
struct DetSource {
    const ffgpu_frame_dets *recs;
    const BBOX *lists;                // NULL: the records' own boxes (stride FFGPU_MAX_DET)
    std::vector<long long> first;     // target t's list starts at box first[t] of `lists`
    long long longest;                // room of the longest list, in boxes
    int stride;                       // the kernels' clamp of a list's length and the pitch of their output lists.  The operator forms: the caller's;
                                      // the executor forms derive it from `longest`, each family by its own rule
};

static_assert(FFGPU_DRAW_ENTRIES == 0 && FFGPU_CROP_ENTRIES == 0 && FFGPU_TRACK_ENTRIES == 0 && FFGPU_RELABEL_ENTRIES == 0 && FFGPU_REDACT_ENTRIES == 0 &&
              FFGPU_ZONES_ENTRIES == 0 && FFGPU_CAPTION_ENTRIES == 0 && FFGPU_CAPTION_MERGED == 1 && FFGPU_DRAW_MERGED == 1 && FFGPU_CROP_MERGED == 1 && FFGPU_TRACK_MERGED == 1 && FFGPU_RELABEL_MERGED == 1 &&
              FFGPU_REDACT_MERGED == 1 && FFGPU_ZONES_MERGED == 1 && FFGPU_BLUR_ENTRIES == 0 && FFGPU_BLUR_MERGED == 1, "ffgpu_source_exec: one check of `which` serves the eight families");

// the list stride of an operator form: the caller's with lists, FFGPU_MAX_DET without; -1 with a message outside 1 .. 2^24
inline int ffgpu_list_stride(const char *what, const void *d_lists, int list_stride)
{
    const int stride = d_lists ? list_stride : FFGPU_MAX_DET;
    if (stride < 1 || stride > (1 << 24)) { ffgpu_set_error("%s: bad list_stride %d", what, list_stride); return -1; }
    return stride;
}

// The operator forms: list t starts at list_first[t], or at t x stride without that array.  ntargets has been checked by the caller.
inline int ffgpu_source_dev(const char *what, const void *d_records, const void *d_lists, int list_stride, const int *list_first, int ntargets, DetSource &src)
{
    if (!d_records) { ffgpu_set_error("%s: NULL records", what); return -1; }
    const int stride = ffgpu_list_stride(what, d_lists, list_stride);
    if (stride < 0) return -1;
    src.recs = (const ffgpu_frame_dets *)d_records; src.lists = (const BBOX *)d_lists; src.stride = stride; src.longest = stride;
    src.first.assign((size_t)std::max(ntargets, 0), 0);
    for (int t = 0; t < ntargets && d_lists; t++) {
        if (list_first && list_first[t] < 0) { ffgpu_set_error("%s: target %d: negative list start %d", what, t, list_first[t]); return -1; }
        src.first[t] = list_first ? (long long)list_first[t] : (long long)t * stride;
    }
    return 0;
}

// The executor forms: `which` (FFGPU_<family>_ENTRIES / _MERGED) names the N entries' lists of cand_cap boxes each, or the pictures' merged lists --
// picture g's starts where its first tile's would and has room for all of its tiles' boxes (mrg_off: the ntargets + 1 tile offsets of the last
// merge, NULL or empty before any).  recs, lists and stride are the caller's to set.  A picture with no tile still gets one tile's worth: k_merge_tiles
// never reports more boxes than the room, so the longest room is a safe clamp.
inline int ffgpu_source_exec(const char *what, const char *family, int which, int ntargets, int N, int cand_cap, const std::vector<int> *mrg_off, DetSource &src)
{
    if (which != 0 && which != 1) { ffgpu_set_error("%s: which = %d is neither FFGPU_%s_ENTRIES nor FFGPU_%s_MERGED", what, which, family, family); return -1; }
    const bool merged = which == 1;
    if (merged && (!mrg_off || mrg_off->empty())) { ffgpu_set_error("%s: no ffgpu_exec_merge_tiles has run on this executor", what); return -1; }
    const int want = merged ? (int)mrg_off->size() - 1 : N;
    if (ntargets != want) {
        if (merged) ffgpu_set_error("%s: %d targets for a merge of %d pictures", what, ntargets, want);
        else ffgpu_set_error("%s: %d targets for an executor of batch %d", what, ntargets, want);
        return -1;
    }
    src.recs = nullptr; src.lists = nullptr; src.stride = 0;
    src.first.assign((size_t)ntargets, 0);
    int most = 1;
    for (int t = 0; t < ntargets; t++) {
        src.first[t] = (long long)cand_cap * (merged ? (*mrg_off)[t] : t);
        if (merged) most = std::max(most, (*mrg_off)[t + 1] - (*mrg_off)[t]);
    }
    src.longest = (long long)cand_cap * most;
    return 0;
}
