// ffgpu_text_host.hpp -- the host side of the captions family (include/ffcnn_hip.h: ffgpu_font_builtin, ffgpu_draw_text_*_dev, ffgpu_caption_boxes_dev,
// ffgpu_caption_scene_dev, ffgpu_exec_caption_*) before anything reaches the device: the built-in font's table, the caption spec resolved into a plan,
// and the argument checks.  Plain C++17 with no HIP in it: every function reports through ffgpu_set_error and touches no device, so san/text_driver.cc
// runs the same lines on the CPU under ASan + UBSan (tests/test_captions_abi.py).
#pragma once
#include <stdint.h>
#include <string.h>
#include <math.h>
#include "ffgpu_args.hpp"
#include "ffgpu_streams_host.hpp"

static_assert(sizeof(ffgpu_text_item) == 64 && sizeof(ffgpu_caption_spec) == 48, "include/ffcnn_hip.h states these sizes");
#define FONT8_GLYPHS          96                      // ffgpu_font8.inc: the ASCII glyphs 32..126, then the unknown glyph
#define TEXT_ARG_TARGETS      64                      // targets per launch of the rasteriser
#define CAPTION_ARG_TARGETS   128                     // targets per launch of the box composer
#define SCENE_ARG_TARGETS     512                     // targets per launch of the scene composer
#define CAPTION_STATE_HEADER  144                     // the zones state's header (ffgpu_zones_host.hpp: ZONES_STATE_HEADER)
#define CAPTION_PARTS         (FFGPU_CAPTION_NAME | FFGPU_CAPTION_SCORE | FFGPU_CAPTION_ID)

static const unsigned char ffgpu_font8_glyphs[FONT8_GLYPHS * 8] = {
#include "ffgpu_font8.inc"
};
// the glyph of ffgpu_font8.inc a code shows
inline int ffgpu_font8_index(int code) { return code >= 32 && code <= 126 ? code - 32 : FONT8_GLYPHS - 1; }
inline void ffgpu_font_builtin_host(unsigned char out[2048])
{
    for (int i = 0; i < 2048; i++) out[i] = ffgpu_font8_glyphs[ffgpu_font8_index(i >> 3) * 8 + (i & 7)];
}

// a caption spec as the kernels read it: checked, the palette packed as the draw's entries are (npal == 1: the spec's `color`)
struct CaptionPlan {
    float min_score;
    int   flags, identity, scale, nnames, npal;
    unsigned fg;
    const void *d_names;
    unsigned pal[256];
};

// boxes: the box composer reads every field; the scene composer ignores min_score, the part flags, identity and the names
inline int ffgpu_caption_spec_check(const char *what, const ffgpu_caption_spec *sp, bool boxes, CaptionPlan &pl)
{
    if (!sp) { ffgpu_set_error("%s: NULL spec", what); return -1; }
    memset(&pl, 0, sizeof pl);
    if (boxes) {
        if (!(sp->min_score >= 0.f && sp->min_score <= 1.f)) { ffgpu_set_error("%s: min_score %g is not in [0, 1]", what, (double)sp->min_score); return -1; }
        if (sp->flags & ~(CAPTION_PARTS | FFGPU_CAPTION_OPAQUE)) { ffgpu_set_error("%s: unknown flags 0x%x", what, (unsigned)sp->flags); return -1; }
        if (!(sp->flags & CAPTION_PARTS)) { ffgpu_set_error("%s: flags 0x%x name no part (FFGPU_CAPTION_NAME | _SCORE | _ID)", what, (unsigned)sp->flags); return -1; }
        if (sp->identity != FFGPU_ZONES_NONE && sp->identity != FFGPU_ZONES_TYPE && sp->identity != FFGPU_ZONES_IDS) {
            ffgpu_set_error("%s: identity %d is none of FFGPU_ZONES_NONE, _TYPE, _IDS", what, sp->identity);
            return -1;
        }
        if (sp->nnames < 0 || (sp->d_names ? sp->nnames < 1 : sp->nnames != 0)) {
            ffgpu_set_error("%s: nnames %d (0 with NULL names, else >= 1)", what, sp->nnames);
            return -1;
        }
        pl.min_score = sp->min_score; pl.identity = sp->identity; pl.nnames = sp->nnames; pl.d_names = sp->d_names;
    }
    if (sp->scale < 1 || sp->scale > 4) { ffgpu_set_error("%s: scale %d is outside 1..4", what, sp->scale); return -1; }
    if (ffgpu_palette_plan(what, sp->palette, sp->npalette, sp->color, pl.pal, &pl.npal)) return -1;
    pl.flags = sp->flags; pl.scale = sp->scale;
    pl.fg = ffgpu_pack_colour(sp->fg);
    return 0;
}

// the items of a call: lo = the smallest items_stride (1: the rasteriser and the box composer; 16: the scene composer)
inline int ffgpu_text_items_check(const char *what, const void *d_items, int items_stride, int lo)
{
    if (!d_items) { ffgpu_set_error("%s: NULL items", what); return -1; }
    if (reinterpret_cast<uintptr_t>(d_items) & 3) { ffgpu_set_error("%s: the items must be 4-byte aligned", what); return -1; }
    if (items_stride < lo || items_stride > FFGPU_TEXT_ITEMS) { ffgpu_set_error("%s: items_stride %d is outside %d..%d", what, items_stride, lo, FFGPU_TEXT_ITEMS); return -1; }
    return 0;
}
inline int ffgpu_ntargets_check(const char *what, int ntargets)
{
    if (ntargets < 1 || ntargets > (1 << 24)) { ffgpu_set_error("%s: %d targets (ntargets >= 1)", what, ntargets); return -1; }
    return 0;
}

// the rasteriser's arguments but the descriptors (ffgpu_frame_table checks those)
inline int ffgpu_draw_text_args_check(const char *what, const void *d_items, int items_stride, const void *targets, int ntargets)
{
    if (ffgpu_text_items_check(what, d_items, items_stride, 1)) return -1;
    if (!targets) { ffgpu_set_error("%s: NULL targets", what); return -1; }
    return ffgpu_ntargets_check(what, ntargets);
}

// what the box composer and the executor forms check alike, before either looks at its records
inline int ffgpu_caption_boxes_args_check(const char *what, const ffgpu_caption_spec *spec, const void *d_ids, const void *d_items, int items_stride, CaptionPlan &pl)
{
    if (ffgpu_caption_spec_check(what, spec, true, pl)) return -1;
    if (ffgpu_text_items_check(what, d_items, items_stride, 1)) return -1;
    if (spec->identity == FFGPU_ZONES_IDS && !d_ids) { ffgpu_set_error("%s: NULL ids with identity FFGPU_ZONES_IDS", what); return -1; }
    if (spec->identity != FFGPU_ZONES_IDS && d_ids) { ffgpu_set_error("%s: ids given without identity FFGPU_ZONES_IDS", what); return -1; }
    if (reinterpret_cast<uintptr_t>(d_ids) & 3) { ffgpu_set_error("%s: the ids must be 4-byte aligned", what); return -1; }
    return 0;
}

// what a scene composer reads of the zones call (this one and ffgpu_outline_scene_dev, ffgpu_lines_host.hpp), in two halves: the pointers are looked at
// before the spec and the items, the ranges behind them
inline int ffgpu_scene_source_nulls_check(const char *what, const void *d_scenes, const void *d_state, const void *d_events, const int *streams)
{
    if (!d_scenes) { ffgpu_set_error("%s: NULL scenes", what); return -1; }
    if (!d_state) { ffgpu_set_error("%s: NULL state", what); return -1; }
    if (!d_events) { ffgpu_set_error("%s: NULL events", what); return -1; }
    if (!streams) { ffgpu_set_error("%s: NULL streams", what); return -1; }
    return 0;
}
inline int ffgpu_scene_source_ranges_check(const char *what, const void *d_scenes, const void *d_state, int nstreams, int capacity, const void *d_events,
                                           int events_stride, const int *streams, int ntargets)
{
    if (ffgpu_ntargets_check(what, ntargets)) return -1;
    if (nstreams < 1 || nstreams > 65536) { ffgpu_set_error("%s: nstreams %d is outside 1..65536", what, nstreams); return -1; }
    if (capacity < 1 || capacity > FFGPU_ZONES_DETS) { ffgpu_set_error("%s: capacity %d is outside 1..%d", what, capacity, FFGPU_ZONES_DETS); return -1; }
    if (events_stride < FFGPU_ZONES_ROW) { ffgpu_set_error("%s: events_stride %d is below FFGPU_ZONES_ROW = %d", what, events_stride, FFGPU_ZONES_ROW); return -1; }
    if ((reinterpret_cast<uintptr_t>(d_scenes) | reinterpret_cast<uintptr_t>(d_state) | reinterpret_cast<uintptr_t>(d_events)) & 3) {
        ffgpu_set_error("%s: the scenes, the state and the events must be 4-byte aligned", what);
        return -1;
    }
    return ffgpu_stream_range_check(what, streams, ntargets, nstreams);
}

inline int ffgpu_caption_scene_args_check(const char *what, const void *d_scenes, const void *d_state, int nstreams, int capacity, const void *d_events,
                                          int events_stride, const int *streams, int ntargets, const ffgpu_caption_spec *spec, const void *d_items,
                                          int items_stride, CaptionPlan &pl)
{
    if (ffgpu_scene_source_nulls_check(what, d_scenes, d_state, d_events, streams)) return -1;
    if (ffgpu_caption_spec_check(what, spec, false, pl)) return -1;
    if (ffgpu_text_items_check(what, d_items, items_stride, 16)) return -1;
    return ffgpu_scene_source_ranges_check(what, d_scenes, d_state, nstreams, capacity, d_events, events_stride, streams, ntargets);
}
