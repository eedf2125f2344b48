// ffgpu_lines_host.hpp -- the host side of the outlines family (include/ffcnn_hip.h: ffgpu_draw_segments_*_dev, ffgpu_outline_scene_dev,
// ffgpu_outline_spec_check) before anything reaches the device: the outline spec resolved into a plan, and the argument checks.  Plain C++17 with no
// HIP in it: every function reports through ffgpu_set_error and touches no device, so san/lines_driver.cc runs the same lines on the CPU under
// ASan + UBSan (tests/test_outlines_abi.py).  What a scene composer reads of a zones call is checked by
// ffgpu_text_host.hpp's ffgpu_scene_source_*_check, which the captions' scene composer shares.
#pragma once
#include "ffgpu_text_host.hpp"

static_assert(sizeof(ffgpu_seg_item) == 32 && sizeof(ffgpu_outline_spec) == 40, "include/ffcnn_hip.h states these sizes");
#define SEG_ARG_TARGETS       64                      // targets per launch of the segment rasteriser
#define OUTLINE_ARG_TARGETS   512                     // targets per launch of the scene composer
#define OUTLINE_PARTS         (FFGPU_OUTLINE_ZONES | FFGPU_OUTLINE_LINES | FFGPU_OUTLINE_MARKERS)
#define OUTLINE_FLAGS         (OUTLINE_PARTS | FFGPU_OUTLINE_TICKS | FFGPU_OUTLINE_ALARM)

// an outline spec as the kernel reads it: checked, the palette packed as the draw's entries are (npal == 1: the spec's `color`)
struct OutlinePlan {
    int flags, thickness, line_dash, marker, npal;
    unsigned alarm;
    unsigned pal[256];
};

inline int ffgpu_outline_spec_plan(const char *what, const ffgpu_outline_spec *sp, OutlinePlan &pl)
{
    if (!sp) { ffgpu_set_error("%s: NULL spec", what); return -1; }
    memset(&pl, 0, sizeof pl);
    if (sp->flags & ~OUTLINE_FLAGS) { ffgpu_set_error("%s: unknown flags 0x%x", what, (unsigned)sp->flags); return -1; }
    if (!(sp->flags & OUTLINE_PARTS)) { ffgpu_set_error("%s: flags 0x%x name no part (FFGPU_OUTLINE_ZONES | _LINES | _MARKERS)", what, (unsigned)sp->flags); return -1; }
    if ((sp->flags & FFGPU_OUTLINE_TICKS) && !(sp->flags & FFGPU_OUTLINE_LINES)) { ffgpu_set_error("%s: FFGPU_OUTLINE_TICKS without FFGPU_OUTLINE_LINES", what); return -1; }
    if ((sp->flags & FFGPU_OUTLINE_ALARM) && !(sp->flags & FFGPU_OUTLINE_ZONES)) { ffgpu_set_error("%s: FFGPU_OUTLINE_ALARM without FFGPU_OUTLINE_ZONES", what); return -1; }
    if (sp->thickness < 1 || sp->thickness > 8) { ffgpu_set_error("%s: thickness %d is outside 1..8", what, sp->thickness); return -1; }
    if (sp->line_dash < 0 || sp->line_dash > 6) { ffgpu_set_error("%s: line_dash %d is outside 0..6", what, sp->line_dash); return -1; }
    if (sp->marker < 0 || sp->marker > 32) { ffgpu_set_error("%s: marker %d is outside 0..32", what, sp->marker); return -1; }
    if ((sp->flags & FFGPU_OUTLINE_MARKERS) && sp->marker < 1) { ffgpu_set_error("%s: marker %d with FFGPU_OUTLINE_MARKERS (at least 1)", what, sp->marker); return -1; }
    if (ffgpu_palette_plan(what, sp->palette, sp->npalette, sp->color, pl.pal, &pl.npal)) return -1;
    if (sp->reserved != 0) { ffgpu_set_error("%s: reserved must be 0", what); return -1; }
    pl.flags = sp->flags; pl.thickness = sp->thickness; pl.line_dash = sp->line_dash; pl.marker = sp->marker;
    pl.alarm = ffgpu_pack_colour(sp->alarm);
    return 0;
}

// the segment items of a call: lo = the smallest items_stride (1: the rasteriser; FFGPU_OUTLINE_FIXED: the scene composer)
inline int ffgpu_seg_items_check(const char *what, const void *d_items, int items_stride, int lo)
{
    if (!d_items) { ffgpu_set_error("%s: NULL items", what); return -1; }
    if (reinterpret_cast<uintptr_t>(d_items) & 3) { ffgpu_set_error("%s: the items must be 4-byte aligned", what); return -1; }
    if (items_stride < lo || items_stride > FFGPU_SEG_ITEMS) { ffgpu_set_error("%s: items_stride %d is outside %d..%d", what, items_stride, lo, FFGPU_SEG_ITEMS); return -1; }
    return 0;
}

// the segment rasteriser's arguments but the descriptors (ffgpu_frame_table checks those)
inline int ffgpu_draw_segments_args_check(const char *what, const void *d_items, int items_stride, const void *targets, int ntargets)
{
    if (ffgpu_seg_items_check(what, d_items, items_stride, 1)) return -1;
    if (!targets) { ffgpu_set_error("%s: NULL targets", what); return -1; }
    return ffgpu_ntargets_check(what, ntargets);
}

inline int ffgpu_outline_scene_args_check(const char *what, const void *d_scenes, const void *d_state, int nstreams, int capacity, const void *d_events,
                                          int events_stride, const int *streams, int ntargets, const ffgpu_outline_spec *spec, const void *d_items,
                                          int items_stride, OutlinePlan &pl)
{
    if (ffgpu_scene_source_nulls_check(what, d_scenes, d_state, d_events, streams)) return -1;
    if (ffgpu_outline_spec_plan(what, spec, pl)) return -1;
    if (ffgpu_seg_items_check(what, d_items, items_stride, FFGPU_OUTLINE_FIXED)) return -1;
    return ffgpu_scene_source_ranges_check(what, d_scenes, d_state, nstreams, capacity, d_events, events_stride, streams, ntargets);
}
