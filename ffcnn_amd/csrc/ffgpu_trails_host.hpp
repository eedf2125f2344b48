// ffgpu_trails_host.hpp -- the host side of the track trails (include/ffcnn_hip.h: ffgpu_trails_state_bytes, ffgpu_trails_spec_check,
// ffgpu_trails_boxes_dev, ffgpu_exec_trails) before anything reaches the device: the state's size, the spec resolved into a plan, the argument checks.
// Plain C++17 with no HIP in it: every function reports through ffgpu_set_error and touches no device, so san/trails_driver.cc runs the same lines on
// the CPU under ASan + UBSan (tests/test_trails_abi.py).  The launch's entry table and the stream checks are ffgpu_streams_host.hpp's,
// the palette is ffgpu_args.hpp's.
#pragma once
#include "ffgpu_args.hpp"
#include "ffgpu_zones_host.hpp"

static_assert(sizeof(ffgpu_trail_point) == 12 && sizeof(ffgpu_trail_slot) == 416 && sizeof(ffgpu_trails_spec) == 64 && sizeof(ffgpu_seg_item) == 32,
              "include/ffcnn_hip.h states these sizes");
static_assert(FFGPU_TRAILS_ENTRIES == 0 && FFGPU_TRAILS_MERGED == 1 && FFGPU_TRAILS_DETS == FFGPU_ZONES_DETS, "ffgpu_source_exec: one check of `which` serves every family");
#define TRAILS_STATE_HEADER 16                        // { int frames, live, reserved[2] }
#define TRAILS_ARG_ENTRIES  64                        // records per launch (the 1 KB palette travels with them)
#define TRAILS_FLAGS        (FFGPU_TRAILS_COAST | FFGPU_TRAILS_TAPER)

inline size_t ffgpu_trails_state_bytes_host(int nstreams, int capacity)
{
    if (nstreams < 1 || nstreams > 65536 || capacity < 1 || capacity > FFGPU_TRAILS_DETS) return 0;
    return (size_t)nstreams * (TRAILS_STATE_HEADER + sizeof(ffgpu_trail_slot) * (size_t)capacity);
}

// a trails spec as the kernel reads it: checked, the palette packed as the draw's entries are (npal == 1: the spec's `color`)
struct TrailsPlan {
    int capacity, max_missed, identity, flags, anchor, points, min_move, thickness, coast_dash, npal;
    float min_score;
    unsigned pal[256];
};

inline int ffgpu_trails_spec_plan(const char *what, const ffgpu_trails_spec *sp, TrailsPlan &pl)
{
    if (!sp) { ffgpu_set_error("%s: NULL spec", what); return -1; }
    memset(&pl, 0, sizeof pl);
    if (sp->capacity < 1 || sp->capacity > FFGPU_TRAILS_DETS) { ffgpu_set_error("%s: capacity %d is outside 1..%d", what, sp->capacity, FFGPU_TRAILS_DETS); return -1; }
    if (sp->max_missed < 0 || sp->max_missed > (1 << 20)) { ffgpu_set_error("%s: max_missed %d is outside 0..2^20", what, sp->max_missed); return -1; }
    if (sp->identity != FFGPU_ZONES_TYPE && sp->identity != FFGPU_ZONES_IDS) {
        ffgpu_set_error("%s: identity %d is neither FFGPU_ZONES_TYPE nor _IDS (with _NONE there is nobody to remember)", what, sp->identity);
        return -1;
    }
    if (sp->flags & ~TRAILS_FLAGS) { ffgpu_set_error("%s: unknown flags 0x%x", what, (unsigned)sp->flags); return -1; }
    if (!(sp->min_score >= 0.f && sp->min_score <= 1.f)) { ffgpu_set_error("%s: min_score %g is not in [0, 1]", what, (double)sp->min_score); return -1; }
    if (sp->anchor != 0 && sp->anchor != 1) { ffgpu_set_error("%s: anchor %d is neither 0 nor 1", what, sp->anchor); return -1; }
    if (sp->points < 2 || sp->points > FFGPU_TRAIL_POINTS) { ffgpu_set_error("%s: points %d is outside 2..%d", what, sp->points, FFGPU_TRAIL_POINTS); return -1; }
    if (sp->min_move < 0 || sp->min_move > (1 << 20)) { ffgpu_set_error("%s: min_move %d is outside 0..2^20", what, sp->min_move); return -1; }
    if (sp->thickness < 1 || sp->thickness > 8) { ffgpu_set_error("%s: thickness %d is outside 1..8", what, sp->thickness); return -1; }
    if (sp->coast_dash < 0 || sp->coast_dash > 6) { ffgpu_set_error("%s: coast_dash %d is outside 0..6", what, sp->coast_dash); return -1; }
    if (ffgpu_palette_plan(what, sp->palette, sp->npalette, sp->color, pl.pal, &pl.npal)) return -1;
    if (sp->reserved0 != 0 || sp->reserved != 0) { ffgpu_set_error("%s: spec: reserved must be 0", what); return -1; }
    pl.capacity = sp->capacity; pl.max_missed = sp->max_missed; pl.identity = sp->identity; pl.flags = sp->flags; pl.anchor = sp->anchor;
    pl.points = sp->points; pl.min_move = sp->min_move; pl.thickness = sp->thickness; pl.coast_dash = sp->coast_dash; pl.min_score = sp->min_score;
    return 0;
}

// what the operator and the executor form check alike, before either looks at its records
inline int ffgpu_trails_args_check(const char *what, const int *streams, int ntargets, const ffgpu_trails_spec *spec, const void *d_state, int nstreams,
                                   const void *d_ids, const void *d_rows, const void *d_items, int items_stride, int first_item, int nitems, TrailsPlan &pl)
{
    if (!streams) { ffgpu_set_error("%s: NULL streams", what); return -1; }
    if (ffgpu_trails_spec_plan(what, spec, pl)) return -1;
    if (!d_state) { ffgpu_set_error("%s: NULL state", what); return -1; }
    if (!d_rows) { ffgpu_set_error("%s: NULL rows", what); return -1; }
    if (spec->identity == FFGPU_ZONES_IDS && !d_ids) { ffgpu_set_error("%s: NULL ids with identity FFGPU_ZONES_IDS", what); return -1; }
    if (spec->identity != FFGPU_ZONES_IDS && d_ids) { ffgpu_set_error("%s: ids given without identity FFGPU_ZONES_IDS", what); return -1; }
    if (ffgpu_streams_check(what, ntargets, nstreams, d_state)) return -1;
    if (!d_items) {
        if (items_stride != 0 || first_item != 0 || nitems != 0) {
            ffgpu_set_error("%s: NULL items with items_stride %d, first_item %d, nitems %d (all 0 then)", what, items_stride, first_item, nitems);
            return -1;
        }
    } else {
        if (reinterpret_cast<uintptr_t>(d_items) & 3) { ffgpu_set_error("%s: the items must be 4-byte aligned", what); return -1; }
        if (items_stride < 1 || items_stride > FFGPU_SEG_ITEMS) { ffgpu_set_error("%s: items_stride %d is outside 1..%d", what, items_stride, FFGPU_SEG_ITEMS); return -1; }
        if (first_item < 0) { ffgpu_set_error("%s: negative first_item %d", what, first_item); return -1; }
        if (nitems < 1) { ffgpu_set_error("%s: nitems %d (at least 1)", what, nitems); return -1; }
        if ((long long)first_item + nitems > items_stride) {
            ffgpu_set_error("%s: items %d .. %lld lie outside a row of items_stride %d", what, first_item, (long long)first_item + nitems - 1, items_stride);
            return -1;
        }
    }
    return ffgpu_stream_range_check(what, streams, ntargets, nstreams);
}
