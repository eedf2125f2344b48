// ffgpu_zones_host.hpp -- the host side of the zones family (include/ffcnn_hip.h: ffgpu_scene_check, ffgpu_zones_boxes_dev, ffgpu_exec_zones) before
// anything reaches the device: the scene check and the spec and argument checks (the launch's entry table, its grouping by video stream and the stream
// checks are ffgpu_streams_host.hpp's).  Plain C++17 with no HIP in it: every function reports through ffgpu_set_error and touches no device, so
// san/zones_driver.cc runs the same lines on the CPU under ASan + UBSan (tests/test_zones_abi.py).
#pragma once
#include <stdint.h>
#include <string.h>
#include <math.h>
#include "ffcnn_hip.h"
#include "ffgpu_streams_host.hpp"

static_assert(sizeof(ffgpu_zone) == 96 && sizeof(ffgpu_line) == 32 && sizeof(ffgpu_scene) == 1040 && sizeof(ffgpu_zones_spec) == 32 &&
              sizeof(ffgpu_zone_slot) == 64, "include/ffcnn_hip.h states these sizes");
#define ZONES_STATE_HEADER 144                        // { int frames, live, reserved[2]; unsigned total_entered[8], total_left[8], total_fwd[8], total_back[8] }
#define ZONES_ARG_ENTRIES  128                        // records per launch

inline size_t ffgpu_zones_state_bytes_host(int nstreams, int capacity)
{
    if (nstreams < 1 || nstreams > 65536 || capacity < 1 || capacity > FFGPU_ZONES_DETS) return 0;
    return (size_t)nstreams * (ZONES_STATE_HEADER + sizeof(ffgpu_zone_slot) * (size_t)capacity);
}

// what is wrong with a scene before the caller uploads it (the kernel itself is total over any bytes)
inline int ffgpu_scene_check_host(const ffgpu_scene *sc, int n)
{
    const char *const what = "scene_check";
    if (!sc) { ffgpu_set_error("%s: NULL scenes", what); return -1; }
    if (n < 1) { ffgpu_set_error("%s: %d scenes (n >= 1)", what, n); return -1; }
    for (int s = 0; s < n; s++) {
        const ffgpu_scene &c = sc[s];
        if (c.nzones < 0 || c.nzones > FFGPU_SCENE_ZONES) { ffgpu_set_error("%s: scene %d: nzones %d is outside 0..%d", what, s, c.nzones, FFGPU_SCENE_ZONES); return -1; }
        if (c.nlines < 0 || c.nlines > FFGPU_SCENE_LINES) { ffgpu_set_error("%s: scene %d: nlines %d is outside 0..%d", what, s, c.nlines, FFGPU_SCENE_LINES); return -1; }
        if (c.anchor != 0 && c.anchor != 1) { ffgpu_set_error("%s: scene %d: anchor %d is neither 0 nor 1", what, s, c.anchor); return -1; }
        if (c.reserved != 0) { ffgpu_set_error("%s: scene %d: reserved must be 0", what, s); return -1; }
        for (int z = 0; z < c.nzones; z++) {
            const ffgpu_zone &zn = c.zone[z];
            if (zn.nverts < 3 || zn.nverts > FFGPU_ZONE_VERTS) { ffgpu_set_error("%s: scene %d: zone %d: nverts %d is outside 3..%d", what, s, z, zn.nverts, FFGPU_ZONE_VERTS); return -1; }
            for (int i = 0; i < zn.nverts; i++)
                if (!isfinite(zn.x[i]) || !isfinite(zn.y[i])) { ffgpu_set_error("%s: scene %d: zone %d: vertex %d is not finite", what, s, z, i); return -1; }
            if (zn.dwell_frames < 0) { ffgpu_set_error("%s: scene %d: zone %d: negative dwell_frames %d", what, s, z, zn.dwell_frames); return -1; }
            if (zn.reserved[0] != 0 || zn.reserved[1] != 0) { ffgpu_set_error("%s: scene %d: zone %d: reserved must be 0", what, s, z); return -1; }
        }
        for (int l = 0; l < c.nlines; l++) {
            const ffgpu_line &ln = c.line[l];
            if (!isfinite(ln.ax) || !isfinite(ln.ay) || !isfinite(ln.bx) || !isfinite(ln.by)) { ffgpu_set_error("%s: scene %d: line %d is not finite", what, s, l); return -1; }
            if (ln.ax == ln.bx && ln.ay == ln.by) { ffgpu_set_error("%s: scene %d: line %d: A equals B", what, s, l); return -1; }
        }
    }
    return 0;
}

inline int ffgpu_zones_spec_check(const char *what, const ffgpu_zones_spec *sp)
{
    if (!sp) { ffgpu_set_error("%s: NULL spec", what); return -1; }
    if (sp->capacity < 1 || sp->capacity > FFGPU_ZONES_DETS) { ffgpu_set_error("%s: capacity %d is outside 1..%d", what, sp->capacity, FFGPU_ZONES_DETS); return -1; }
    if (sp->max_missed < 0 || sp->max_missed > (1 << 20)) { ffgpu_set_error("%s: max_missed %d is outside 0..2^20", what, sp->max_missed); return -1; }
    if (sp->identity != FFGPU_ZONES_NONE && sp->identity != FFGPU_ZONES_TYPE && sp->identity != FFGPU_ZONES_IDS) {
        ffgpu_set_error("%s: identity %d is none of FFGPU_ZONES_NONE, _TYPE, _IDS", what, sp->identity);
        return -1;
    }
    if (sp->flags & ~FFGPU_ZONES_GATE_INVERT) { ffgpu_set_error("%s: unknown flags 0x%x", what, (unsigned)sp->flags); return -1; }
    if (!(sp->min_score >= 0.f && sp->min_score <= 1.f)) { ffgpu_set_error("%s: min_score %g is not in [0, 1]", what, (double)sp->min_score); return -1; }
    if (sp->reserved != 0) { ffgpu_set_error("%s: spec: reserved must be 0", what); return -1; }
    return 0;
}

// what the operator and the executor form check alike, before either looks at its records
inline int ffgpu_zones_args_check(const char *what, const int *streams, int ntargets, const ffgpu_zones_spec *spec, const void *d_scenes, const void *d_state,
                                  int nstreams, const void *d_ids, const void *d_events, const void *d_out_records, const void *d_out_lists)
{
    if (!streams) { ffgpu_set_error("%s: NULL streams", what); return -1; }
    if (ffgpu_zones_spec_check(what, spec)) return -1;
    if (!d_scenes) { ffgpu_set_error("%s: NULL scenes", what); return -1; }
    if (!d_state) { ffgpu_set_error("%s: NULL state", what); return -1; }
    if (!d_events) { ffgpu_set_error("%s: NULL events", what); return -1; }
    if (spec->identity == FFGPU_ZONES_IDS && !d_ids) { ffgpu_set_error("%s: NULL ids with identity FFGPU_ZONES_IDS", what); return -1; }
    if (spec->identity != FFGPU_ZONES_IDS && d_ids) { ffgpu_set_error("%s: ids given without identity FFGPU_ZONES_IDS", what); return -1; }
    if (ffgpu_streams_check(what, ntargets, nstreams, d_state)) return -1;
    if (reinterpret_cast<uintptr_t>(d_scenes) & 3) { ffgpu_set_error("%s: the scenes must be 4-byte aligned", what); return -1; }
    if (d_out_lists && !d_out_records) { ffgpu_set_error("%s: d_out_lists without d_out_records", what); return -1; }
    return ffgpu_stream_range_check(what, streams, ntargets, nstreams);
}
