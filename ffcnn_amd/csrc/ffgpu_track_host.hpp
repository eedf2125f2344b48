// ffgpu_track_host.hpp -- the host side of the tracker (include/ffcnn_hip.h: ffgpu_track_state_bytes, ffgpu_track_boxes_dev, ffgpu_exec_track) before
// anything reaches the device: the state's size and the spec and argument checks (the launch's entry table and the stream checks are
// ffgpu_streams_host.hpp's).  Plain C++17 with no HIP in it: every function reports through ffgpu_set_error and touches no device, so
// san/track_driver.cc runs the same lines on the CPU under ASan + UBSan (tests/test_tracks_abi.py).
#pragma once
#include "ffcnn_hip.h"
#include "ffgpu_streams_host.hpp"

static_assert(sizeof(ffgpu_track) == 48 && sizeof(ffgpu_track_spec) == 32, "include/ffcnn_hip.h states these sizes");
#define TRACK_STATE_HEADER 16                         // { int issued, frames, live, reserved }

inline size_t ffgpu_track_state_bytes_host(int nstreams, int capacity)
{
    if (nstreams < 1 || nstreams > 65536 || capacity < 1 || capacity > FFGPU_TRACK_DETS) return 0;
    return (size_t)nstreams * (TRACK_STATE_HEADER + sizeof(ffgpu_track) * (size_t)capacity);
}

inline int ffgpu_track_spec_check(const char *what, const ffgpu_track_spec *sp)
{
    if (!sp) { ffgpu_set_error("%s: NULL spec", what); return -1; }
    if (sp->capacity < 1 || sp->capacity > FFGPU_TRACK_DETS) { ffgpu_set_error("%s: capacity %d is outside 1..%d", what, sp->capacity, FFGPU_TRACK_DETS); return -1; }
    if (sp->max_missed < 0 || sp->max_missed > (1 << 20)) { ffgpu_set_error("%s: max_missed %d is outside 0..2^20", what, sp->max_missed); return -1; }
    if (sp->min_hits < 1 || sp->min_hits > (1 << 20)) { ffgpu_set_error("%s: min_hits %d is outside 1..2^20", what, sp->min_hits); return -1; }
    if (!(sp->iou_thresh >= 0.f && sp->iou_thresh <= 1.f)) { ffgpu_set_error("%s: iou_thresh %g is not in [0, 1]", what, (double)sp->iou_thresh); return -1; }
    if (!(sp->min_score >= 0.f && sp->min_score <= 1.f)) { ffgpu_set_error("%s: min_score %g is not in [0, 1]", what, (double)sp->min_score); return -1; }
    if (!(sp->birth_score >= 0.f && sp->birth_score <= 1.f)) { ffgpu_set_error("%s: birth_score %g is not in [0, 1]", what, (double)sp->birth_score); return -1; }
    if (sp->class_aware != 0 && sp->class_aware != 1) { ffgpu_set_error("%s: class_aware %d is neither 0 nor 1", what, sp->class_aware); return -1; }
    if (sp->reserved != 0) { ffgpu_set_error("%s: spec: reserved must be 0", what); return -1; }
    return 0;
}

// what the operator and the executor form check alike, before either looks at its records
inline int ffgpu_track_args_check(const char *what, const int *streams, int ntargets, const ffgpu_track_spec *spec, const void *d_state, int nstreams,
                                  const void *d_ids, const void *d_out_records, const void *d_out_lists)
{
    if (!streams) { ffgpu_set_error("%s: NULL streams", what); return -1; }
    if (ffgpu_track_spec_check(what, spec)) return -1;
    if (!d_state) { ffgpu_set_error("%s: NULL state", what); return -1; }
    if (!d_ids) { ffgpu_set_error("%s: NULL ids", what); return -1; }
    if (ffgpu_streams_check(what, ntargets, nstreams, d_state)) return -1;
    if (d_out_lists && !d_out_records) { ffgpu_set_error("%s: d_out_lists without d_out_records", what); return -1; }
    return ffgpu_stream_range_check(what, streams, ntargets, nstreams);
}
