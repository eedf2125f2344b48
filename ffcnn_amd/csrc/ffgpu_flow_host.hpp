// ffgpu_flow_host.hpp -- the host side of the flow maps (include/ffcnn_hip.h: ffgpu_flow_state_bytes, ffgpu_flow_spec_check, ffgpu_flow_update_*_dev,
// ffgpu_flow_boxes_dev, ffgpu_exec_flow_boxes) before anything reaches the device: the state's layout, the spec resolved into a plan, the argument
// checks of the update and of the box operator, and the rounds an update call is enqueued in.  Plain C++17 with no HIP in it: every function reports
// through ffgpu_set_error and touches no device, so san/flow_driver.cc runs the same lines on the CPU under ASan + UBSan (tests/test_flow_abi.py).
// The targets and the class table's check are ffgpu_args.hpp's, the stream checks ffgpu_streams_host.hpp's; the wording of a rejection is the motion
// maps' (ffgpu_motion_host.hpp) wherever the reason is the same.
#pragma once
#include "ffgpu_args.hpp"
#include "ffgpu_streams_host.hpp"

static_assert(sizeof(ffgpu_flow_spec) == 64, "include/ffcnn_hip.h states this size");
static_assert(FFGPU_FLOW_ENTRIES == 0 && FFGPU_FLOW_MERGED == 1, "ffgpu_source_exec: one check of `which` serves every family");
#define FLOW_STATE_HEADER 16                          // { int frames; int gdx; int gdy; int support; }
#define FLOW_ARG_TARGETS  64                          // targets per update launch, records per box launch
#define FLOW_TILE_W       64                          // an update tile, in pixels: whole blocks at both block sizes
#define FLOW_TILE_H       32
#define FLOW_MAX_RANGE    16

// where a stream's parts lie in its block
struct FlowLayout {
    int    w, h, block_log2, gw, gh, pitch;           // pitch: bytes from one row of a luma plane to the next, ALIGN(w, 16)
    size_t plane_bytes, recs_off, stream_bytes;       // plane p lies at FLOW_STATE_HEADER + p * plane_bytes
};
inline bool ffgpu_flow_layout(int w, int h, int block_log2, FlowLayout &l)
{
    if (w < 1 || w > FFGPU_FLOW_MAX_SIDE || h < 1 || h > FFGPU_FLOW_MAX_SIDE || block_log2 < 3 || block_log2 > 4) return false;
    const int b = 1 << block_log2;
    l.w = w; l.h = h; l.block_log2 = block_log2; l.gw = (w + b - 1) >> block_log2; l.gh = (h + b - 1) >> block_log2; l.pitch = (w + 15) & ~15;
    l.plane_bytes = (size_t)l.pitch * (size_t)h;
    l.recs_off = (size_t)FLOW_STATE_HEADER + 2 * l.plane_bytes;
    l.stream_bytes = l.recs_off + ((8 * (size_t)l.gw * (size_t)l.gh + 15) & ~(size_t)15);
    return true;
}
inline size_t ffgpu_flow_state_bytes_host(int nstreams, int w, int h, int block_log2)
{
    FlowLayout l;
    if (nstreams < 1 || nstreams > 65536 || !ffgpu_flow_layout(w, h, block_log2, l)) return 0;
    return (size_t)nstreams * l.stream_bytes;
}

// a flow spec as the kernels read it: checked, the class table copied
struct FlowPlan {
    FlowLayout lay;
    int range, min_spread, nclasses;
    float min_score;
    unsigned char classes[256];
};

inline int ffgpu_flow_spec_plan(const char *what, const ffgpu_flow_spec *sp, FlowPlan &pl)
{
    if (!sp) { ffgpu_set_error("%s: NULL spec", what); return -1; }
    memset(&pl, 0, sizeof pl);
    if (sp->w < 1 || sp->w > FFGPU_FLOW_MAX_SIDE || sp->h < 1 || sp->h > FFGPU_FLOW_MAX_SIDE) {
        ffgpu_set_error("%s: a model of %d x %d pixels (1..%d each)", what, sp->w, sp->h, FFGPU_FLOW_MAX_SIDE);
        return -1;
    }
    if (sp->block_log2 < 3 || sp->block_log2 > 4) { ffgpu_set_error("%s: block_log2 %d is outside 3..4", what, sp->block_log2); return -1; }
    if (sp->range < 1 || sp->range > FLOW_MAX_RANGE) { ffgpu_set_error("%s: range %d is outside 1..%d", what, sp->range, FLOW_MAX_RANGE); return -1; }
    if (sp->min_spread < 0 || sp->min_spread > 65535) { ffgpu_set_error("%s: min_spread %d is outside 0..65535", what, sp->min_spread); return -1; }
    if (sp->flags) { ffgpu_set_error("%s: unknown flags 0x%x", what, (unsigned)sp->flags); return -1; }
    if (ffgpu_class_table_check(what, sp->classes, sp->nclasses)) return -1;
    for (int r : sp->reserved) if (r != 0) { ffgpu_set_error("%s: spec: reserved must be 0", what); return -1; }
    ffgpu_flow_layout(sp->w, sp->h, sp->block_log2, pl.lay);
    pl.range = sp->range; pl.min_spread = sp->min_spread; pl.nclasses = sp->nclasses; pl.min_score = sp->min_score;
    if (sp->classes) memcpy(pl.classes, sp->classes, (size_t)sp->nclasses);
    return 0;
}

// what every entry point with a state and streams checks alike (out: what the entry point calls its required output)
inline int ffgpu_flow_common_check(const char *what, const int *streams, int ntargets, const ffgpu_flow_spec *spec, const void *d_state, int nstreams,
                                   const void *d_out, const char *out, FlowPlan &pl)
{
    if (!streams) { ffgpu_set_error("%s: NULL streams", what); return -1; }
    if (ffgpu_flow_spec_plan(what, spec, pl)) return -1;
    if (!d_state) { ffgpu_set_error("%s: NULL state", what); return -1; }
    if (!d_out) { ffgpu_set_error("%s: NULL %s", what, out); return -1; }
    if (ffgpu_streams_check(what, ntargets, nstreams, d_state)) return -1;
    return ffgpu_stream_range_check(what, streams, ntargets, nstreams);
}

// The update's arguments, as ffgpu_motion_update_args_check resolves the motion maps': tab[t].first carries the target's stream; a target of stream
// -1 or with a NULL address has p0 == NULL.  round[t]: the target is the round[t]-th frame of its stream in this call (a skipped target: round 0,
// where its zero row is written); the return value is the number of rounds, or -1.
template <class Frame>
int ffgpu_flow_update_args_check(const char *what, const Frame *targets, int ntargets, const int *streams, const ffgpu_flow_spec *spec, const void *d_state,
                                 int nstreams, const void *d_rows, FlowPlan &pl, std::vector<DrawTarget> &tab, std::vector<int> &round)
{
    if (!targets) { ffgpu_set_error("%s: NULL targets", what); return -1; }
    if (ffgpu_flow_common_check(what, streams, ntargets, spec, d_state, nstreams, d_rows, "rows", pl)) return -1;
    if (ffgpu_frame_table(what, FRAME_DRAW, targets, ntargets, tab)) return -1;
    for (int t = 0; t < ntargets; t++)                                            // (a skipped target's size is not looked at: nothing of it is read)
        if (tab[t].p0 && streams[t] >= 0 && (tab[t].w != pl.lay.w || tab[t].h != pl.lay.h)) {
            ffgpu_set_error("%s: target %d: %d x %d pixels, the spec's model is %d x %d", what, t, tab[t].w, tab[t].h, pl.lay.w, pl.lay.h);
            return -1;
        }
    std::vector<int> seen((size_t)nstreams, 0);
    round.assign((size_t)ntargets, 0);
    int nrounds = 1;
    for (int t = 0; t < ntargets; t++) {
        tab[t].first = streams[t];
        if (streams[t] < 0) tab[t].p0 = nullptr;
        if (!tab[t].p0) continue;
        round[t] = seen[(size_t)streams[t]]++;
        nrounds = std::max(nrounds, round[t] + 1);
    }
    return nrounds;
}

// what the box operator and the executor form check alike, before either looks at its records
inline int ffgpu_flow_boxes_args_check(const char *what, const int *streams, int ntargets, const ffgpu_flow_spec *spec, const void *d_state, int nstreams,
                                       const void *d_words, FlowPlan &pl)
{
    return ffgpu_flow_common_check(what, streams, ntargets, spec, d_state, nstreams, d_words, "words", pl);
}
