// ffgpu_motion_host.hpp -- the host side of the motion maps (include/ffcnn_hip.h: ffgpu_motion_state_bytes, ffgpu_motion_spec_check,
// ffgpu_motion_update_*_dev, ffgpu_motion_gate_dev, ffgpu_exec_motion_gate) before anything reaches the device: the state's layout, the spec
// resolved into a plan, the argument checks of the update and of the gate, and the rounds an update call is enqueued in.  Plain C++17 with no HIP in
// it: every function reports through ffgpu_set_error and touches no device, so san/motion_driver.cc runs the same lines on the CPU under
// ASan + UBSan (tests/test_motion_abi.py).  The targets and the class table's check are ffgpu_args.hpp's, the stream checks
// ffgpu_streams_host.hpp's.
#pragma once
#include "ffgpu_args.hpp"
#include "ffgpu_streams_host.hpp"

static_assert(sizeof(ffgpu_motion_spec) == 64, "include/ffcnn_hip.h states this size");
static_assert(FFGPU_MOTION_ENTRIES == 0 && FFGPU_MOTION_MERGED == 1, "ffgpu_source_exec: one check of `which` serves every family");
#define MOTION_STATE_HEADER 16                        // { int frames; int reserved[3] }
#define MOTION_ARG_TARGETS  64                        // targets per update launch, records per gate launch
#define MOTION_TILE         64                        // the side of an update tile, in pixels: whole cells at every legal cell size

// where a stream's parts lie in its block
struct MotionLayout {
    int    w, h, cell_log2, gw, gh, pitch;            // pitch: shorts from one row of the plane to the next, ALIGN(w, 8)
    size_t cells_off, stream_bytes;                   // the plane lies at MOTION_STATE_HEADER
};
inline bool ffgpu_motion_layout(int w, int h, int cell_log2, MotionLayout &l)
{
    if (w < 1 || w > FFGPU_MOTION_MAX_SIDE || h < 1 || h > FFGPU_MOTION_MAX_SIDE || cell_log2 < 2 || cell_log2 > 6) return false;
    const int c = 1 << cell_log2;
    l.w = w; l.h = h; l.cell_log2 = cell_log2; l.gw = (w + c - 1) >> cell_log2; l.gh = (h + c - 1) >> cell_log2; l.pitch = (w + 7) & ~7;
    l.cells_off = (size_t)MOTION_STATE_HEADER + 2 * (size_t)l.pitch * (size_t)h;
    l.stream_bytes = l.cells_off + ((4 * (size_t)l.gw * (size_t)l.gh + 15) & ~(size_t)15);
    return true;
}
inline size_t ffgpu_motion_state_bytes_host(int nstreams, int w, int h, int cell_log2)
{
    MotionLayout l;
    if (nstreams < 1 || nstreams > 65536 || !ffgpu_motion_layout(w, h, cell_log2, l)) return 0;
    return (size_t)nstreams * l.stream_bytes;
}

// a motion spec as the kernels read it: checked, the class table copied
struct MotionPlan {
    MotionLayout lay;
    int threshold, learn_shift, learn_shift_changed, min_pixels, cover, warmup, invert, nclasses;
    float min_score;
    unsigned char classes[256];
};

inline int ffgpu_motion_spec_plan(const char *what, const ffgpu_motion_spec *sp, MotionPlan &pl)
{
    if (!sp) { ffgpu_set_error("%s: NULL spec", what); return -1; }
    memset(&pl, 0, sizeof pl);
    if (sp->w < 1 || sp->w > FFGPU_MOTION_MAX_SIDE || sp->h < 1 || sp->h > FFGPU_MOTION_MAX_SIDE) {
        ffgpu_set_error("%s: a model of %d x %d pixels (1..%d each)", what, sp->w, sp->h, FFGPU_MOTION_MAX_SIDE);
        return -1;
    }
    if (sp->cell_log2 < 2 || sp->cell_log2 > 6) { ffgpu_set_error("%s: cell_log2 %d is outside 2..6", what, sp->cell_log2); return -1; }
    if (sp->threshold < 1 || sp->threshold > 255) { ffgpu_set_error("%s: threshold %d is outside 1..255", what, sp->threshold); return -1; }
    if (sp->learn_shift < 0 || sp->learn_shift > 16) { ffgpu_set_error("%s: learn_shift %d is outside 0..16", what, sp->learn_shift); return -1; }
    if (sp->learn_shift_changed < 0 || sp->learn_shift_changed > 16) { ffgpu_set_error("%s: learn_shift_changed %d is outside 0..16", what, sp->learn_shift_changed); return -1; }
    const int cc = 1 << (2 * sp->cell_log2);
    if (sp->min_pixels < 1 || sp->min_pixels > cc) { ffgpu_set_error("%s: min_pixels %d is outside 1..%d", what, sp->min_pixels, cc); return -1; }
    if (sp->cover < 1 || sp->cover > 256) { ffgpu_set_error("%s: cover %d is outside 1..256", what, sp->cover); return -1; }
    if (sp->warmup < 0 || sp->warmup > 65535) { ffgpu_set_error("%s: warmup %d is outside 0..65535", what, sp->warmup); return -1; }
    if (sp->flags & ~FFGPU_MOTION_GATE_INVERT) { ffgpu_set_error("%s: unknown flags 0x%x", what, (unsigned)sp->flags); return -1; }
    if (ffgpu_class_table_check(what, sp->classes, sp->nclasses)) return -1;
    if (sp->reserved[0] != 0 || sp->reserved[1] != 0) { ffgpu_set_error("%s: spec: reserved must be 0", what); return -1; }
    ffgpu_motion_layout(sp->w, sp->h, sp->cell_log2, pl.lay);
    pl.threshold = sp->threshold; pl.learn_shift = sp->learn_shift; pl.learn_shift_changed = sp->learn_shift_changed; pl.min_pixels = sp->min_pixels;
    pl.cover = sp->cover; pl.warmup = sp->warmup; pl.invert = (sp->flags & FFGPU_MOTION_GATE_INVERT) != 0; pl.nclasses = sp->nclasses; pl.min_score = sp->min_score;
    if (sp->classes) memcpy(pl.classes, sp->classes, (size_t)sp->nclasses);
    return 0;
}

// what every entry point with a state and streams checks alike (out: what the entry point calls its required output)
inline int ffgpu_motion_common_check(const char *what, const int *streams, int ntargets, const ffgpu_motion_spec *spec, const void *d_state, int nstreams,
                                     const void *d_out, const char *out, MotionPlan &pl)
{
    if (!streams) { ffgpu_set_error("%s: NULL streams", what); return -1; }
    if (ffgpu_motion_spec_plan(what, spec, pl)) return -1;
    if (!d_state) { ffgpu_set_error("%s: NULL state", what); return -1; }
    if (!d_out) { ffgpu_set_error("%s: NULL %s", what, out); return -1; }
    if (ffgpu_streams_check(what, ntargets, nstreams, d_state)) return -1;
    return ffgpu_stream_range_check(what, streams, ntargets, nstreams);
}

// The update's arguments: the spec, the state, the streams and the descriptors into the table the launches take.  tab[t].first carries the target's
// stream; a target of stream -1 or with a NULL address has p0 == NULL.  round[t]: the target is the round[t]-th frame of its stream in this call (a
// skipped target: round 0, where its zero row is written); the return value is the number of rounds, or -1.
template <class Frame>
int ffgpu_motion_update_args_check(const char *what, const Frame *targets, int ntargets, const int *streams, const ffgpu_motion_spec *spec, const void *d_state,
                                   int nstreams, const void *d_rows, MotionPlan &pl, std::vector<DrawTarget> &tab, std::vector<int> &round)
{
    if (!targets) { ffgpu_set_error("%s: NULL targets", what); return -1; }
    if (ffgpu_motion_common_check(what, streams, ntargets, spec, d_state, nstreams, d_rows, "rows", pl)) return -1;
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

// what the gate operator and the executor form check alike, before either looks at its records
inline int ffgpu_motion_gate_args_check(const char *what, const int *streams, int ntargets, const ffgpu_motion_spec *spec, const void *d_state, int nstreams,
                                        const void *d_words, const void *d_out_records, const void *d_out_lists, MotionPlan &pl)
{
    if (ffgpu_motion_common_check(what, streams, ntargets, spec, d_state, nstreams, d_words, "words", pl)) return -1;
    if (d_out_lists && !d_out_records) { ffgpu_set_error("%s: d_out_lists without d_out_records", what); return -1; }
    return 0;
}
