// ffgpu_heat_host.hpp -- the host side of the heat maps (include/ffcnn_hip.h: ffgpu_heat_state_bytes, ffgpu_heat_spec_check,
// ffgpu_heat_blend_spec_check, ffgpu_heat_palette, ffgpu_heat_boxes_dev, ffgpu_exec_heat, ffgpu_heat_blend_*_dev) before anything reaches the device:
// the state's size, the two specs resolved into plans, the built-in palette, the argument checks.  Plain C++17 with no HIP in it: every function
// reports through ffgpu_set_error and touches no device, so san/heat_driver.cc runs the same lines on the CPU under ASan + UBSan
// (tests/test_heat_abi.py).  The launch's entry table and the stream checks are ffgpu_streams_host.hpp's; the targets, the
// palette's packing and the class table's check are ffgpu_args.hpp's.
#pragma once
#include "ffgpu_args.hpp"
#include "ffgpu_streams_host.hpp"
#include "ffgpu_zones_host.hpp"

static_assert(sizeof(ffgpu_heat_spec) == 56 && sizeof(ffgpu_heat_blend_spec) == 48, "include/ffcnn_hip.h states these sizes");
static_assert(FFGPU_HEAT_ENTRIES == 0 && FFGPU_HEAT_MERGED == 1 && FFGPU_HEAT_DETS == FFGPU_ZONES_DETS, "ffgpu_source_exec: one check of `which` serves every family");
#define HEAT_STATE_HEADER 16                          // { int frames; unsigned peak; int reserved[2] }
#define HEAT_ARG_ENTRIES  64                          // records per accumulate launch
#define HEAT_ARG_TARGETS  64                          // targets per blend launch (the 1 KB palette travels with them)
#define HEAT_GRID_MAX     128                         // cells per side at most: 64 KB of LDS

// one stream's block: the header and gw x gh cells, rounded up to 16 bytes
inline size_t ffgpu_heat_stream_bytes(int gw, int gh) { return ((size_t)HEAT_STATE_HEADER + 4 * (size_t)gw * (size_t)gh + 15) & ~(size_t)15; }
inline size_t ffgpu_heat_state_bytes_host(int nstreams, int gw, int gh)
{
    if (nstreams < 1 || nstreams > 65536 || gw < 1 || gw > HEAT_GRID_MAX || gh < 1 || gh > HEAT_GRID_MAX) return 0;
    return (size_t)nstreams * ffgpu_heat_stream_bytes(gw, gh);
}

inline int ffgpu_heat_geometry_check(const char *what, int gw, int gh, int cell_log2)
{
    if (gw < 1 || gw > HEAT_GRID_MAX || gh < 1 || gh > HEAT_GRID_MAX) { ffgpu_set_error("%s: a grid of %d x %d cells (1..%d each)", what, gw, gh, HEAT_GRID_MAX); return -1; }
    if (cell_log2 < 1 || cell_log2 > 8) { ffgpu_set_error("%s: cell_log2 %d is outside 1..8", what, cell_log2); return -1; }
    return 0;
}

// a heat spec as the kernel reads it: checked, the class table copied
struct HeatPlan {
    int gw, gh, cell_log2, mode, anchor, spread, gain, decay_shift, nclasses;
    float min_score;
    unsigned char classes[256];
};

inline int ffgpu_heat_spec_plan(const char *what, const ffgpu_heat_spec *sp, HeatPlan &pl)
{
    if (!sp) { ffgpu_set_error("%s: NULL spec", what); return -1; }
    memset(&pl, 0, sizeof pl);
    if (ffgpu_heat_geometry_check(what, sp->gw, sp->gh, sp->cell_log2)) return -1;
    if (sp->mode != FFGPU_HEAT_ANCHOR && sp->mode != FFGPU_HEAT_BOX) { ffgpu_set_error("%s: mode %d is neither FFGPU_HEAT_ANCHOR nor FFGPU_HEAT_BOX", what, sp->mode); return -1; }
    if (sp->flags != 0) { ffgpu_set_error("%s: unknown flags 0x%x", what, (unsigned)sp->flags); return -1; }
    if (sp->anchor != 0 && sp->anchor != 1) { ffgpu_set_error("%s: anchor %d is neither 0 nor 1", what, sp->anchor); return -1; }
    if (sp->spread < 0 || sp->spread > 4) { ffgpu_set_error("%s: spread %d is outside 0..4", what, sp->spread); return -1; }
    if (sp->mode == FFGPU_HEAT_BOX && sp->spread != 0) { ffgpu_set_error("%s: spread %d with FFGPU_HEAT_BOX (0 then)", what, sp->spread); return -1; }
    if (sp->gain < 1 || sp->gain > 65536) { ffgpu_set_error("%s: gain %d is outside 1..65536", what, sp->gain); return -1; }
    if (sp->decay_shift < 0 || sp->decay_shift > 16) { ffgpu_set_error("%s: decay_shift %d is outside 0..16", what, sp->decay_shift); return -1; }
    if (ffgpu_class_table_check(what, sp->classes, sp->nclasses)) return -1;
    if (sp->reserved != 0) { ffgpu_set_error("%s: spec: reserved must be 0", what); return -1; }
    pl.gw = sp->gw; pl.gh = sp->gh; pl.cell_log2 = sp->cell_log2; pl.mode = sp->mode; pl.anchor = sp->anchor; pl.spread = sp->spread; pl.gain = sp->gain;
    pl.decay_shift = sp->decay_shift; pl.nclasses = sp->nclasses; pl.min_score = sp->min_score;
    if (sp->classes) memcpy(pl.classes, sp->classes, (size_t)sp->nclasses);
    return 0;
}

// the built-in palette: the ramp of include/ffcnn_hip.h, B G R 0, or converted to Y U V 0
inline void ffgpu_heat_palette_host(int nv12, unsigned char out[1024])
{
    static const int at[5] = { 0, 64, 128, 192, 255 };
    static const int col[5][3] = { { 255, 0, 0 }, { 255, 255, 0 }, { 0, 255, 0 }, { 0, 255, 255 }, { 0, 0, 255 } };
    auto clamp8 = [](int v) { return v < 0 ? 0 : v > 255 ? 255 : v; };
    for (int v = 0, s = 0; v < 256; v++) {
        if (v > at[s + 1]) s++;
        const int v0 = at[s], v1 = at[s + 1];
        int c[3];
        for (int k = 0; k < 3; k++) c[k] = (col[s][k] * (v1 - v) + col[s + 1][k] * (v - v0) + (v1 - v0) / 2) / (v1 - v0);
        if (nv12) {
            const int B = c[0], G = c[1], R = c[2];                               // (>> of a negative int: arithmetic, as the contract says)
            c[0] = clamp8((29 * B + 150 * G + 77 * R + 128) >> 8);
            c[1] = clamp8(((128 * B - 85 * G - 43 * R + 128) >> 8) + 128);
            c[2] = clamp8(((-21 * B - 107 * G + 128 * R + 128) >> 8) + 128);
        }
        out[4 * v] = (unsigned char)c[0]; out[4 * v + 1] = (unsigned char)c[1]; out[4 * v + 2] = (unsigned char)c[2]; out[4 * v + 3] = 0;
    }
}

// a blend spec as the kernel reads it: checked, the palette packed as the draw's entries are
struct HeatBlendPlan {
    int gw, gh, cell_log2, full_scale, floor, opacity, smooth, ramp;
    unsigned pal[256];
};

inline int ffgpu_heat_blend_spec_plan(const char *what, const ffgpu_heat_blend_spec *sp, bool nv12, HeatBlendPlan &pl)
{
    if (!sp) { ffgpu_set_error("%s: NULL spec", what); return -1; }
    memset(&pl, 0, sizeof pl);
    if (ffgpu_heat_geometry_check(what, sp->gw, sp->gh, sp->cell_log2)) return -1;
    if (sp->full_scale < 0) { ffgpu_set_error("%s: negative full_scale %d", what, sp->full_scale); return -1; }
    if (sp->floor < 0 || sp->floor > 255) { ffgpu_set_error("%s: floor %d is outside 0..255", what, sp->floor); return -1; }
    if (sp->opacity < 1 || sp->opacity > 255) { ffgpu_set_error("%s: opacity %d is outside 1..255", what, sp->opacity); return -1; }
    if (sp->sampling != FFGPU_HEAT_NEAREST && sp->sampling != FFGPU_HEAT_SMOOTH) {
        ffgpu_set_error("%s: sampling %d is neither FFGPU_HEAT_NEAREST nor FFGPU_HEAT_SMOOTH", what, sp->sampling);
        return -1;
    }
    if (sp->flags & ~FFGPU_HEAT_RAMP_ALPHA) { ffgpu_set_error("%s: unknown flags 0x%x", what, (unsigned)sp->flags); return -1; }
    if (sp->reserved[0] != 0 || sp->reserved[1] != 0) { ffgpu_set_error("%s: spec: reserved must be 0", what); return -1; }
    pl.gw = sp->gw; pl.gh = sp->gh; pl.cell_log2 = sp->cell_log2; pl.full_scale = sp->full_scale; pl.floor = sp->floor; pl.opacity = sp->opacity;
    pl.smooth = sp->sampling == FFGPU_HEAT_SMOOTH; pl.ramp = sp->flags & FFGPU_HEAT_RAMP_ALPHA;
    unsigned char own[1024];
    const unsigned char *src = sp->palette;
    if (!src) { ffgpu_heat_palette_host(nv12 ? 1 : 0, own); src = own; }
    int npal;
    return ffgpu_palette_plan(what, src, 256, nullptr, pl.pal, &npal);                  // (all 256 entries: the check inside cannot fail)
}

// what the accumulate operator and the executor form check alike, before either looks at its records
inline int ffgpu_heat_args_check(const char *what, const int *streams, int ntargets, const ffgpu_heat_spec *spec, const void *d_state, int nstreams,
                                 const void *d_rows, HeatPlan &pl)
{
    if (!streams) { ffgpu_set_error("%s: NULL streams", what); return -1; }
    if (ffgpu_heat_spec_plan(what, spec, pl)) return -1;
    if (!d_state) { ffgpu_set_error("%s: NULL state", what); return -1; }
    if (!d_rows) { ffgpu_set_error("%s: NULL rows", what); return -1; }
    if (ffgpu_streams_check(what, ntargets, nstreams, d_state)) return -1;
    return ffgpu_stream_range_check(what, streams, ntargets, nstreams);
}

// the blend's arguments: the spec, the state, the streams and the descriptors into the table the launches take (a target of stream -1: skipped)
template <class Frame>
int ffgpu_heat_blend_args_check(const char *what, const void *d_state, int nstreams, const int *streams, const Frame *targets, int ntargets,
                                const ffgpu_heat_blend_spec *spec, bool nv12, HeatBlendPlan &pl, std::vector<DrawTarget> &tab)
{
    if (!d_state) { ffgpu_set_error("%s: NULL state", what); return -1; }
    if (!streams) { ffgpu_set_error("%s: NULL streams", what); return -1; }
    if (!targets) { ffgpu_set_error("%s: NULL targets", what); return -1; }
    if (ffgpu_heat_blend_spec_plan(what, spec, nv12, pl)) return -1;
    if (ffgpu_streams_check(what, ntargets, nstreams, d_state)) return -1;
    if (ffgpu_stream_range_check(what, streams, ntargets, nstreams)) return -1;
    if (ffgpu_frame_table(what, FRAME_DRAW, targets, ntargets, tab)) return -1;
    for (int t = 0; t < ntargets; t++) {
        tab[t].first = streams[t];                                                // (the blend reads no list: the slot carries the stream)
        if (streams[t] < 0) tab[t].p0 = nullptr;
    }
    return 0;
}
