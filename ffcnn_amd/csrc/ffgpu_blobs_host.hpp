// ffgpu_blobs_host.hpp -- the host side of the motion blobs (include/ffcnn_hip.h: ffgpu_blobs_spec_check, ffgpu_blobs_dev) before anything reaches
// the device: the spec resolved into a plan, the LDS a workgroup of k_blobs needs for the plan's grid, and the argument checks.  Plain C++17 with
// no HIP in it: every function reports through ffgpu_set_error and touches no device.  The geometry and the state's layout are the motion maps'
// (ffgpu_motion_host.hpp), the stream checks ffgpu_streams_host.hpp's.
#pragma once
#include "ffgpu_motion_host.hpp"

static_assert(sizeof(ffgpu_blobs_spec) == 64, "include/ffcnn_hip.h states this size");
static_assert(FFGPU_BLOBS_MAX_CELLS == 32768 && FFGPU_BLOBS_COMPONENTS == 2048, "cell indices and component numbers share 16 bits with two markers");
#define BLOBS_ARG_TARGETS 64                          // targets per launch
#define BLOBS_LANES       1024                        // a workgroup of k_blobs: 16 waves
#define BLOBS_LDS_MAX     (160 * 1024)                // the LDS of a gfx950 compute unit

// a blobs spec as the kernel reads it, and where the parts of a workgroup's LDS lie (bytes from its start; 16-byte aligned each)
struct BlobsPlan {
    MotionLayout lay;
    int min_pixels, warmup, connect, min_cells, max_cells, max_boxes, pad, type;
    int ncell, wpr, ntab, npow2;                      // cells; 64-bit mask words per row; table entries; sort slots
    unsigned mask_off, tab_off, key_off, rank_off, lds;
    size_t label_pitch;                               // shorts from one target's labels to the next
};

// The LDS of a grid: the labels (a short per cell), the rows' bit masks, the table (6 words per entry), the sort keys, the components' ranks.  A
// grid of n cells has (n + 1) / 2 components at most, so a small grid has a small table.
inline void ffgpu_blobs_lds(BlobsPlan &pl)
{
    const unsigned a16 = 15u;
    pl.ncell = pl.lay.gw * pl.lay.gh;
    pl.wpr = (pl.lay.gw + 63) / 64;
    pl.ntab = std::min(FFGPU_BLOBS_COMPONENTS, (pl.ncell + 1) / 2);
    pl.npow2 = 1;
    while (pl.npow2 < pl.ntab) pl.npow2 <<= 1;
    pl.mask_off = (2u * (unsigned)pl.ncell + a16) & ~a16;
    pl.tab_off = pl.mask_off + 8u * (unsigned)(pl.wpr * pl.lay.gh);
    pl.key_off = (pl.tab_off + 24u * (unsigned)pl.ntab + a16) & ~a16;
    pl.rank_off = pl.key_off + 8u * (unsigned)pl.npow2;
    pl.lds = (pl.rank_off + 2u * (unsigned)pl.ntab + a16) & ~a16;
    pl.label_pitch = ((size_t)pl.ncell + 7) & ~(size_t)7;
}

inline int ffgpu_blobs_spec_plan(const char *what, const ffgpu_blobs_spec *sp, BlobsPlan &pl)
{
    if (!sp) { ffgpu_set_error("%s: NULL spec", what); return -1; }
    memset(&pl, 0, sizeof pl);
    if (sp->w < 1 || sp->w > FFGPU_MOTION_MAX_SIDE || sp->h < 1 || sp->h > FFGPU_MOTION_MAX_SIDE) {
        ffgpu_set_error("%s: a model of %d x %d pixels (1..%d each)", what, sp->w, sp->h, FFGPU_MOTION_MAX_SIDE);
        return -1;
    }
    if (sp->cell_log2 < 2 || sp->cell_log2 > 6) { ffgpu_set_error("%s: cell_log2 %d is outside 2..6", what, sp->cell_log2); return -1; }
    const int cc = 1 << (2 * sp->cell_log2);
    if (sp->min_pixels < 1 || sp->min_pixels > cc) { ffgpu_set_error("%s: min_pixels %d is outside 1..%d", what, sp->min_pixels, cc); return -1; }
    if (sp->warmup < 0 || sp->warmup > 65535) { ffgpu_set_error("%s: warmup %d is outside 0..65535", what, sp->warmup); return -1; }
    if (sp->connect != 4 && sp->connect != 8) { ffgpu_set_error("%s: connect %d is neither 4 nor 8", what, sp->connect); return -1; }
    if (sp->min_cells < 1 || sp->min_cells > FFGPU_BLOBS_MAX_CELLS) { ffgpu_set_error("%s: min_cells %d is outside 1..%d", what, sp->min_cells, FFGPU_BLOBS_MAX_CELLS); return -1; }
    if (sp->max_cells != 0 && (sp->max_cells < sp->min_cells || sp->max_cells > FFGPU_BLOBS_MAX_CELLS)) {
        ffgpu_set_error("%s: max_cells %d is neither 0 nor in %d..%d", what, sp->max_cells, sp->min_cells, FFGPU_BLOBS_MAX_CELLS);
        return -1;
    }
    if (sp->max_boxes < 1 || sp->max_boxes > FFGPU_MAX_DET) { ffgpu_set_error("%s: max_boxes %d is outside 1..%d", what, sp->max_boxes, FFGPU_MAX_DET); return -1; }
    if (sp->pad < 0 || sp->pad > 256) { ffgpu_set_error("%s: pad %d is outside 0..256", what, sp->pad); return -1; }
    if (sp->flags) { ffgpu_set_error("%s: unknown flags 0x%x", what, (unsigned)sp->flags); return -1; }
    for (int r : sp->reserved) if (r) { ffgpu_set_error("%s: spec: reserved must be 0", what); return -1; }
    ffgpu_motion_layout(sp->w, sp->h, sp->cell_log2, pl.lay);
    if ((long)pl.lay.gw * pl.lay.gh > FFGPU_BLOBS_MAX_CELLS) {
        ffgpu_set_error("%s: a grid of %d x %d cells (%d cells at most)", what, pl.lay.gw, pl.lay.gh, FFGPU_BLOBS_MAX_CELLS);
        return -1;
    }
    pl.min_pixels = sp->min_pixels; pl.warmup = sp->warmup; pl.connect = sp->connect; pl.min_cells = sp->min_cells; pl.max_cells = sp->max_cells;
    pl.max_boxes = sp->max_boxes; pl.pad = sp->pad; pl.type = sp->type;
    ffgpu_blobs_lds(pl);
    if (pl.lds > BLOBS_LDS_MAX) { ffgpu_set_error("%s: a grid of %d x %d cells needs %u bytes of LDS", what, pl.lay.gw, pl.lay.gh, pl.lds); return -1; }   // (no legal grid does)
    return 0;
}

inline int ffgpu_blobs_args_check(const char *what, const int *streams, int ntargets, const ffgpu_blobs_spec *spec, const void *d_state, int nstreams,
                                  const void *d_words, const void *d_out_records, BlobsPlan &pl)
{
    if (!streams) { ffgpu_set_error("%s: NULL streams", what); return -1; }
    if (ffgpu_blobs_spec_plan(what, spec, pl)) return -1;
    if (!d_state) { ffgpu_set_error("%s: NULL state", what); return -1; }
    if (!d_words) { ffgpu_set_error("%s: NULL words", what); return -1; }
    if (!d_out_records) { ffgpu_set_error("%s: NULL records", what); return -1; }
    if (ffgpu_streams_check(what, ntargets, nstreams, d_state)) return -1;
    return ffgpu_stream_range_check(what, streams, ntargets, nstreams);
}
