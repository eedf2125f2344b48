// ffgpu_dev.hpp -- shared declarations of the HIP side of libffcnn_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "ffgpu_internal.h"
#include "ffgpu_args.hpp"
#include "ffgpu_streams_host.hpp"
#include "ffgpu_track_host.hpp"
#include "ffgpu_zones_host.hpp"
#include "ffgpu_text_host.hpp"
#include "ffgpu_lines_host.hpp"
#include "ffgpu_trails_host.hpp"
#include "ffgpu_heat_host.hpp"
#include "ffgpu_motion_host.hpp"
#include "ffgpu_preview_host.hpp"
#include "ffgpu_warp_host.hpp"

#define FFGPU_CHECK(expr)                                                                   \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) {                                                             \
            ffgpu_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return -1;                                                                      \
        }                                                                                   \
    } while (0)

// One grouped convolution on device tensors.  Strides are in floats:
// element (c, n, y, x) of the input lives at in + c*in_cs + n*in_ns + y*iw + x.
// CNHW tensors have cs = N*h*w, ns = h*w; the frame-major batch input has
// cs = h*w, ns = C*h*w.
struct ConvDesc {
    const float *in;
    const float *const *in_ind;   // optional: device slot holding the input pointer (the executor's parameter block);
                                  // when set the kernel reads *in_ind instead of `in` -- a captured graph then serves
                                  // every input buffer.  Only the kernels ffgpu_conv_supports_ind() names honour it.
    const float *filt;     // fn rows of K4+4 floats (conv.h layout)
    float       *out;
    const float *residual; // optional: out = act2(conv_act(...) + residual), same layout as out (fused shortcut)
    const float *wpack;    // optional: plan-time weight image (ffgpu_pw_pack_floats / ffgpu_pw_pack) of the kernel AUTO picks; a launch of any other kernel ignores it
    int   N;
    int   iw, ih, ic;
    int   ow, oh, oc;
    int   fs, stride, pad, groups;
    int   act;            // activation of the conv itself
    int   res_act;        // activation applied after adding the residual
    int   flags;          // FFGPU_COMPAT_V6
    long  in_cs, in_ns, out_cs, out_ns, res_cs, res_ns;
    int   nsplit;         // implicit-GEMM split-K factor frozen at plan time (ffgpu_conv_plan); 0 = decided at launch (single-layer calls)
    int   kernel;         // FFGPU_K_* frozen at plan time (ffgpu_conv_plan): ffgpu_launch_conv(AUTO), the pack size and the pack kernel all follow it,
                          // so a later change of the FFGPU_* tuning environment cannot pair one kernel with another kernel's weight image; 0 = pick at launch
    int   x3_mt;          // k_conv_x3's MT (16-row blocks per wave) / k_pw_x3t's RB (32-row blocks per wave): the layout of the packed image, frozen with the plan; 0 = decided at launch
    // the SPARSE form of a yolo head's input layer (ffgpu_conv_x3.inc; sp_classes == 0: none): the head's classes and objectness threshold, its list of
    // pixel quads (N ih iw / 4 ints) and the list's counter.  The packed image then holds the form's two row-permuted images behind the regular one.
    int   sp_classes;
    float sp_thresh;
    int  *sp_list, *sp_ctr;
};
// internal bit of ConvDesc::flags (never part of the public flag set): the step reads the executor's BATCH INPUT (frame-major, possibly through the
// parameter block) -- kernels that cannot read through ConvDesc::in_ind are not picked for it, so the one-graph-for-every-input property survives
#define FFGPU_F_BATCH_INPUT (1 << 30)

static inline int conv_k4(const ConvDesc &d) { return (d.fs * d.fs * (d.ic / d.groups) + 3) & ~3; }

// Fused 1x1 expand -> depthwise 3x3 -> 1x1 project [+ residual] on CNHW tensors.
// What ffgpu_irb_plan decided for one block, all of it: the kernel family and instantiation, the tile, the layout of the packed image and the launch
// shape.  The FFGPU_* tuning environment is read once, there; packing and every launch follow the plan, so a switch changed later cannot pair one
// kernel with another kernel's image.
enum { IRB_NONE = 0, IRB_THIN, IRB_WAVE, IRB_WG };   // not planned / refused; k_irb_thin (8 expanded channels, streaming); k_irbw, k_irbw2 (a wave owns a tile); k_irb (fallback)
struct IrbPlan {
    int family;
    int inst;                 // IRB_WAVE / IRB_WG: index into the family's table of instantiations (irbw_kernels[], irb_kernels[])
    int half;                 // IRB_WAVE: the "half last group" form of image and kernel (FFGPU_IRBW_HALF)
    int pack_floats;          // floats of the packed image
    int lds, grid, block;     // dynamic LDS bytes, workgroups, threads per workgroup
    int KS1, OT, NSI, NSO, TWq, TH, EW, EH, ngroups, G, WPB, big, x3, xl;   // IRB_WAVE: input-channel quads, 16-channel output tiles, input / output strips, tile and halo,
                              // 16-channel groups, waves per tile, tiles per workgroup, register budget, split-bf16 expand, LDS-resident split tile (OT, TH: IRB_WG too)
    int xcd, region;          // IRB_WAVE: tile order XCD by XCD; floats behind the shared constants (E slices, then the group split's partial sums)
    int TW, NF, ECH, NW, KS, wbufs, red_off;   // IRB_WG: tile width, frames per tile, channels per chunk, waves, waves per strip, chunk buffers in LDS, offset of the reduce scratch
    int band, front_band;     // IRB_THIN: rows per wave in k_irb_thin / in k_front
};
struct IrbDesc {
    const float *in; float *out; const float *residual;
    const float *w1, *wd, *w2;
    int N, H, W, OH, OW, ic, ec, oc, stride;
    int act1, actd, act2, res_act;
    const float *pk;          // packed constants (plan.pack_floats floats, filled by ffgpu_irb_pack)
    int flags;                // FFGPU_CONCURRENT: tile splits chosen for several chains in flight
    IrbPlan plan;             // ffgpu_irb_plan; a descriptor without one is refused by pack and launch
};
bool   ffgpu_irb_plan(IrbDesc &d);                     // false: no fused kernel takes the block.  Reads geometry, activations and flags; the pointers may follow
size_t ffgpu_irb_pack_floats(const IrbDesc &d);
int    ffgpu_irb_pack(const IrbDesc &d, float *pk, hipStream_t s);
int    ffgpu_launch_irb(const IrbDesc &d, hipStream_t s);
int    ffgpu_irb_plan_line(const IrbDesc &d, char *buf, size_t cap);   // the plan as one canonical line of text (ffgpu_irb_plan_text)
int    ffgpu_irb_thin_launch_line(const IrbDesc &d, char *buf, size_t cap);   // a planned thin block's launch as one line: single or paired form, band, tasks, grid (ffgpu_irb_thin_launch_text)
int    ffgpu_irb_s2_launch_line(const IrbDesc &d, char *buf, size_t cap);     // a planned block's launch as one line: the streaming stride-2 form (k_irb_thin_s2) or the planned key, frames per wave, band, tasks, grid (ffgpu_irb_s2_launch_text)
int    ffgpu_irb_keys(char *buf, size_t cap);                            // the key of every instantiation of the three families, one per line (ffgpu_irb_instantiations)
// a run of B >= 2 blocks on one small plane (48 -> 224 -> 48, stride 1, linear project and shortcut) as one launch, one frame per workgroup
// (ffgpu_irb_stage.inc): the blocks' own planned descriptors, whose packed images the kernel reads; in = blocks[0].in, out = blocks[B - 1].out
#define IRBS_MAXB 8              /* blocks in a run */
bool   ffgpu_irb_stage_ok(const IrbDesc *blocks, int B);
int    ffgpu_launch_irb_stage(const IrbDesc *blocks, int B, hipStream_t s);
int    ffgpu_irb_stage_line(const IrbDesc *blocks, int B, bool wanted, char *buf, size_t cap);   // one launch ("stage ...") or B of them ("blocks ..."), as one line of text
bool   ffgpu_front_ok(const ConvDesc &c, const IrbDesc &d);      // first layer (3x3 s2, 3 -> 8) + thin block as one streaming kernel
// How a forward's batch arrives.  IN_F32: fp32 frames (ExecParams::frames; the staging kernels of ffgpu_input.inc write them for u8 sources the first
// kernel cannot take).  The u8 forms are read by k_front itself: IN_U8 frames of the net's own geometry (ExecParams::bgr), IN_BGR_FRAMES / IN_NV12_FRAMES
// frames of any size, one descriptor each in ExecParams::frames_tab.  An executor keeps one captured graph per form.
enum InputForm { IN_F32, IN_U8, IN_BGR_FRAMES, IN_NV12_FRAMES, IN_FORMS };
int    ffgpu_launch_front(const ConvDesc &c, const IrbDesc &d, InputForm form, hipStream_t s);
bool   ffgpu_front_nv12_fused();                                 // NV12 frames go into the NV12 form of k_front where the plan has it (FFGPU_NV12_FRONT, else the measured default)
int    ffgpu_front_plan_line(const IrbDesc &d, InputForm form, char *buf, size_t cap);   // the instantiation and launch shape for `form` as one line of text (ffgpu_front_plan_text)
int    ffgpu_front_nc(const IrbDesc &d);                         // output columns per lane k_front uses for this block (3 or 4; the resizing form: 3 only)

// depthwise K x K (stride 1, same padding) + pointwise 1 x 1 as one launch (ffgpu_dwpw.inc); dw.out == pw.in is never written
bool   ffgpu_dwpw_ok(const ConvDesc &dw, const ConvDesc &pw);
size_t ffgpu_dwpw_pack_floats(const ConvDesc &dw, const ConvDesc &pw);
int    ffgpu_dwpw_pack(const ConvDesc &dw, const ConvDesc &pw, float *pk, hipStream_t s);
int    ffgpu_launch_dwpw(const ConvDesc &dw, const ConvDesc &pw, const float *wpack, hipStream_t s);

size_t ffgpu_pw_pack_floats(const ConvDesc &d);
void   ffgpu_conv_plan(ConvDesc &d);                   // freezes kernel / nsplit / x3_mt for this layer NOW (the tuning environment is read once, here)
int    ffgpu_pw_pack(const ConvDesc &d, float *pk, hipStream_t s);

// the forward's frame table (FrameDesc: ffgpu_args.hpp)
// NV12 -> BGR in 32-bit integers (include/ffcnn_hip.h): { yoff, cy, crv, cgu, cgv, cbu } per FFGPU_YUV_* matrix
#define FFGPU_YUV_MATRICES { { 16, 298, 409, 100, 208, 516 }, { 0, 256, 359, 88, 183, 454 }, { 16, 298, 459, 55, 136, 541 }, { 0, 256, 403, 48, 120, 475 } }
int  ffgpu_launch_set_frames(FrameDesc *d_tab, const FrameDesc *h_desc, int n, hipStream_t s);
// staging (ffgpu_input.inc): the table's frames (BGR, or NV12 converted where sampled) -> the fp32 batch the IN_F32 graph consumes
int  ffgpu_launch_input_frames(const FrameDesc *d_tab, bool nv12, float *out, int N, int W, int H, const float mean[3], const float norm[3], hipStream_t s);

// Per-executor parameter block in device memory: what changes from one forward to the next without changing the
// launch list.  A one-thread kernel (ffgpu_launch_set_params) rewrites it in stream order in front of the graph launch,
// so ONE instantiated graph serves every input buffer and every box scale (the first round keyed a graph cache on them).
struct ExecParams {
    const float *frames;      // this forward's batch input (frame-major N x C x H x W)
    int s1, s2;               // box rescale ratio (ffcnn.c:267-273), applied by k_nms
    ffgpu_frame_dets *ring;   // record ring of the multi-GPU gather (ffgpu_exec_set_ring), or NULL
    int ring_slots, ring_stride;
    int bbox_max;             // NET.bbox_max of this forward: the reference re-reads it on every net_forward (ffcnn.c:461-463)
    // form IN_U8: u8 BGR frames of the net's own geometry, converted by the first kernel itself (k_front<.., true>; NULL: every other form)
    const unsigned char *bgr;
    long  bgr_frame;          // bytes from one frame to the next
    int   bgr_pitch;          // bytes per image row (ALIGN(3 w, 4), ffcnn.c:262)
    float mean[3], norm[3];   // the u8 forms: net_input's per-channel mean / norm (plane order R, G, B); IN_F32: zero
    // ffgpu_exec_forward_bgr_frames_dev / _nv12_frames_dev, fused (IN_BGR_FRAMES / IN_NV12_FRAMES) or staged (IN_F32): this forward's per-frame table
    // (N entries; k_nms takes each frame's s1 / s2 from it, the resizing k_front its source); NULL for every other entry point
    const FrameDesc *frames_tab;
};
int  ffgpu_launch_set_params(ExecParams *d_prm, const ExecParams &v, hipStream_t s);
bool ffgpu_conv_supports_ind(const ConvDesc &d);    // the kernel ffgpu_launch_conv would pick reads ConvDesc::in_ind

// true, with "<what>: no HIP device visible ..." as the error: what every entry point that needs no executor asks first (ffgpu_exec.hip)
bool ffgpu_no_device(const char *what);

// kernels.hip
int         ffgpu_launch_conv(const ConvDesc &d, int variant, hipStream_t s);
const char *ffgpu_conv_kernel_name(const ConvDesc &d, int variant);
int ffgpu_launch_pool(const float *in, float *out, int N, int c, int w, int h, int fs, int stride, int is_max, hipStream_t s);
int ffgpu_launch_spp(const float *in, float *const out[3], const int fs[3], int n, long planes, int w, int h, hipStream_t s);
int ffgpu_launch_upsample(const float *in, float *out, long planes, int w, int h, int stride, hipStream_t s);
int ffgpu_launch_add_act(const float *a, const float *b, float *out, long n, int act, hipStream_t s);
int ffgpu_launch_copy(const float *src, float *dst, long n, hipStream_t s);
int ffgpu_launch_hash64(const float *x, long n, unsigned long long *out, hipStream_t s);
int ffgpu_launch_input_bgr(const unsigned char *bgr, float *out, int N, int w, int h, int W, int H,
                           int sw, int sh, int s1, int s2, const float mean[3], const float norm[3], hipStream_t s);

struct YoloHead {
    const float *in;       // CNHW, 3*(5+classes) channels
    int   w, h, classes;
    int   anchors[3][2];
    float thresh, scale_xy;
    int   key_base;        // emission-order key of this head's first candidate
};
// cand / cand_key: `cap` slots per frame (cap = 3 * cells summed over the heads: every anchor of every cell has a slot, so
// the decode never drops a candidate -- the reference's buffer holds bbox_max = 51 200 of them, ffcnn.c:243,463)
int ffgpu_launch_yolo(const YoloHead &hd, int N, int netw, int neth, BBOX *cand, int *cand_key, int *ncand, int cap, int *ring_ctr, int *sp_ctr, hipStream_t s);
// may the pointwise layer d in front of a yolo head of `classes` classes run in the sparse form (shape and kernel; the knob and the executor's flags are the caller's)
bool ffgpu_conv_sparse_head_ok(const ConvDesc &d, int classes);
int  ffgpu_conv_sparse_head_line(const ConvDesc &d, int classes, bool wanted, char *buf, size_t cap);   // that layer's launch as one line of text (ffgpu_sparse_head_launch_text)
// full (may be NULL): cap boxes per frame, ALL survivors in score order (the fixed-size record keeps the first FFGPU_MAX_DET)
// bbox_max: the reference stops appending candidates at net->bbox_max in emission order (ffcnn.c:463); same here
// scratch (cap_pow2 > FFGPU_NMS_LDS_CAP only): 12 bytes x cap_pow2 per frame of global memory instead of LDS
int ffgpu_launch_nms(const BBOX *cand, const int *cand_key, int *ncand, int cap, BBOX *full, void *scratch,
                     ffgpu_frame_dets *dets, ffgpu_frame_dets *dets_host, const int *ring_ctr, int N,
                     float thresh, int use_min, const ExecParams *prm, hipStream_t s);
#define FFGPU_NMS_LDS_CAP 8192
bool ffgpu_nms_in_lds(int cap_pow2);      // the work arrays of cap_pow2 slots fit the CURRENT device's LDS (else: global scratch, 13 bytes per slot and frame)
int ffgpu_launch_clear(int *ncand, int N, int *ring_ctr, hipStream_t s);

// tiled detection (ffgpu_merge.inc): the caller's tile table as the CSR k_merge_tiles reads (checked entry by entry; off receives the pictures' offsets),
// its upload in stream order (ints by value as kernel arguments), and the merge of the tiles' records / lists per picture
int    ffgpu_merge_build_tab(const char *what, const ffgpu_tile *tiles, int ntiles, int nimages, std::vector<int> &tab, std::vector<int> *off);
size_t ffgpu_merge_tab_bytes(int ntiles);
int    ffgpu_launch_set_ints(int *d_dst, const int *h_src, int n, hipStream_t s);
int    ffgpu_launch_merge_tiles(const int *d_tab, const std::vector<int> &tab, const ffgpu_frame_dets *recs, const BBOX *lists, int stride,
                                float thresh, int use_min, ffgpu_frame_dets *out_recs, BBOX *out_lists, void *scratch, hipStream_t s);

// the detections drawn into the frames (ffgpu_draw.inc; DrawTarget: ffgpu_args.hpp).  targets[t] draws record t of `src`
int ffgpu_draw_style_check(const char *what, const ffgpu_draw_style *st, unsigned pal[256], int *npal);
int ffgpu_launch_draw(bool nv12, const DetSource &src, const std::vector<DrawTarget> &targets, const unsigned pal[256], int npal, int thickness, hipStream_t s);

// the detections cut out of the frames (ffgpu_crop.inc; CropSrc: ffgpu_args.hpp).  CropPlan: the caller's spec, checked, with the class filter's bytes copied.
struct CropPlan {
    int   out_w, out_h, form, per_target, nclasses, num, den;
    float min_score, mean[3], norm[3];
    unsigned char classes[256];
};
int ffgpu_box_sel_check(const char *what, int nclasses, const unsigned char *classes, int margin_num, int margin_den);
int ffgpu_crop_spec_check(const char *what, const ffgpu_crop_spec *sp, CropPlan &pl);
int ffgpu_crop_buffers_check(const char *what, const void *d_out, const void *d_table, int capacity);
int ffgpu_launch_crop(bool nv12, const DetSource &src, const std::vector<CropSrc> &sources, const CropPlan &pl, void *d_out, void *d_table, int capacity, hipStream_t s);

// the detections' regions redacted in the frames (ffgpu_redact.inc).  RedactPlan: the caller's spec, checked (nv12: the cell must be even), with the
// class filter's bytes copied and the colour packed as the draw's palette entries are.  targets[t] is redacted by record t of `src`
struct RedactPlan {
    int   mode, cell, outside, nclasses, num, den;
    float min_score;
    unsigned colour;
    unsigned char classes[256];
};
int ffgpu_redact_spec_check(const char *what, const ffgpu_redact_spec *sp, bool nv12, RedactPlan &pl);
int ffgpu_launch_redact(const char *what, bool nv12, const DetSource &src, const std::vector<DrawTarget> &targets, const RedactPlan &pl, hipStream_t s);

// the detections' regions blurred in the frames through a scratch surface per target (ffgpu_blur.inc).  BlurPlan: the caller's spec, checked, with the
// class filter's bytes copied.  targets[t] is blurred by record t of `src` through scratch[t]; ffgpu_launch_blur first holds the scratch table against
// the targets (same w x h, NULL where the target is, no overlap) and launches nothing when it does not fit
struct BlurPlan {
    int   radius, passes, outside, nclasses, num, den;
    float min_score;
    unsigned char classes[256];
};
int ffgpu_blur_spec_check(const char *what, const ffgpu_blur_spec *sp, BlurPlan &pl);
int ffgpu_launch_blur(const char *what, bool nv12, const DetSource &src, const std::vector<DrawTarget> &targets, const std::vector<DrawTarget> &scratch,
                      const BlurPlan &pl, hipStream_t s);

// what the reset of every per-stream family ends in (ffgpu_kernels.hip): ffgpu_state_span's checks (ffgpu_streams_host.hpp), then the bytes cleared on `stream`
int ffgpu_state_reset(const char *what, void *d_state, size_t all, int nstreams, int which_stream, void *stream);

// the detections tracked across a stream's frames (ffgpu_track.inc): the launches; the checks both entry points share are host code with no HIP in it
// (ffgpu_track_host.hpp)
int ffgpu_launch_track(const DetSource &src, const int *streams, int ntargets, const ffgpu_track_spec &spec, void *d_state, void *d_ids, void *d_out_records, void *d_out_lists, hipStream_t s);

// zones and lines (ffgpu_zones.inc): the launches; the checks both entry points share are host code with no HIP in it (ffgpu_zones_host.hpp)
int ffgpu_launch_zones(const DetSource &src, const int *streams, int ntargets, const ffgpu_zones_spec &spec, const void *d_scenes, void *d_state, const void *d_ids,
                       void *d_events, void *d_out_records, void *d_out_lists, hipStream_t s);

// captions (ffgpu_text.inc): the launches; the checks the entry points share are host code with no HIP in it (ffgpu_text_host.hpp).  targets[t] draws
// items t * items_stride ... of d_items; target t's items are composed from record t of `src`
int ffgpu_launch_draw_text(bool nv12, const void *d_items, int items_stride, const void *d_font, const std::vector<DrawTarget> &targets, hipStream_t s);
int ffgpu_launch_caption_boxes(const DetSource &src, int ntargets, const CaptionPlan &pl, const void *d_ids, void *d_items, int items_stride, hipStream_t s);

// outlines (ffgpu_lines.inc): the segment rasteriser's launches; the checks are host code with no HIP in it (ffgpu_lines_host.hpp)
int ffgpu_launch_draw_segments(bool nv12, const void *d_items, int items_stride, const std::vector<DrawTarget> &targets, hipStream_t s);

// track trails (ffgpu_trails.inc): the launches; the checks both entry points share are host code with no HIP in it (ffgpu_trails_host.hpp)
int ffgpu_launch_trails(const DetSource &src, const int *streams, int ntargets, const TrailsPlan &pl, void *d_state, const void *d_ids, void *d_rows, void *d_items,
                        int items_stride, int first_item, int nitems, hipStream_t s);

// heat maps (ffgpu_heat.inc): the accumulate launches; the checks both entry points share are host code with no HIP in it (ffgpu_heat_host.hpp)
int ffgpu_launch_heat(const DetSource &src, const int *streams, int ntargets, const HeatPlan &pl, void *d_state, void *d_rows, hipStream_t s);

// motion maps (ffgpu_motion.inc): the gate launches; the checks both entry points share are host code with no HIP in it (ffgpu_motion_host.hpp)
int ffgpu_launch_motion_gate(const DetSource &src, const int *streams, int ntargets, const MotionPlan &pl, const void *d_state, void *d_words, void *d_out_records,
                             void *d_out_lists, hipStream_t s);

// the crops classified (ffgpu_feature.inc): the checks both entry points share, and the launches.  Features: frame n of the tensor is frame n % pn of
// parts[n / pn], a CNHW tensor of pn frames (a split executor has one part per chain; at most 8).
int ffgpu_feature_args_check(const char *what, int n, int c, int h, int w, int pool, int post, const void *d_out, long out_stride);
int ffgpu_launch_features(const float *const *parts, int nparts, int pn, int c, int h, int w, int pool, int post, float *d_out, long out_stride, hipStream_t s);
int ffgpu_relabel_args_check(const char *what, const void *d_table, int capacity, const void *d_labels, int k, int ntargets, const ffgpu_relabel_spec *spec,
                             const void *d_out_records);
int ffgpu_launch_relabel(const void *d_table, int capacity, const void *d_labels, int k, const DetSource &src, int ntargets, const ffgpu_relabel_spec &spec,
                         void *d_out_records, void *d_out_lists, hipStream_t s);
