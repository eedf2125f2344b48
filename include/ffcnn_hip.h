/*
 * ffcnn_hip.h -- additive, device-resident / batched C-ABI of libffcnn_hip.so.
 *
 * ffcnn.h and conv.h keep the reference's host-pointer interfaces (one frame,
 * H2D + D2H around every call).  Nothing in the reference has a batch
 * dimension or a device boundary, so the entry points below
 * are new names; each one states which reference code path it is the batched
 * counterpart of.  Plain C types only: pointers, sizes, ints.
 *
 * Device tensor layout ("CNHW"): a tensor of C channels for a batch of N frames
 * is C*N contiguous planes of H*W fp32, plane (c, n) at ((c*N + n)*H*W).  For
 * N == 1 this is exactly the reference's planar CHW tensor (ffcnn.c:436).  The
 * batch INPUT is the exception: frames are handed over frame-major, N x C x H x W
 * (each frame is one reference input tensor), and the first layer reads that.
 *
 * Error convention: functions returning int give 0 on success, negative on
 * failure; ffgpu_last_error() describes the last failure on the calling thread.
 * There is no CPU fallback anywhere: without a HIP device every call fails.
 */
#ifndef FFCNN_AMD_FFCNN_HIP_H
#define FFCNN_AMD_FFCNN_HIP_H

#include <stddef.h>
#include "ffcnn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FFGPU_MAX_DET   128   /* boxes per frame in the fixed-size RECORD (the gather unit); a frame with more keeps   */
                              /* all of them in the executor's full list: ffgpu_exec_read_boxes                        */

/* Candidate capacity: the reference appends candidates to a buffer of net->bbox_max = 51 200 entries (ffcnn.c:243,463).
 * Here every anchor of every head cell owns a slot (3 * cells summed over the heads: 1 500 per frame at 320x320), so the
 * decode never drops one; if a frame ever has more than net->bbox_max candidates, the FIRST bbox_max in the reference's
 * emission order go into NMS, as in the reference.  ffgpu_exec_cand_capacity() returns the slots per frame.
 * `ncand` and the candidate list (ffgpu_exec_read_layer, layer -2) are NOT cut at bbox_max: they hold every decoded candidate.
 * A candidate whose score is exactly 0 (ignore_thresh <= 0) is dead in NMS as in the reference (ffcnn.c:305,324): counted in ncand,
 * present among the candidates, never suppressing, in no list and no record.
 * Boxes are the reference's bit for bit (tests/detect_tail), with one exception: a coordinate that is NaN there is NaN here, but the
 * sign and payload of that NaN are unspecified (IEEE 754 leaves them to the implementation). */

/* Activations on non-finite values are the reference's (utils.h:15-23) in EVERY kernel, whichever one a layer or block is planned onto:
 * relu(x) is x > 0 ? x : 0, so relu(NaN) = 0 and relu(-Inf) = 0 (relu(+Inf) = +Inf); leaky(NaN) = NaN, leaky(-Inf) = -Inf; linear hands
 * every value on; sigmoid(+Inf) = 1, sigmoid(-Inf) = 0, sigmoid(NaN) = NaN.  A NaN or Inf that an activation does not remove propagates as
 * in conv-v0.c:7-31 (w * Inf = +-Inf, 0 * Inf = NaN).
 *
 * Non-finite INPUTS: this holds for every convolution kernel -- the plain fp32 ones (conv_generic, dw3_stream, dw_lds / dw_pair, pw_mfma,
 * pw_gemm, conv_dense8 / conv_first, conv_igemm, conv_thin, the fused dwpw pair), the opt-in pw_bf16 and the split-bf16 ones alike, with or
 * without a fused residual.  An output is non-finite exactly when its window (the taps INSIDE the plane, of its own group's channels) holds a
 * non-finite input: +-Inf with the sign of w * Inf where one Inf meets non-zero weights, NaN where it meets a zero weight, an Inf of the
 * opposite sign or a NaN.  Nothing else is touched: what a kernel reads only to fill a tile -- a padded k-slot that re-reads the last input
 * channel, a tap outside the plane loaded from a clamped address, a pixel beyond the last one -- counts as zero before it is multiplied, never
 * as 0 * x (tests/conv_kernels). */

/* Per-frame detection record as it lies in device (and gathered host) memory.
 * This is the unit the multi-GPU gather moves: fixed size, 16 + 128*24 bytes. */
typedef struct {
    int  count;               /* boxes valid in box[] (post-NMS, source-image coords): min(nfull, FFGPU_MAX_DET)     */
    int  ncand;               /* candidates that passed ignore_thresh before NMS                                      */
    int  overflow;            /* bit 0: ncand > bbox_max (truncated like the reference); bit 2: nfull > FFGPU_MAX_DET  */
                              /* (bit 1 is set by ffgpu_pack_records on frames that lost boxes to its cap)             */
    int  nfull;               /* boxes that survived NMS (all of them are in the executor's full list)                 */
    BBOX box[FFGPU_MAX_DET];
} ffgpu_frame_dets;

typedef struct ffgpu_exec ffgpu_exec;     /* a planned executor: one NET x one batch size */

/* executor flags */
#define FFGPU_KEEP_ALL   1    /* no arena reuse: every tensor that is materialised can be read */
                              /* back (combine with FFGPU_NO_FUSE for one tensor per layer)    */
#define FFGPU_COMPAT_V6  2    /* reproduce conv-v6.c:422-441 (5x5 depthwise row oh-2 defect) */
#define FFGPU_NO_GRAPH   4    /* launch kernels eagerly instead of replaying a HIP graph     */
#define FFGPU_NO_FUSE    8    /* one kernel per reference layer (no cross-layer fusion)      */
#define FFGPU_HOST_DETS  16   /* the NMS kernel also writes the records to a pinned host     */
                              /* mirror (ffgpu_exec_dets_host): no D2H copy after a forward   */
#define FFGPU_SPLIT2     32   /* even batch: the two halves run as two parallel branches of   */
                              /* one graph (same results; fills the latency gaps of the       */
                              /* small-plane launches); not with FFGPU_KEEP_ALL               */

#define FFGPU_CONCURRENT 64   /* several executors of this device run at the same time (one   */
                              /* stream each): plan for throughput -- the small planes' tiles  */
                              /* are split over fewer waves (less redundant work per wave; a   */
                              /* lone chain is ~4 % slower, four in flight ~3.5 % faster)      */

#define FFGPU_BF16_PW   128   /* OPT-IN reduced precision: compute-bound pointwise layers (ic, oc >= 128, >= 16 384 pixels) round  */
                              /* inputs and weights to bf16 and accumulate in fp32 on the bf16 matrix cores (16x the fp32 rate). */
                              /* Never the default: outputs then differ from the reference by up to 2^-7 scale' sum|w x| per   */
                              /* value (env FFGPU_BF16_PW=1 sets it for every executor).  yolo-fastest has no such layer.      */

/* ---- process / device --------------------------------------------------- */
int         ffgpu_device_count(void);
int         ffgpu_set_device(int ordinal);            /* hipSetDevice for this thread        */
const char *ffgpu_last_error(void);
const char *ffgpu_build_info(void);                   /* "gfx950 ... <git describe/date>"    */

/* ---- weights (counterpart of ffcnn.c:211-239's weight_buf, in HBM) ------ */
/* Device address and byte size of the folded filter rows (same layout as
 * NET.weight_buf).  This is the buffer a multi-GPU job broadcasts (RCCL). */
int ffgpu_net_weights_dev(NET *net, void **dev_ptr, size_t *bytes);
/* Call after writing the device weights from outside (e.g. after a broadcast):
 * refreshes derived device-side packings.  Runs on `stream` (hipStream_t or NULL). */
int ffgpu_net_weights_commit(NET *net, void *stream);

/* ---- batched forward (counterpart of net_forward, ffcnn.c:476-520) ------ */
ffgpu_exec *ffgpu_exec_create(NET *net, int batch, int flags);
void        ffgpu_exec_destroy(ffgpu_exec *ex);
int         ffgpu_exec_batch(const ffgpu_exec *ex);
size_t      ffgpu_exec_arena_bytes(const ffgpu_exec *ex);
int         ffgpu_exec_kernel_count(const ffgpu_exec *ex);   /* launches per forward */
/* What one forward of this plan must move and compute: bytes = per launch the tensors it reads / writes once each
 * (fused launches keep their inner tensors on chip), flops = 2 x multiply-adds of every conv layer (ffcnn.c:374-379). */
int         ffgpu_exec_work_model(const ffgpu_exec *ex, double *hbm_bytes, double *flops);

/* Box rescale ratio for every frame of the batch (what net_input derives per
 * image, ffcnn.c:267-273).  Default s1 = s2 = 1 (boxes in network pixels). */
int ffgpu_exec_set_scale(ffgpu_exec *ex, int s1, int s2);

/* d_frames: device pointer, batch x C x H x W fp32 (frame-major).  Enqueues the
 * whole net + YOLO decode + NMS on `stream` (hipStream_t; NULL = the executor's
 * own stream) and returns without synchronising.  The executor replays ONE HIP
 * graph whatever buffer d_frames points to (the pointer and the box scale travel
 * through a small device parameter block written in stream order in front of
 * the graph): handing over a fresh buffer per call costs nothing extra. */
int ffgpu_exec_forward_dev(ffgpu_exec *ex, const float *d_frames, void *stream);

/* Same, from host memory (H2D copy included), then waits for completion. */
int ffgpu_exec_forward_host(ffgpu_exec *ex, const float *h_frames);

/* u8 BGR frames on the device (batch x h x ALIGN(3w,4) bytes, all the same size)
 * -> letterboxed fp32 input + forward: the batched net_input (ffcnn.c:259-289)
 * fused in front of the net.  Sets the scale from (w,h) like net_input does. */
int ffgpu_exec_forward_bgr_dev(ffgpu_exec *ex, const unsigned char *d_bgr, int w, int h,
                               const float mean[3], const float norm[3], void *stream);

/* One u8 BGR frame of a mixed batch: its own device allocation, size and row pitch. */
typedef struct {
    const unsigned char *bgr;   /* device address of row 0 of this frame, B G R bytes per pixel, any byte alignment */
    int w, h;                   /* pixels, >= 1 */
    int pitch;                  /* bytes from one row to the next, >= 3 w; 0 = ALIGN(3 w, 4) as net_input (ffcnn.c:262) */
    int reserved;               /* 0 */
} ffgpu_bgr_frame;              /* 24 bytes */

/* frames: HOST array of `nframes` (== ffgpu_exec_batch(ex)) descriptors; the array is free again on return, the pixels must stay
 * valid until the forward completes.  Frame n = net_input(frames[n]) (ffcnn.c:259-289) with its own s1/s2, then the forward; records
 * of frame n are rescaled by frame n's s1/s2.  Enqueued on `stream` without synchronising, like ffgpu_exec_forward_bgr_dev.
 * On plans that start with the fused first kernel the letterbox resize runs inside it (no fp32 batch is written); the
 * executor's own scale (ffgpu_exec_set_scale) is left as it was. */
int ffgpu_exec_forward_bgr_frames_dev(ffgpu_exec *ex, const ffgpu_bgr_frame *frames, int nframes,
                                      const float mean[3], const float norm[3], void *stream);

/* NV12 -> BGR matrices of ffgpu_nv12_frame::matrix.  In 32-bit integers, with c = Y - yoff, d = U - 128, e = V - 128:
 *   R = clamp((cy c         + crv e + 128) >> 8, 0, 255)        (>> is arithmetic, the clamp comes last)
 *   G = clamp((cy c - cgu d - cgv e + 128) >> 8, 0, 255)
 *   B = clamp((cy c + cbu d         + 128) >> 8, 0, 255)
 *                                     yoff   cy  crv  cgu  cgv  cbu */
#define FFGPU_YUV_BT601_LIMITED 0   /*  16  298  409  100  208  516 */
#define FFGPU_YUV_BT601_FULL    1   /*   0  256  359   88  183  454 */
#define FFGPU_YUV_BT709_LIMITED 2   /*  16  298  459   55  136  541 */
#define FFGPU_YUV_BT709_FULL    3   /*   0  256  403   48  120  475 */

/* One NV12 frame of a mixed batch (what video decoders write): a full-resolution Y plane and a half-resolution plane of interleaved
 * U V pairs, (h + 1) / 2 rows of (w + 1) / 2 pairs; odd sizes are legal. */
typedef struct {
    const unsigned char *y;     /* device address of row 0 of the Y plane, any byte alignment                           */
    const unsigned char *uv;    /* device address of row 0 of the interleaved U V plane, 2-byte aligned;                */
                                /* NULL = y + pitch_y * h (one contiguous surface)                                      */
    int w, h;                   /* pixels, >= 1                                                                         */
    int pitch_y;                /* bytes between Y rows, >= w; 0 = w                                                    */
    int pitch_uv;               /* bytes between UV rows, even, >= 2 ((w + 1) / 2); 0 = that minimum                    */
    int matrix;                 /* FFGPU_YUV_*                                                                          */
    int reserved;               /* 0                                                                                    */
} ffgpu_nv12_frame;             /* 40 bytes */

/* ffgpu_exec_forward_bgr_frames_dev for NV12 frames: frame n = net_input (ffcnn.c:259-289) of the BGR image whose pixel (x, y) is the
 * formula above applied to Y[y][x], U = UV[y >> 1][2 (x >> 1)], V = UV[y >> 1][2 (x >> 1) + 1] (nearest chroma), then the forward.
 * net_input samples nearest-neighbour, so only the sampled pixels are converted, inside the kernel that samples them; no BGR image is
 * ever written.  Default route: k_input_nv12_frames writes the fp32 batch in front of the ordinary graph (staged).  FFGPU_NV12_FRONT=1
 * sends the frames into the NV12 form of the fused first kernel instead, on plans that start with it at three columns per lane (no fp32
 * batch; same records, byte for byte); it is not the default because it has not beaten staging by the margin DESIGN 5.15 asks for.
 * FFGPU_NO_U8_FRONT=1 forces staging whatever else is set.  Same contract: host array free on return, pixels valid until the forward completes, enqueued on
 * `stream` without synchronising, nframes == batch, 3-channel nets, the executor's own scale untouched.  Rejected with the frame's
 * index in the message: NULL y, w or h < 1, pitch_y < w, pitch_uv odd or below its minimum, an odd uv address, matrix outside 0..3,
 * reserved != 0.  A failed call leaves the executor usable. */
int ffgpu_exec_forward_nv12_frames_dev(ffgpu_exec *ex, const ffgpu_nv12_frame *frames, int nframes,
                                       const float mean[3], const float norm[3], void *stream);

/* Device address of the batch's ffgpu_frame_dets[batch] (valid after the
 * forward enqueued on the same stream completes). */
int ffgpu_exec_dets_dev(ffgpu_exec *ex, void **dev_ptr, size_t *bytes);
/* FFGPU_HOST_DETS executors: the pinned host mirror of the same `batch` records (valid once the
 * forward's stream has been synchronised); NULL + error otherwise. */
const ffgpu_frame_dets *ffgpu_exec_dets_host(ffgpu_exec *ex);
/* Record ring for the multi-GPU gather: from now on forward number k (k = 0, 1, ... counted on the device) ALSO
 * writes its `batch` records into slot k % slots of the caller-owned device buffer `dev_ring` (slots x batch
 * records), so groups of steps travel in one collective with no copy between graph launches.  Calling it again
 * (or with NULL) restarts the count / detaches.  Synchronises the executor's stream. */
int ffgpu_exec_set_ring(ffgpu_exec *ex, void *dev_ring, int slots);
/* The same with slot k at dev_ring + k * slot_records records (slot_records >= batch): E executors that take turns on E
 * streams share one ring when executor e gets dev_ring + e * batch records, slots / E slots and slot_records = E * batch
 * -- its forward k then lands in the ring's slot k * E + e, i.e. the global step number. */
int ffgpu_exec_set_ring_strided(ffgpu_exec *ex, void *dev_ring, int slots, int slot_records);
/* Synchronise the executor's last stream and copy the records to the host. */
int ffgpu_exec_read_dets(ffgpu_exec *ex, ffgpu_frame_dets *host_out, int max_frames);
/* ALL boxes of `frame` that survived NMS, score order, source-image coordinates (what the reference leaves in
 * net->bbox_list[0..bbox_num)): copies min(nfull, cap) of them and returns nfull.  Synchronises like read_dets. */
int ffgpu_exec_read_boxes(ffgpu_exec *ex, int frame, BBOX *host_out, int cap);
int ffgpu_exec_cand_capacity(const ffgpu_exec *ex);     /* candidate slots per frame (see above)                       */
int ffgpu_exec_graph_captures(const ffgpu_exec *ex);    /* HIP graphs captured so far by this executor (1 after any    */
                                                        /* number of forwards on any number of buffers)                */

/* FFGPU_KEEP_ALL executors only: copy layer `layer`'s OUTPUT for frame `frame`
 * into host_out (oc*oh*ow floats, reference CHW order).  layer == -1 gives the
 * network input as the first layer saw it.  Pre-NMS candidates: layer == -2
 * writes the frame's candidates (up to ffgpu_exec_cand_capacity() BBOX, in network
 * pixels, reference emission order) and returns their count. */
int ffgpu_exec_read_layer(ffgpu_exec *ex, int layer, int frame, float *host_out, size_t cap_floats);

/* FFGPU_KEEP_ALL executors only: host_out[i] = a 64-bit position-dependent hash of
 * layer i's output over the WHOLE batch (every bit of every frame; computed on
 * the device behind the last forward), 0 for layers this executor does not
 * materialise.  cap >= NET.layer_num.  Returns the number of layers hashed.
 * Two forwards of the same frames must give the same values: the reproducibility
 * watch of the concurrency tests reads 8 bytes per layer instead of activations. */
int ffgpu_exec_hash_layers(ffgpu_exec *ex, unsigned long long *host_out, int cap);

/* Mean device time per layer KIND over the last profiled forward, in micro-
 * seconds, indexed by LAYER_TYPE_* (counterpart of ENABLE_NET_PROFILE,
 * ffcnn.c:33,494-510).  Runs one eager forward with hipEvents around each step. */
int ffgpu_exec_profile(ffgpu_exec *ex, const float *d_frames, float us_by_kind[LAYER_TYPE_TOTOAL]);

/* Per-launch breakdown of one eager forward: for step i, layer_of[i] is the
 * reference layer index it implements (-1: executor bookkeeping), us[i] its
 * device time.  Returns the number of steps (<= cap) or a negative error. */
int ffgpu_exec_profile_steps(ffgpu_exec *ex, const float *d_frames, int *layer_of, float *us, int cap);
/* The HBM byte model of ffgpu_exec_work_model step by step: hbm_bytes[i] = what step i must move (its input and
 * output tensors and filter rows, each once), layer_of[i] as above.  Returns the number of steps (<= cap). */
int ffgpu_exec_step_model(const ffgpu_exec *ex, int *layer_of, double *hbm_bytes, int cap);

/* ---- all GPUs of one node from one C process (counterpart of calling net_forward once per frame) ------
 * A batch of `global_batch` independent frames is cut into contiguous shards, one per device (ffgpu_shard_range); every
 * device holds its own copy of the folded filter rows -- broadcast ONCE from rank 0 over RCCL (ncclBroadcast) inside
 * ffgpu_node_create -- and runs the whole net on its shard (own executor, stream and HIP graph); per forward the shards'
 * detection records are gathered on rank 0 (grouped ncclSend / ncclRecv over xGMI) and land in the caller's host buffer
 * in global frame order.  No all-reduce, no activation exchange.  RCCL is loaded at run time (librccl.so.1) the first
 * time a node is created without FFGPU_NODE_LOOPBACK; single-GPU users never load it. */
typedef struct ffgpu_node ffgpu_node;
#define FFGPU_NODE_LOOPBACK 1   /* node_flags: peer copies instead of RCCL; several ranks may share a device (tests) */
#define FFGPU_NODE_DEPTH(n) (((n) & 0xf) << 8)   /* node_flags: up to n (1..8) steps in flight: slot = step % n has its own executor, */
                                /* compute stream and input buffer per device and its own gather / host buffers                   */

/* frames [lo, hi) of `rank` out of `world`: sizes differ by at most one, earlier ranks take the extra */
void        ffgpu_shard_range(int total, int rank, int world, int *lo, int *hi);
/* devices: ndev device ordinals (rank 0 = the device `net` was loaded on) or NULL for that device and the next ndev - 1.
 * exec_flags: FFGPU_* executor flags for the per-device executors (FFGPU_COMPAT_V6, FFGPU_NO_GRAPH, FFGPU_SPLIT2 ...). */
ffgpu_node *ffgpu_node_create(NET *net, int ndev, const int *devices, int global_batch, int exec_flags, int node_flags);
void        ffgpu_node_destroy(ffgpu_node *node);
int         ffgpu_node_ndev(const ffgpu_node *node);
int         ffgpu_node_shard(const ffgpu_node *node, int rank, int *lo, int *hi, int *device);
int         ffgpu_node_set_scale(ffgpu_node *node, int s1, int s2);       /* as ffgpu_exec_set_scale, every rank */
int         ffgpu_node_depth(const ffgpu_node *node);
/* communicators ncclCommInitAll created for this node: ndev on the RCCL path, 0 with one device or FFGPU_NODE_LOOPBACK */
int         ffgpu_node_rccl_ranks(const ffgpu_node *node);
/* rank's input shard on ITS device, (hi - lo) x C x H x W fp32 frame-major, owned by the node (the buffer the NEXT
 * submitted step reads; ffgpu_node_input_slot_dev names a slot explicitly): fill it there ... */
float      *ffgpu_node_input_dev(ffgpu_node *node, int rank);
float      *ffgpu_node_input_slot_dev(ffgpu_node *node, int rank, int slot);
/* ... then run: forward on every device, gather, records of all global_batch frames to host_out; returns when they are there */
int         ffgpu_node_forward(ffgpu_node *node, ffgpu_frame_dets *host_out);
/* or hand over the whole batch in host memory (global_batch x C x H x W fp32): shards are copied to their devices first */
int         ffgpu_node_forward_host(ffgpu_node *node, const float *h_frames, ffgpu_frame_dets *host_out);
/* Pipelined form: submit enqueues the next step on every device (h_frames may be NULL: the slot's input buffers are used as
 * they are) plus its gather and returns the step's ticket (>= 0) without waiting; wait(ticket) blocks until that step's
 * records are on the host and copies them.  At most `depth` tickets may be outstanding.  h_frames is copied into the slot's
 * page-locked staging buffer before submit returns: the caller's buffer is free again at once -- with ONE exception: frames that
 * lie inside memory from ffgpu_host_alloc (page-locked memory this library owns) are uploaded straight from there by an
 * asynchronous DMA and must stay untouched until ffgpu_node_wait(ticket) has returned. */
long        ffgpu_node_submit(ffgpu_node *node, const float *h_frames);
int         ffgpu_node_wait(ffgpu_node *node, long ticket, ffgpu_frame_dets *host_out);
/* The loop above as one call: `steps` steps from the slots' input buffers, `depth` of them in flight (collect step i - depth,
 * submit step i), every step's records brought to the host; host_out (may be NULL) receives the last step's.  If a step fails the
 * steps still in flight are drained (their records dropped) before the error is returned: the node stays usable. */
int         ffgpu_node_run(ffgpu_node *node, long steps, ffgpu_frame_dets *host_out);

/* ---- single operators on device tensors (CNHW, any batch) --------------- */
/* Counterpart of groupconv (conv.h:4-7) without the host round trip.  d_in is
 * ic*batch planes of ih*iw, d_out oc*batch planes of oh*ow; d_filt as conv.h.
 * variant: 0 = auto (what the executor would pick), otherwise a specific kernel
 * id (FFGPU_K_*) for testing/benchmarking; unsupported combinations fail. */
int ffgpu_groupconv_dev(const float *d_in, const float *d_filt, float *d_out, int batch,
                        int iw, int ih, int ic, int groups, int pad, int stride,
                        int fs, int fn, int ow, int oh, int oc, int act,
                        int flags, int variant, void *stream);

enum {
    FFGPU_K_AUTO = 0,
    FFGPU_K_GENERIC = 1,      /* any fs/stride/pad/groups: one thread per output          */
    FFGPU_K_DW_STREAM = 2,    /* depthwise 3x3 s1: register sliding window, 16 B loads    */
    FFGPU_K_DW_LDS = 3,       /* depthwise 3x3/5x5, s1/s2: whole planes staged in LDS     */
    FFGPU_K_PW_MFMA = 4,      /* 1x1: fp32 MFMA 16x16x4, streaming (bandwidth-bound)      */
    FFGPU_K_PW_GEMM = 5,      /* 1x1: fp32 MFMA GEMM tile for compute-bound shapes (ic, oc >= 128) */
    FFGPU_K_DENSE_SMALL = 7,  /* dense 3x3/5x5 with <= 8 input channels (the first layer)   */
    FFGPU_K_IGEMM = 8,        /* dense KxK, groups == 1: implicit GEMM on fp32 MFMA (im2col gathered on the fly) */
    FFGPU_K_PW_BF16 = 9,      /* 1x1, opt-in (FFGPU_BF16_PW): bf16 inputs, fp32 accumulation, v_mfma_f32_32x32x16_bf16 */
    FFGPU_K_GROUP_THIN = 10,  /* 2..7 input channels per group (grouped or dense), any fs / stride / pad: scalar filter taps, several outputs per lane */
    FFGPU_K_PW_X3 = 11,       /* 1x1: fp32-equivalent results from SPLIT operands (three exact bf16 parts each, six partial products, fp32 accumulation) on v_mfma_f32_16x16x32_bf16 */
    FFGPU_K_CONV_X3 = 12,     /* dense 3x3 / stride 1 / pad 1, one group: the same split-operand arithmetic as FFGPU_K_PW_X3 (ffgpu_conv_x3.inc) */
    FFGPU_K_PW_X3T = 13       /* 1x1: the same split-operand arithmetic as a tiled, double-buffered GEMM (ffgpu_pw_x3t.inc): every input value split once per 256 output channels */
};

/* name of the kernel `variant` resolves to for this shape (for logs/benches) */
const char *ffgpu_groupconv_kernel_name(int batch, int iw, int ih, int ic, int groups, int pad,
                                        int stride, int fs, int fn, int variant);

/* Times `iters` launches of one conv on `stream` with hipEvents recorded on that
 * stream (after `warmup` untimed launches); returns mean microseconds per launch
 * or a negative value on error. */
float ffgpu_groupconv_time_dev(const float *d_in, const float *d_filt, float *d_out, int batch,
                               int iw, int ih, int ic, int groups, int pad, int stride,
                               int fs, int fn, int ow, int oh, int oc, int act,
                               int flags, int variant, int warmup, int iters, void *stream);

/* Fused block: 1x1 expand -> depthwise 3x3 (stride 1|2, pad 1) -> 1x1 project [+ residual], i.e.
 * three consecutive groupconv calls of the reference plus the shortcut that follows them
 * (ffcnn.c:418-423) in one kernel; the expanded tensors never leave the CU.  CNHW device
 * tensors; d_w1/d_wd/d_w2 are the three layers' filter rows (conv.h layout); d_res may be NULL.
 * iters > 0: returns mean microseconds per launch (HIP events on `stream`) instead of 0. */
float ffgpu_irb_dev(const float *d_in, const float *d_w1, const float *d_wd, const float *d_w2,
                    const float *d_res, float *d_out, int batch, int iw, int ih, int ic, int ec, int oc,
                    int stride, int act1, int actd, int act2, int res_act, int warmup, int iters, void *stream);

/* The same block as an executor created with `flags` (FFGPU_CONCURRENT or 0) plans and launches it: ffgpu_irb_dev is this call with flags 0. */
float ffgpu_irb_flags_dev(const float *d_in, const float *d_w1, const float *d_wd, const float *d_w2,
                          const float *d_res, float *d_out, int batch, int iw, int ih, int ic, int ec, int oc,
                          int stride, int act1, int actd, int act2, int res_act, int flags, int warmup, int iters, void *stream);

/* What the LAUNCH of a thin block (8 expanded channels, k_irb_thin) does, as one line of text in buf (at most cap bytes; returns snprintf's count):
 * "thin<IC,8,OC> W= H= N= band= nbands= ntasks= grid= block=" -- one frame per wave, the planned band and grid -- or
 * "thin_pair<IC,8,OC,NC> ..." -- two frames per wave, NC = 3, 4 or 5 columns per lane, the launch's own band and grid: taken where an NC divides
 * the row into at most 32 lanes, the batch has two frames, flags has FFGPU_CONCURRENT and FFGPU_THIN_PAIR is not 0 --, or "unsupported" for a
 * block the planner gives another family.  Arguments as ffgpu_irb_plan_text, whose line does not change with the form.  Pure host code. */
int ffgpu_irb_thin_launch_text(int batch, int iw, int ih, int ic, int ec, int oc, int stride, int act1, int actd, int act2, int res_act,
                               int flags, char *buf, int cap);

/* What the LAUNCH of a planned block does where the streaming stride-2 form (k_irb_thin_s2) may take it, as one line of text in buf (at most cap bytes;
 * returns snprintf's count): "thin_s2<4,24,8,3> frames= band= tasks= grid= block= W= H= N= lanes= nbands=" -- frames per wave, output rows per
 * task, the launch's own tasks and grid: taken where the block is stride 2 with 4 -> 24 -> 8 channels on an even-width plane, a row of the output
 * fits 32 lanes at three columns per lane and has at least three, the batch has at least two frames, the block has no residual, its input tensor fits
 * 32-bit offsets (under 2^30 floats), the activations are linear, relu or leaky, flags has FFGPU_CONCURRENT and FFGPU_THIN_S2 is not 0 --, or
 * "<planned key> frames= band= tasks= grid= block=" where the launch follows the plan, or "unsupported".  Arguments as ffgpu_irb_plan_text, whose
 * line does not change with the form.  Pure host code. */
int ffgpu_irb_s2_launch_text(int batch, int iw, int ih, int ic, int ec, int oc, int stride, int act1, int actd, int act2, int res_act,
                             int flags, char *buf, int cap);

/* The SPARSE form of the pointwise layer in front of a yolo head (3 anchors: ic -> 3 (5 + classes) channels, CNHW, batch ih iw a multiple of 4) on
 * caller-owned device tensors, as an FFGPU_CONCURRENT executor without FFGPU_KEEP_ALL / FFGPU_NO_FUSE runs it unless FFGPU_SPARSE_HEAD=0: a box pass writes the 15 box and
 * objectness channels of every pixel and appends to d_list (batch ih iw / 4 ints) the index of every quad of four consecutive pixels that holds a
 * (pixel, anchor) whose objectness can reach `thresh` (k_yolo's own test), counting them in *d_count; a class pass then writes the 3 x classes class
 * channels of the listed quads and of no other pixel.  Every value written has the bits of the dense launch (ffgpu_groupconv_dev, variant
 * FFGPU_K_CONV_X3).  *d_count is the caller's to zero before the call; a count above batch ih iw / 4 on entry makes the class pass take every quad.
 * List order is unspecified.  Returns 0, or -1 with ffgpu_last_error(). */
int ffgpu_sparse_head_dev(const float *d_in, const float *d_filt, float *d_out, int batch, int iw, int ih, int ic, int classes, int act,
                          float thresh, int *d_list, int *d_count, void *stream);

/* What an executor made with `flags` launches for that layer, as one line of text in buf (at most cap bytes; returns snprintf's count):
 * "sparse box<1,NW> rows=15 grid= class<MT,NW> rows= grid= quads= image=" -- the two passes' instantiations and workgroups, the list's capacity, the
 * dwords of the packed image (the regular one and the two row-permuted ones behind it) -- or "dense <kernel>".  Pure host code. */
int ffgpu_sparse_head_launch_text(int batch, int iw, int ih, int ic, int classes, int flags, char *buf, int cap);

/* What the planner decides for that block, as one line of text in buf (at most cap bytes; returns snprintf's count): the kernel
 * family and instantiation, every scalar of the parameter block the launch would pass, LDS bytes, grid, block, `half`, the floats
 * of the packed image -- or "unsupported".  flags: FFGPU_CONCURRENT or 0.  Pure host code (no device needed): for tests and logs. */
int ffgpu_irb_plan_text(int batch, int iw, int ih, int ic, int ec, int oc, int stride, int act1, int actd, int act2, int res_act,
                        int flags, char *buf, int cap);

/* What an executor of `batch` frames created with `flags` does with a run of `blocks` consecutive blocks 48 -> 224 -> 48 (stride 1, linear
 * projection and shortcut) on an iw x ih plane, as one line of text in buf (at most cap bytes; returns snprintf's count): "stage ..." with the
 * merged launch's parameter block, LDS bytes, grid and block where the run becomes one launch (FFGPU_CONCURRENT, at least 32 frames,
 * FFGPU_IRB_STAGE not 0, neither FFGPU_KEEP_ALL nor FFGPU_NO_FUSE, a plane the stage kernel holds), else "blocks ..." -- one launch per
 * block -- or "unsupported".  Pure host code (no device needed): for tests and logs. */
int ffgpu_irb_stage_plan_text(int batch, int iw, int ih, int blocks, int act1, int actd, int flags, char *buf, int cap);

/* Which instantiation of the first kernel (k_front: layers 0 - 3 of a net that starts like yolo-fastest) a batch takes and how it is
 * launched, as one line of text in buf (at most cap bytes; returns snprintf's count).  pw x ph is the 8-channel plane (the net input is 2 pw x 2 ph);
 * form: 0 fp32 frames, 1 u8 BGR frames of the net's size, 2 u8 BGR frames of any size, 3 NV12 frames.  The line reads
 * "front<OC,U8,NC,RS,NV> W= H= N= band= nbands= ntasks= grid= block=" (the template arguments: NC = output columns per lane, RS / NV = the resizing
 * BGR / NV12 gather), "staged" where the form has no instantiation for the plane, or "unsupported".  It describes the launch, not the planner's choice:
 * whether a plan starts with k_front at all also depends on the batch (FFGPU_FRONT_MIN_PX) and FFGPU_NO_FRONT.  Pure host code (no device needed): for tests and logs. */
int ffgpu_front_plan_text(int batch, int pw, int ph, int form, char *buf, int cap);

/* The key of every instantiation the fused-block families have -- the first word of ffgpu_irb_plan_text's line -- one per line in buf
 * (at most cap bytes; returns snprintf's count): the thin ones, then the wave ones, then the workgroup ones for both wave counts, read
 * from the tables the planner dispatches through.  Pure host code: for tests that must reach every one of them. */
int ffgpu_irb_instantiations(char *buf, int cap);

/* Every environment variable the library reads, one per line in buf (at most cap bytes; returns snprintf's count): name, kind of parse
 * (INT: unset or empty gives the default, else atoi; ON: atoi != 0; SET: present at all; TEXT: the string), default (`computed`: it depends
 * on the shape or the build; `-`: none), class (product, tuning, test, lab), the value a read would return now under the current
 * environment (TEXT: set / unset; a computed default: the number in the environment, or `default`), then what the variable does.  Pure
 * host code (no device needed).  INTEGRATION.md section 6 describes the variables; this is the table it is checked against. */
int ffgpu_knobs_text(char *buf, int cap);

/* Fused pair: depthwise K x K (K = 3 | 5, stride 1, pad K / 2) -> pointwise 1x1, i.e. two consecutive groupconv calls of the
 * reference in one kernel (the depthwise tensor never leaves the CU).  CNHW device tensors; d_wd / d_wp are the two layers'
 * filter rows (conv.h layout).  iters > 0: returns mean microseconds per launch (HIP events on `stream`) instead of 0. */
float ffgpu_dwpw_dev(const float *d_in, const float *d_wd, const float *d_wp, float *d_out, int batch, int iw, int ih,
                     int c, int oc, int fs, int actd, int actp, int warmup, int iters, void *stream);

/* ---- compact records for the multi-GPU gather ("fixed-size detection records to rank 0"): the
 * `batch` records of each of `nslots` steps (slot s starts at record s * slot_stride_records of d_records, e.g. a ring
 * set with ffgpu_exec_set_ring) are packed into nslots blocks of ffgpu_packed_records_bytes(batch, cap) bytes:
 *     int total, over, batch, cap | { int count, ncand, overflow, nfull } x batch | BBOX box[cap]
 * boxes of the frames behind each other in frame order (a frame's first box sits at the sum of the counts before it).  A step with more than `cap` boxes keeps the first `cap`
 * (over = 1, overflow |= 2 on the frames that lost boxes).  ffcnn_amd/dist.py unpacks them on the host. */
size_t ffgpu_packed_records_bytes(int batch, int cap);
/* host side: one packed block -> `batch` fixed-size records (unused box slots zero, as the NMS kernel leaves them).  Returns 0, or 1
 * if the block had dropped boxes / does not describe (batch, cap) -- the caller then fetches the full-size records --, -1 on bad arguments.
 * Pure host code (what ffgpu_node_wait runs on the gathered blocks). */
int    ffgpu_unpack_records(const void *block, int batch, int cap, ffgpu_frame_dets *out);
int    ffgpu_pack_records(const void *d_records, int nslots, long slot_stride_records, int batch, int cap, void *d_out, void *stream);

/* ---- tiled detection: the boxes of the tiles of a large picture merged on the device --------------------------------------------------
 * The net sees 320x320; a 1080p or 4K picture letterboxed down to it loses every small object.  The remedy is to cut the picture into
 * overlapping tiles and run the tiles as one batch: a tile is a frame descriptor (ffgpu_bgr_frame / ffgpu_nv12_frame) whose address is
 * bgr + y0 * pitch + 3 * x0 with the picture's pitch -- no copy.  What follows moves the tiles' boxes back into picture coordinates and
 * suppresses the duplicates the overlaps and the tile borders produce, without a host round trip.
 *
 * Batch entry t may be declared a tile of picture image[t] with origin (x0[t], y0[t]).  Its survivors are the forward's full post-NMS
 * list (nfull boxes in score order, in the tile's source pixels: what ffgpu_exec_read_boxes returns).  The merged result of picture g:
 *   1. every survivor of every tile of g is translated: x1 += (float)x0, x2 += (float)x0, y1 += (float)y0, y2 += (float)y0 (one fp32
 *      addition per coordinate, no FMA contraction);
 *   2. the union is ordered by score descending, then position of the tile in the caller's table ascending, then index in the tile's
 *      list ascending (a total order: identical pixels under two tiles give exact score ties);
 *   3. the greedy class-aware suppression of ffcnn.c:298-322 runs on it with the arithmetic of the forward's own NMS: area =
 *      (x2 - x1) * (y2 - y1), a box goes when metric > thresh, a suppressed box never suppresses another;
 *   4. the survivors are written in that order, not rescaled.
 * The merged record is an ffgpu_frame_dets: count = min(nfull, FFGPU_MAX_DET), nfull = survivors of the merge, ncand = sum of the tiles'
 * ncand, overflow bit 0 = OR of the tiles' bit 0, bit 2 = nfull > FFGPU_MAX_DET, unused box slots zero.
 * This is TWO-STAGE NMS -- per tile, then across tiles -- and deliberately not NMS over the union of the raw candidates.  With the
 * reference's metric (intersection / min area, ffcnn.c:316,519) a partial box cut off by a tile border lies inside the whole box the
 * neighbouring tile sees and scores near 1 against it.  A picture with one tile at (0, 0) gives that entry's own record; listing a tile
 * twice changes nothing; a picture without boxes (or without tiles) gives a zero record.  Boxes are not clipped to the picture. */
typedef struct {
    int image;                  /* 0 .. nimages-1, or -1: this batch entry is no tile (ignored) */
    int x0, y0;                 /* tile origin in the picture, >= 0 */
    int reserved;               /* 0 */
} ffgpu_tile;                   /* 16 bytes */

#define FFGPU_MERGE_LDS_SLOTS 1024   /* a picture whose tiles hold at most this many boxes together is merged in LDS (the normal case: tens); */
                                     /* a larger union is merged in the global scratch buffer: correct, not fast                             */

/* The operator, on device records and lists with no executor (like ffgpu_pack_records).  d_records: ntiles ffgpu_frame_dets; d_lists: tile
 * t's nfull boxes at box t * list_stride (nfull <= list_stride), or NULL: the records' own box[0 .. count).  tiles: HOST array, free on
 * return.  d_out_records: nimages records.  d_out_lists (may be NULL): the full list of picture g starts at box list_stride x (number of
 * tiles of pictures < g) -- FFGPU_MAX_DET takes list_stride's place when d_lists is NULL -- and has room for all of its tiles' boxes.
 * d_scratch (16-byte aligned, ffgpu_merge_tiles_scratch_bytes(ntiles, list_stride) bytes) may be NULL when no picture CAN exceed the LDS
 * slots (tiles of the picture x list_stride <= FFGPU_MERGE_LDS_SLOTS) and the table has at most 220 tiles; otherwise the call fails, with
 * a message, before anything is launched.  Enqueued on `stream` without synchronising.  Rejected with the entry's index in the message:
 * image outside -1 .. nimages-1, a negative origin, reserved != 0; also nimages < 1 or > ntiles and a NULL table. */
size_t ffgpu_merge_tiles_scratch_bytes(int ntiles, int list_stride);
int    ffgpu_merge_tiles_dev(const void *d_records, const void *d_lists, int list_stride, const ffgpu_tile *tiles, int ntiles, int nimages,
                             float thresh, int use_min, void *d_out_records, void *d_out_lists, void *d_scratch, size_t scratch_bytes, void *stream);

/* On an executor: enqueues the merge of the last forward's records and full lists behind it on `stream` (NULL = the executor's own; it
 * must be the stream of that forward), with the net's own setting (threshold 0.5, min-area metric).  ntiles == batch.  A post-pass: the
 * captured graph, the per-entry records and their ring / host mirror are untouched.  The tile table reaches the device in stream order
 * as a kernel argument, skipped while the table is unchanged on that stream: a steady tiling costs ONE extra launch per forward.  Buffers
 * belong to the executor (allocated by the first call).  Works on FFGPU_SPLIT2 executors.  A rejected call leaves the executor usable. */
int ffgpu_exec_merge_tiles(ffgpu_exec *ex, const ffgpu_tile *tiles, int ntiles, int nimages, void *stream);
/* the merged records on the device: `nimages` of the last merge (valid once it has completed) */
int ffgpu_exec_merged_dev(ffgpu_exec *ex, void **dev_ptr, size_t *bytes);
/* synchronise like ffgpu_exec_read_dets / ffgpu_exec_read_boxes and copy: the merged records (returns how many), ALL merged boxes of one
 * picture (copies min(nfull, cap), returns nfull) */
int ffgpu_exec_read_merged(ffgpu_exec *ex, ffgpu_frame_dets *host_out, int max_images);
int ffgpu_exec_read_merged_boxes(ffgpu_exec *ex, int image, BBOX *host_out, int cap);

/* The planner: pure host code, usable without a device (like ffgpu_shard_range).  Cuts an img_w x img_h picture into a grid of equal
 * tiles (rows of tiles, left to right, top to bottom) and returns their number -- also when `cap` is too small: the first `cap` are
 * written -- or -1.  Every tile has the same effective size min(tile, image), one pixel larger where align == 2 needs it; every tile lies
 * inside the picture, together they cover it, neighbours overlap by at least overlap - (align - 1) pixels, every origin is a multiple
 * of `align` (use 2 for NV12, whose chroma phase cannot shift by one pixel), the first tile starts at 0 and the last ends at the picture's
 * edge; the same arguments always give the same plan.  Rejected: sizes < 1, overlap < 0 or >= the tile size, align not 1 or 2, and align
 * 2 with a tile 1 pixel wide (high) in a wider (higher) picture, which even origins cannot cover. */
typedef struct { int x0, y0, w, h; } ffgpu_tile_rect;
int ffgpu_tile_plan(int img_w, int img_h, int tile_w, int tile_h, int overlap_x, int overlap_y, int align, ffgpu_tile_rect *out, int cap);

/* ---- the detections drawn into the frames on the device ---------------------------------------------------------------------------------
 * The reference's program ends by outlining its boxes in the picture (ffcnn.c:583-589, bmp_rectangle of bmpfile.c:145-156).  What follows does
 * that where the frames and the records already lie, in HBM, for u8 BGR and NV12 surfaces: no frame crosses the bus.
 *
 * One box, as the reference draws it.  Its integer corners are (a, b, c, d) = ((int)x1, (int)y1, (int)x2, (int)y2): truncated toward zero,
 * values outside int saturate, NaN gives 0 (what v_cvt_i32_f32 does; the C cast is undefined there, so this sentence is the definition).
 * Rectangle (a, b, c, d) is the pixel set of bmp_rectangle: (x, b) and (x, d) for a <= x <= c, (a, y) and (c, y) for b <= y <= d; a pixel
 * outside 0 <= x < w, 0 <= y < h of the target is dropped.  The quirks belong to the contract: with a > c and b <= d the two vertical lines
 * are still drawn, a box wholly outside draws nothing.  thickness = T draws the T rectangles (a + i, b + i, c - i, d - i), i = 0 .. T-1,
 * computed as if in 64-bit integers (no wrap-around); T = 1 is exactly the reference.
 * A target's result is what drawing its boxes serially in list order would leave: a later box overwrites an earlier one.  Only outline
 * pixels are written; every other byte of the target -- row padding, the pixels between the outlines, the memory before and behind it --
 * stays as it was.  The result does not depend on the order in which the device executes anything: the same bytes on every run.
 * BGR targets (ffgpu_bgr_frame): a drawn pixel becomes the three bytes B, G, R of the box's colour.
 * NV12 targets (ffgpu_nv12_frame; `matrix` is ignored): the colour is Y, U, V bytes, nothing is converted.  A drawn pixel (x, y) sets
 * Y[y][x] = Y and the chroma pair UV[y >> 1][x >> 1] = (U, V); the serial order holds per chroma sample too: the last box in list order
 * that touches any of the sample's up to four luma pixels gives it its value.  Odd widths and heights are legal.
 * A box of class `type` takes palette entry type mod npalette (the non-negative remainder), or `color` when there is no palette.
 * Targets: a descriptor keeps the meaning and the checks it has for the forward (BGR heights above 2^30 - 1 are rejected here as well), except
 * that a NULL pixel address (bgr, y) means "skip this target".  The descriptors' const pointers are WRITTEN THROUGH.  Targets of one call
 * must not overlap in memory; where they do, each overlapping byte holds one of the values written to it, which one is unspecified. */
typedef struct {
    unsigned char color[4];         /* the colour when palette is NULL: B G R 0 (BGR targets) / Y U V 0 (NV12 targets)          */
    const unsigned char *palette;   /* HOST array of npalette x 4 bytes (same byte order), or NULL                               */
    int npalette;                   /* 0 with a NULL palette, else 1..256                                                        */
    int thickness;                  /* 1..8                                                                                      */
} ffgpu_draw_style;                 /* 24 bytes: color at 0, palette at 8, npalette at 16, thickness at 20                       */

/* The operators, on device records and lists with no executor (like ffgpu_merge_tiles_dev).  Target t draws record t of d_records.
 * d_lists == NULL: the record's own box[0 .. count), count clamped to [0, FFGPU_MAX_DET].  Otherwise nfull boxes, clamped to
 * [0, list_stride], starting at box list_first[t] of d_lists, or at box t * list_stride when list_first is NULL; list_first is a HOST
 * array (merged lists do not start at a uniform stride).  Whatever the records hold, nothing is read or written outside the buffers and
 * the targets' w x h.  targets, list_first and style (with its palette) are HOST memory and free again on return.  Any ntargets >= 1;
 * the tables travel as kernel arguments, 64 targets per launch.  Enqueued on `stream` without synchronising.  Rejected before anything is
 * launched, with the target's index in the message where there is one: NULL records, targets or style, ntargets < 1, a bad list_stride, a
 * negative list start, thickness outside 1..8, npalette outside its range or inconsistent with palette, a descriptor the forward would
 * reject other than for a NULL address. */
int ffgpu_draw_boxes_bgr_dev (const void *d_records, const void *d_lists, int list_stride, const int *list_first,
                              const ffgpu_bgr_frame  *targets, int ntargets, const ffgpu_draw_style *style, void *stream);
int ffgpu_draw_boxes_nv12_dev(const void *d_records, const void *d_lists, int list_stride, const int *list_first,
                              const ffgpu_nv12_frame *targets, int ntargets, const ffgpu_draw_style *style, void *stream);

#define FFGPU_DRAW_ENTRIES 0   /* entry n's full post-NMS list into targets[n]; ntargets == batch                                      */
#define FFGPU_DRAW_MERGED  1   /* picture g's merged list (last ffgpu_exec_merge_tiles) into targets[g]; ntargets == its nimages        */
/* On an executor: a post-pass like ffgpu_exec_merge_tiles, enqueued on `stream` (NULL = the executor's own; it must be the stream of the
 * forward or merge it follows) without synchronising.  The captured graph, the records, the full lists, the ring and the host mirror are
 * untouched.  FFGPU_DRAW_ENTRIES with the very array handed to the forward draws each frame's boxes into that frame; a tile descriptor
 * draws the tile's boxes inside the tile.  Works on FFGPU_SPLIT2 executors.  Rejected like the operators, and: ntargets not as stated, a
 * `which` that is neither, FFGPU_DRAW_MERGED when no merge has run, the wrong stream.  A rejected call leaves the executor usable. */
int ffgpu_exec_draw_bgr (ffgpu_exec *ex, int which, const ffgpu_bgr_frame  *targets, int ntargets, const ffgpu_draw_style *style, void *stream);
int ffgpu_exec_draw_nv12(ffgpu_exec *ex, int which, const ffgpu_nv12_frame *targets, int ntargets, const ffgpu_draw_style *style, void *stream);

/* ---- the detections cut out of the frames on the device, for a second stage ---------------------------------------------------------------
 * A cascade looks again at each detected object -- with this net at full resolution, with another cfg, for a thumbnail.  What follows selects
 * boxes, resamples each one's region of its source frame into one slot of a caller-owned batch buffer exactly as net_input (ffcnn.c:259-289)
 * would if the region were an image of its own, and moves the boxes of a forward over those slots back into source coordinates; no record and
 * no frame crosses the bus.
 *
 * Sources: descriptors as the draw contract takes them (ffgpu_bgr_frame / ffgpu_nv12_frame with the draw contract's checks, a NULL pixel
 * address = "skip this source": none of its boxes take part); a w or h of 2^31 - 1 is rejected as well.  The sources are only read.
 *
 * Selection.  Sources are walked in ascending order, each one's list in list order.  A box QUALIFIES when score >= min_score (a NaN score never
 * does) and its class is allowed: every type with classes == NULL, else 0 <= type < nclasses and classes[type] != 0.  Its integer corners
 * (a, b, c, d) are the draw contract's (toward zero, saturating, NaN -> 0).  In 64-bit integers: mx = (c - a + 1) num / den,
 * my = (d - b + 1) num / den, X0 = max(a - mx, 0), X1 = min(c + mx, w - 1), Y0 = max(b - my, 0), Y1 = min(d + my, h - 1).  A qualifying box
 * with a > c or b > d, or with X0 > X1 or Y0 > Y1, is counted in `empty` (wherever it stands in its list) and takes nothing.  Every other
 * qualifying box is SELECTED until its source has per_target selected boxes.  `total` counts the selected boxes; the first taken =
 * min(total, capacity) of them, in that order, own slots 0 .. taken-1.
 * The table, in the caller's device memory (16-byte aligned, ffgpu_crop_table_bytes(capacity) bytes): a header { int total, taken, empty,
 * capacity } and `capacity` entries ffgpu_crop.  Entry n < taken: the source's index, the box's index in its list, its type and score, the
 * region x0 = X0, y0 = Y0, w = X1 - X0 + 1, h = Y1 - Y0 + 1, and net_input's letterbox of a w x h image into out_w x out_h (ffcnn.c:267-273)
 * as sw, sh, s1, s2.  Entries taken .. capacity-1: target = -1, s1 = s2 = 1, zero elsewhere.  No atomic decides an order: the table is the
 * same byte for byte on every run and however many sources there are.
 * Pixels.  Slot n < taken is net_input of the region: output pixel (x, y), x < sw, y < sh, is source pixel (x0 + x s1 / s2, y0 + y s1 / s2)
 * (integer division, 64-bit product).  The source pixel is the frame's B G R bytes, or for NV12 the integer formula above with nearest
 * chroma taken at the PICTURE's coordinates: odd origins are legal, no region is rounded.  FFGPU_CROP_F32: ((float)byte - mean) * norm, two
 * roundings, planes R G B.  FFGPU_CROP_U8: the three bytes.  Every other pixel of the slot, all of slots taken .. capacity-1 and, in the U8
 * form, every row's padding bytes are zero.  A call writes every byte of `capacity` slots and of the table and nothing before or behind them. */
#define FFGPU_CROP_F32 0   /* slot n: three planes R, G, B of out_h x out_w fp32 = frame n of ffgpu_exec_forward_dev's batch                    */
#define FFGPU_CROP_U8  1   /* slot n: out_h rows of ALIGN(3 out_w, 4) bytes B G R = frame n of ffgpu_exec_forward_bgr_dev's batch, or a picture */
typedef struct {
    int   out_w, out_h;             /* 1..4096: the second stage's geometry                                                       */
    int   form;                     /* FFGPU_CROP_F32 | FFGPU_CROP_U8                                                             */
    int   per_target;               /* 1..2^24: selected boxes per source at most                                                 */
    float min_score;
    int   nclasses;                 /* 0 with NULL classes, else 1..256                                                           */
    const unsigned char *classes;   /* HOST array of nclasses bytes (non-zero: the class is allowed), or NULL: every class        */
    int   margin_num, margin_den;   /* den 1..1024, num 0..4 den: the region is the box grown by num / den of its size each way   */
    float mean[3], norm[3];         /* FFGPU_CROP_F32 only: net_input's per-channel mean / norm (plane order R, G, B)             */
    int   reserved;                 /* 0                                                                                          */
} ffgpu_crop_spec;                  /* 72 bytes: out_w 0, out_h 4, form 8, per_target 12, min_score 16, nclasses 20, classes 24,  */
                                    /* margin_num 32, margin_den 36, mean 40, norm 52, reserved 64                                */
typedef struct {
    int   target, box, type;        /* the source's index, the box's index in its list, the box's class                           */
    float score;
    int   x0, y0, w, h;             /* the region in the source                                                                   */
    int   sw, sh, s1, s2;           /* its letterbox: it fills the top-left sw x sh of the slot, source pixel = (x s1 / s2, ...)    */
} ffgpu_crop;                       /* 48 bytes, behind the table's 16-byte header                                                */

/* pure host code: the bytes of a table of `capacity` entries, and of one slot (0 for arguments outside their ranges) */
size_t ffgpu_crop_table_bytes(int capacity);
size_t ffgpu_crop_slot_bytes(int out_w, int out_h, int form);

/* The operators, on device records and lists with no executor.  d_records, d_lists, list_stride and the HOST array list_first are the draw
 * operators' and so are the clamps of the counts: whatever the records hold, nothing is read outside the buffers the host has sized or outside
 * a source's w x h.  d_out: capacity x ffgpu_crop_slot_bytes bytes, 16-byte aligned.  sources, list_first, spec and spec->classes are HOST
 * memory and free again on return; the tables travel as kernel arguments, 64 sources per launch, and the count of boxes selected so far
 * travels in the table's header in stream order.  Enqueued on `stream` without synchronising.  Rejected before anything is launched, with the
 * source's index ("target k") in the message where there is one: NULL records, sources, spec, output or table, ntargets < 1, capacity < 1
 * (or above 2^24), a spec field outside its range, nclasses inconsistent with classes, reserved != 0, a bad list_stride, a negative list
 * start, an output or table that is not 16-byte aligned, ntargets x list_stride above 2^31 - 1, a descriptor the forward would reject other
 * than for a NULL address. */
int ffgpu_crop_boxes_bgr_dev (const void *d_records, const void *d_lists, int list_stride, const int *list_first, const ffgpu_bgr_frame  *sources,
                              int ntargets, const ffgpu_crop_spec *spec, void *d_out, void *d_table, int capacity, void *stream);
int ffgpu_crop_boxes_nv12_dev(const void *d_records, const void *d_lists, int list_stride, const int *list_first, const ffgpu_nv12_frame *sources,
                              int ntargets, const ffgpu_crop_spec *spec, void *d_out, void *d_table, int capacity, void *stream);

#define FFGPU_CROP_ENTRIES 0   /* entry n's full post-NMS list out of sources[n]; ntargets == batch                                      */
#define FFGPU_CROP_MERGED  1   /* picture g's merged list (last ffgpu_exec_merge_tiles) out of sources[g]; ntargets == its nimages        */
/* On an executor: a post-pass like ffgpu_exec_draw_*, enqueued on `stream` (NULL = the executor's own; it must be the stream of the forward
 * or merge it follows) without synchronising.  The captured graph, the records, the full lists, the ring and the host mirror are untouched;
 * the output and the table are the caller's.  Works on FFGPU_SPLIT2 executors.  Rejected like the operators, and: ntargets not as stated, a
 * `which` that is neither, FFGPU_CROP_MERGED when no merge has run, the wrong stream.  A rejected call leaves the executor usable. */
int ffgpu_exec_crop_bgr (ffgpu_exec *ex, int which, const ffgpu_bgr_frame  *sources, int ntargets, const ffgpu_crop_spec *spec,
                         void *d_out, void *d_table, int capacity, void *stream);
int ffgpu_exec_crop_nv12(ffgpu_exec *ex, int which, const ffgpu_nv12_frame *sources, int ntargets, const ffgpu_crop_spec *spec,
                         void *d_out, void *d_table, int capacity, void *stream);

/* Map back: d_records holds `capacity` records of a forward over the slots (boxes in slot pixels rescaled by the SLOT's own s1 / s2 = 1, i.e.
 * in the second net's pixels: run that forward with the default scale), d_lists (may be NULL) their full lists, list n at box n x list_stride.
 * For slot n < taken every box of record n -- its own box[0 .. count), count clamped to [0, FFGPU_MAX_DET], and its nfull list boxes, clamped to
 * [0, list_stride], when d_lists and d_out_lists are given -- becomes x * (float)s1 / (float)s2 + (float)x0, y likewise: fp32 multiply, then
 * divide, then add, not contracted (k_nms's rescale followed by the merge's translation).  type, score and the four counters are copied,
 * unused box slots of the record are zero; list boxes behind nfull are not written.  Slots taken .. capacity-1 give zero records (a net run on
 * a zero frame may emit boxes: they do not leak).  In place (d_out_records == d_records, d_out_lists == d_lists) is legal.  Rejected: a NULL
 * table or records, capacity < 1, a table that is not 16-byte aligned, a bad list_stride with d_lists given. */
int ffgpu_crops_to_source_dev(const void *d_table, int capacity, const void *d_records, const void *d_lists, int list_stride,
                              void *d_out_records, void *d_out_lists, void *stream);

/* ---- the detections tracked across a stream's frames on the device ---------------------------------------------------------------------------
 * Every step above treats a frame as if it were alone.  What follows associates the boxes of consecutive frames of one video stream -- "is this
 * the car of the previous frame?" -- where the records lie, in HBM: a greedy, class-aware IoU tracker with "last box, no motion model".  Its
 * result is a pure function of its inputs: the same bytes on every run, comparable byte for byte (tests/tracks/trackref.py restates it).
 *
 * Streams and order.  A call handles ntargets records.  streams[t] (a HOST int array) is the video stream of record t, 0 .. nstreams-1, or -1:
 * the entry is ignored.  The records of one stream are consecutive in time in ascending t; across calls, order on the HIP stream is time order.
 * Streams are independent of each other.
 * State, in the caller's device memory (16-byte aligned, ffgpu_track_state_bytes(nstreams, capacity) bytes): per stream a 16-byte header
 * { int issued, frames, live, reserved } and `capacity` entries ffgpu_track.  id == 0 is a free slot and a free slot is all zero; all-zero
 * memory is the valid empty state, so hipMemsetAsync (or ffgpu_track_reset_dev) initialises it.  Ids are ++issued, a 32-bit counter: after
 * 2^32 - 1 births of one stream it wraps (through 0 and the negative ids); this is not handled.
 *
 * One frame of one stream, in this order:
 *   1. Detections.  The record's list is walked in list order (d_lists, list_stride, list_first and the clamps of the draw operators).  A box is
 *      CONSIDERED when score >= min_score (a NaN score never is), until FFGPU_TRACK_DETS boxes are considered; further qualifying boxes are
 *      counted in `dropped`.
 *   2. IoU of track a (its last box) and considered detection j, with exactly the arithmetic of the merge with use_min == 0: area =
 *      (x2 - x1) * (y2 - y1); xa = a.x1 > j.x1 ? a.x1 : j.x1, ya likewise, xb = a.x2 < j.x2 ? a.x2 : j.x2, yb likewise; inter =
 *      (xb - xa) * (yb - ya) if xa < xb && ya < yb, else 0; iou = inter / (area_a + area_j - inter): fp32, not contracted, IEEE division.  A
 *      pair is ELIGIBLE when iou >= iou_thresh (NaN never is) and, with class_aware, the types are equal.
 *   3. Matching.  The eligible pairs are walked in the total order "iou descending (as fp32 values compare), then track slot ascending, then
 *      detection index ascending"; a pair whose track and detection are both still unmatched is a match.  No atomic and no arrival order
 *      decides anything.
 *   4. A matched track takes the detection's type, score and box; hits += 1, missed = 0, det = the box's index in its list.
 *   5. An unmatched track: missed += 1, det = -1; if missed > max_missed the slot is freed (zeroed).
 *   6. Births, after the frees, in ascending detection index: an unmatched considered detection with score >= birth_score takes the lowest free
 *      slot: id = ++issued, hits = 1, missed = 0, born = frames, det = its index.  With no free slot it is counted in `refused`.
 *   7. frames += 1 and live = the number of occupied slots -- also for a frame without boxes.
 *
 * Outputs per record t; every byte is written, for streams[t] == -1 as zero.  S = list_stride, or FFGPU_MAX_DET when d_lists is NULL.
 *   d_ids: row t of 8 + S ints: the header { considered, matched, born, refused, dropped, freed, live, frame } (frame: the stream's frame
 *     number of this record = `frames` before step 7), then ids[k] for box k of the list: 0 when the box was not considered or was neither
 *     matched nor born, else the id of its track when that track now has hits >= min_hits, else -id.  Entries behind the list are 0.
 *   d_out_records / d_out_lists (may be NULL; list t at box t x S): the TRACKED RECORD: the n considered boxes whose track now has hits >=
 *     min_hits, in list order, unchanged except that `type` is the track id.  count = min(n, FFGPU_MAX_DET), nfull = n, ncand and overflow
 *     bit 0 copied, bit 2 = n > FFGPU_MAX_DET; unused box slots of the record and of the list are zero.  The outputs must not overlap the inputs.
 * The tracked record is the composition point and needs no new code: the draw operators colour it per OBJECT (the palette entry is type mod
 * npalette, and type is the track id), the crop operators put the track id into ffgpu_crop.type, so a cascade can look once per object. */
#define FFGPU_TRACK_DETS 128   /* considered detections per frame at most; also the largest capacity */
typedef struct {
    int   capacity;                 /* 1..128: track slots per stream (as the state was sized)                                      */
    int   max_missed;               /* 0..2^20: a track survives this many consecutive frames without a match                       */
    int   min_hits;                 /* 1..2^20: a track is reported with its positive id from this many hits on                     */
    float iou_thresh;               /* finite, in [0, 1]                                                                            */
    float min_score;                /* finite, in [0, 1]: a detection is considered from this score on                              */
    float birth_score;              /* finite, in [0, 1]: an unmatched detection starts a track from this score on                  */
    int   class_aware;              /* 0 | 1: a pair needs equal types                                                              */
    int   reserved;                 /* 0                                                                                            */
} ffgpu_track_spec;                 /* 32 bytes: capacity 0, max_missed 4, min_hits 8, iou_thresh 12, min_score 16, birth_score 20, */
                                    /* class_aware 24, reserved 28                                                                  */
typedef struct {
    int   id, type;                 /* id 0: a free slot (all zero); type, score and the box: the last matched detection's          */
    float score, x1, y1, x2, y2;
    int   hits, missed;             /* matched frames in all; consecutive frames without a match                                    */
    int   born, det;                /* the stream's frame number of its birth; its box's index in the last frame's list, or -1      */
    int   reserved;                 /* 0                                                                                            */
} ffgpu_track;                      /* 48 bytes, behind each stream's 16-byte header { int issued, frames, live, reserved }         */

/* pure host code: the bytes of the state of nstreams (1..65536) streams of capacity (1..128) slots; 0 for arguments outside their ranges */
size_t ffgpu_track_state_bytes(int nstreams, int capacity);
/* zeroes the state of one stream, or of all with which_stream == -1, in stream order (a memset; no kernel) */
int ffgpu_track_reset_dev(void *d_state, int nstreams, int capacity, int which_stream, void *stream);

/* The operator, on device records and lists with no executor.  d_records, d_lists, list_stride and the HOST array list_first are the draw
 * operators'.  One workgroup per video stream walks that stream's records of the call serially, tracks and detections in LDS; streams,
 * list_first and spec are HOST memory and free again on return; the tables travel as kernel arguments, 128 records per launch, the launches of
 * one call in order on `stream`.  Enqueued without synchronising.  Rejected before anything is launched, with the entry's index in the message
 * where there is one: NULL records, streams, spec, state or ids, ntargets < 1, nstreams outside 1..65536, a stream index outside
 * -1..nstreams-1, a spec field outside its range or reserved != 0, a state that is not 16-byte aligned, a bad list_stride, a negative list
 * start, d_out_lists without d_out_records.  A rejected call leaves the state as it was. */
int ffgpu_track_boxes_dev(const void *d_records, const void *d_lists, int list_stride, const int *list_first, const int *streams, int ntargets,
                          const ffgpu_track_spec *spec, void *d_state, int nstreams, void *d_ids, void *d_out_records, void *d_out_lists, void *stream);

#define FFGPU_TRACK_ENTRIES 0   /* entry n's full post-NMS list is record n; ntargets == batch; S = ffgpu_exec_cand_capacity()                      */
#define FFGPU_TRACK_MERGED  1   /* picture g's merged list (last ffgpu_exec_merge_tiles) is record g; ntargets == its nimages; S =                */
                                /* ffgpu_exec_cand_capacity() x the most tiles any picture of that merge has                                     */
/* On an executor: a post-pass like ffgpu_exec_crop_*, enqueued on `stream` (NULL = the executor's own; it must be the stream of the forward or
 * merge it follows) without synchronising.  The captured graph, the records, the full lists, the ring and the host mirror are untouched; state,
 * ids and the tracked records are the caller's.  Works on FFGPU_SPLIT2 executors.  Rejected like the operator, and: ntargets not as stated, a
 * `which` that is neither, FFGPU_TRACK_MERGED when no merge has run, the wrong stream.  A rejected call leaves the state and the executor usable. */
int ffgpu_exec_track(ffgpu_exec *ex, int which, const int *streams, int ntargets, const ffgpu_track_spec *spec, void *d_state, int nstreams,
                     void *d_ids, void *d_out_records, void *d_out_lists, void *stream);

/* ---- the crops classified on the device: features, top-k labels, relabelling ---------------------------------------------------------------------
 * The crops above fill a batch "for a second stage".  Where that stage is a detector its records come back with ffgpu_crops_to_source_dev.  Where it is
 * a classifier or an embedding net -- a cfg WITHOUT a [yolo] layer -- its product is the tensor its last layer leaves.  What follows turns that tensor
 * into one fp32 row per frame, a row into its k best labels, and each crop's best label into the class of the first stage's box the crop was cut from,
 * where the data lie, in HBM; nothing crosses the bus and nothing synchronises.  No atomic is used anywhere: every result is a pure function of its
 * inputs, the same bytes on every run (tests/features/featref.py restates the contract in numpy).
 *
 * Headless executors.  ffgpu_exec_create accepts a cfg without a [yolo] layer, with every flag combination, and every ffgpu_exec_forward_* form runs it;
 * its records come out with count = ncand = nfull = overflow = 0 and ffgpu_exec_cand_capacity() is 1.
 *
 * Features.  Input: a tensor in the device layout "CNHW": plane (c, n) at ((c*N + n)*H*W), fp32.  Output: N rows of D fp32, frame-major: row n starts at
 * d_out + n * out_stride (in floats), out_stride >= D, in the caller's memory; every element of every row is written, nothing between or behind the rows.
 * `pool` selects the row:
 *   FFGPU_FEAT_FLAT: D = C*H*W.  The frame's tensor in the reference's CHW order, i.e. what ffgpu_exec_read_layer returns, bit for bit, NaN payloads
 *     and -0 included.
 *   FFGPU_FEAT_MEAN: D = C.  The fp32 sum of the plane divided by (float)(H*W) with IEEE division.  The summation order is the implementation's; it is
 *     a FIXED order: no atomic, independent of n and N (and of the tensor's alignment): a frame's row is the same bytes wherever the frame stands.
 *   FFGPU_FEAT_MAX: D = C.  The plane's maximum.  Any NaN in the plane gives the quiet NaN 0x7fc00000; zeros compare as -0 < +0, so the result is
 *     order-free and exact.
 * `post` is applied to the row after pooling:
 *   FFGPU_POST_NONE: the pooled row as it is.
 *   FFGPU_POST_SOFTMAX: m = max_i x_i; e_i = expf(x_i - m), the accurate expf, not the fast intrinsic; out_i = e_i / sum(e).  A row with any NaN or
 *     +Inf, or with only -Inf, is all NaN (0x7fc00000).  A -Inf element in any other row gives 0.
 *   FFGPU_POST_L2: r = sqrtf(sum(x_i * x_i)); out_i = x_i / r.  With r == 0 the row is all zeros.  Non-finite inputs give what IEEE arithmetic of that
 *     formula gives.
 * At most two launches per call (one without a `post`). */
#define FFGPU_FEAT_FLAT    0
#define FFGPU_FEAT_MEAN    1
#define FFGPU_FEAT_MAX     2
#define FFGPU_POST_NONE    0
#define FFGPU_POST_SOFTMAX 1
#define FFGPU_POST_L2      2
typedef struct {
    int layer;                      /* -1: the tensor the net's last layer leaves; >= 0: that layer's output (FFGPU_KEEP_ALL executors only)   */
    int pool, post;                 /* FFGPU_FEAT_*, FFGPU_POST_*                                                                              */
    int reserved;                   /* 0                                                                                                       */
} ffgpu_feature_spec;               /* 16 bytes: layer 0, pool 4, post 8, reserved 12                                                          */

/* pure host code: D for a tensor of c x h x w per frame; 0 for sizes below 1, a pool outside its range, a plane (h * w) or a row (D) above 2^24 */
int ffgpu_feature_dim(int c, int h, int w, int pool);
/* pure host code: D of `spec` on this executor, or -1 with a message where ffgpu_exec_features would reject the spec */
int ffgpu_exec_feature_dim(const ffgpu_exec *ex, const ffgpu_feature_spec *spec);

/* The operator, on any device tensor with no executor.  Enqueued on `stream` without synchronising.  Rejected before anything is launched: NULL
 * pointers, sizes below 1, D (or a plane) above 2^24, out_stride < D, an enum outside its range, an input or output that is not 4-byte aligned. */
int ffgpu_features_dev(const float *d_in, int n, int c, int h, int w, int pool, int post, float *d_out, long out_stride, void *stream);

/* On an executor: a post-pass like ffgpu_exec_crop_*, enqueued on `stream` (NULL = the executor's own; it must be the stream of the forward it follows)
 * without synchronising.  The captured graph, the records, the full lists, the ring and the host mirror are untouched; the rows are the caller's (N =
 * ffgpu_exec_batch(ex)).  layer == -1 means the tensor the net's last layer leaves, aliases resolved: a trailing dropout or one-source route gives its
 * source's tensor; it is legal on every plan (the arena reuses a range only for a tensor first used behind the range's last use, and none is; nothing overwrites it after the forward).  layer >= 0 is
 * legal only on FFGPU_KEEP_ALL executors, for a materialised layer, exactly as ffgpu_exec_read_layer decides.  A [yolo] layer (it has no tensor), a layer
 * fused away and an alias of the net input are rejected with a message.  Works on FFGPU_SPLIT2 executors: each part writes its frames' rows, in the same
 * launches.  Rejected like the operator, and: a NULL spec, reserved != 0, the wrong stream.  A rejected call leaves the executor usable. */
int ffgpu_exec_features(ffgpu_exec *ex, const ffgpu_feature_spec *spec, float *d_out, long out_stride, void *stream);

/* Top-k.  Input: n rows of d fp32, row r at d_in + r * in_stride (in_stride >= d).  Output: row r of d_out holds k entries ffgpu_label, 8 bytes each
 * (row r at byte 8 k r): the row's elements in this total order: value descending, as fp32 values compare; then index ascending -- so +0 and -0 tie and
 * the lower index wins; NaN is never selected.  Missing entries are { -1, 0.0f }: d < k, or too few elements that are no NaN.  The result is exact given
 * the row.  One launch per call.  Rejected before anything is launched: NULL pointers, n < 1, d outside 1..2^24, in_stride < d, k outside
 * 1..FFGPU_TOPK_MAX, an input or output that is not 4-byte aligned. */
#define FFGPU_TOPK_MAX 16
typedef struct { int index; float value; } ffgpu_label;      /* 8 bytes */
int ffgpu_topk_dev(const float *d_in, int n, int d, long in_stride, int k, void *d_out, void *stream);

/* Relabel.  Inputs: a crop table exactly as ffgpu_crop_boxes_* leaves it (d_table, capacity); its slots' top-k rows (d_labels: `capacity` rows of k
 * ffgpu_label; only entry 0 of each row is used, k is passed for the row pitch); the first stage's records and its lists if any: d_records, d_lists,
 * list_stride, the HOST array list_first and the clamps of the counts are the draw operators'.
 * Outputs, laid out like the tracked record's: d_out_records[t], and list t at box t x S of d_out_lists (may be NULL); S = list_stride, or FFGPU_MAX_DET
 * with NULL lists (the list is then the record's own box[0 .. count)).  They are copies of record t and of its list: counters and boxes unchanged, unused
 * slots zero.  For every table entry n < taken whose label has index >= 0 and value >= min_value (a NaN value never), box entry.box of target
 * entry.target gets type = type_base + index, and with FFGPU_RELABEL_LABEL_SCORE also score = value.  The patch lands in the list, and in the record's
 * box[] where entry.box < count.  Boxes no entry refers to, and boxes of rejected labels, stay as they were; an entry whose target is outside
 * 0 .. ntargets-1 or whose box lies behind its list is ignored.  Every output byte is written.  The outputs must not overlap the inputs.  A table entry
 * names one box at most once, so no order decides anything.  One launch per 256 targets.  The relabelled record is a composition point like the tracked
 * record: ffgpu_draw_*, ffgpu_crop_* and ffgpu_track_* consume it unchanged. */
#define FFGPU_RELABEL_KEEP_SCORE  0
#define FFGPU_RELABEL_LABEL_SCORE 1
typedef struct {
    float min_value;                /* a label is applied from this value on                                                                   */
    int   type_base;                /* the new type is type_base + index                                                                       */
    int   score_mode;               /* FFGPU_RELABEL_*                                                                                         */
    int   reserved;                 /* 0                                                                                                       */
} ffgpu_relabel_spec;               /* 16 bytes: min_value 0, type_base 4, score_mode 8, reserved 12                                           */

/* The operator, on device records and lists with no executor.  list_first and spec are HOST memory and free again on return.  Enqueued on `stream`
 * without synchronising.  Rejected before anything is launched, with the target's index in the message where there is one: NULL table, labels, records,
 * spec or output records, capacity < 1, k outside 1..FFGPU_TOPK_MAX, ntargets < 1, a score_mode outside its range, reserved != 0, a table that is not
 * 16-byte aligned, labels or outputs that are not 4-byte aligned, a bad list_stride, a negative list start, outputs that are the inputs. */
int ffgpu_crops_relabel_dev(const void *d_table, int capacity, const void *d_labels, int k, const void *d_records, const void *d_lists, int list_stride,
                            const int *list_first, int ntargets, const ffgpu_relabel_spec *spec, void *d_out_records, void *d_out_lists, void *stream);

#define FFGPU_RELABEL_ENTRIES 0   /* entry n's record and full post-NMS list; ntargets == batch; S = ffgpu_exec_cand_capacity()                        */
#define FFGPU_RELABEL_MERGED  1   /* picture g's merged record and list (last ffgpu_exec_merge_tiles); ntargets == its nimages; S as FFGPU_TRACK_MERGED */
/* On the FIRST stage's executor: a post-pass like ffgpu_exec_track, enqueued on `stream` (NULL = the executor's own; it must be the stream of the forward
 * or merge it follows) without synchronising.  The captured graph, the records, the full lists, the ring and the host mirror are untouched; table, labels
 * and the relabelled records are the caller's.  Works on FFGPU_SPLIT2 executors.  Rejected like the operator, and: ntargets not as stated, a `which` that
 * is neither, FFGPU_RELABEL_MERGED when no merge has run, the wrong stream.  A rejected call leaves the executor usable. */
int ffgpu_exec_relabel(ffgpu_exec *ex, int which, const void *d_table, int capacity, const void *d_labels, int k, int ntargets,
                       const ffgpu_relabel_spec *spec, void *d_out_records, void *d_out_lists, void *stream);

/* ---- re-identification on the device: embeddings matched against a gallery, new ones enrolled -----------------------------------------------------
 * Where the second stage is an embedding net its rows (ffgpu_exec_features, usually FFGPU_FEAT_MEAN + FFGPU_POST_L2) mean something only next to other
 * rows: "which known person, vehicle or product is this?".  What follows compares query rows with a gallery of rows that lives in HBM, leaves the k best
 * gallery rows of every query as rows of ffgpu_label -- what ffgpu_crops_relabel_dev / ffgpu_exec_relabel consume, so the identity becomes the box's
 * type and draw, crop and track take it from there -- and appends the queries nobody recognised to the gallery, all where the data lie and with no
 * synchronisation.  There is no executor form: the operators work on caller-owned rows, as ffgpu_topk_dev does.  No atomic is used anywhere and nothing
 * depends on an arrival order: the same bytes on every run (tests/gallery/matchref.py restates the contract in numpy).
 *
 * The gallery is a HOST struct of device pointers, free again on return.  `count` is read ON THE DEVICE when the kernels run: an enrolment earlier on
 * the same stream grows the gallery for the match behind it with no host involvement.  A count outside 0 .. capacity is clamped. */
typedef struct {
    float *d_rows;                  /* capacity rows of d fp32, row g at d_rows + g * row_stride (floats), row_stride >= d                      */
    int   *d_ids;                   /* may be NULL: capacity ints; the label's index is d_ids[g] (g itself with NULL); d_ids[g] < 0: row g is disabled */
    int   *d_head;                  /* may be NULL: 16 bytes on the device { int count, issued, dropped, reserved }; rows g >= count are not there.
                                       NULL: count = capacity.  All-zero = the valid empty gallery (hipMemsetAsync initialises it)               */
    long   row_stride;
    int    capacity;                /* 1 .. 2^20                                                                                               */
    int    d;                       /* 1 .. 4096                                                                                               */
} ffgpu_gallery;                    /* 40 bytes: d_rows 0, d_ids 8, d_head 16, row_stride 24, capacity 32, d 36                                */

/* Match.  Queries: nq rows of g->d fp32, row q at d_q + q * q_stride (q_stride >= d).
 *  1. sim(q, g) is the dot product of query row q and gallery row g, in fp32.  The summation order is the implementation's; it is a FIXED order,
 *     independent of q, nq, g, capacity, count, the strides and every alignment: a pair of rows gives the same bits wherever it stands.
 *  2. A row behind count, or a disabled row, has sim = 0x7fc00000.
 *  3. Row q of d_out_labels holds k entries ffgpu_label (row q at byte 8 k q): the gallery rows in this total order: sim descending, as fp32 values
 *     compare; then gallery row g ascending -- ffgpu_topk_dev's order; NaN is never selected.  Missing entries are { -1, 0.0f }.  index is d_ids[g],
 *     or g when d_ids is NULL -- applied after the selection, so rows of one identity each take an entry; value is sim(q, g).
 *  4. d_sim may be NULL.  Otherwise element (q, g) for every g < capacity is written at d_sim + q * sim_stride + g, sim_stride >= capacity, and
 *     nothing else is written.  The labels are the same bytes with and without d_sim.
 *  5. Every byte of d_out_labels is written.
 *  6. nq is 1..4096, k is 1..FFGPU_TOPK_MAX.  Pointers need only 4-byte alignment (d_head: 16); wider loads are used only where the address permits,
 *     with the same bits either way.
 *  7. d_work is the caller's scratch of at least ffgpu_match_workspace_bytes(nq, capacity, k) bytes, free again when the call's work has run.
 * No synchronisation; everything is enqueued on `stream`.  At most two launches per call.  Rejected before anything is launched, each with its own
 * message: a NULL query, gallery, d_rows, labels or workspace; nq, k, capacity or d outside their ranges; q_stride or row_stride < d; sim_stride <
 * capacity; work_bytes below ffgpu_match_workspace_bytes; a pointer that is not 4-byte aligned; a d_head that is not 16-byte aligned.  A rejected call
 * launches nothing and leaves everything usable. */
size_t ffgpu_match_workspace_bytes(int nq, int capacity, int k);   /* pure host code; 0 for arguments outside their ranges */
int ffgpu_match_dev(const float *d_q, int nq, long q_stride, const ffgpu_gallery *g, int k, void *d_out_labels, float *d_sim, long sim_stride,
                    void *d_work, size_t work_bytes, void *stream);

/* Enrol: open-set re-identification with no host round trip -- whoever was not recognised becomes known.  d_ids and d_head are required.  d_labels:
 * nq rows of k ffgpu_label as ffgpu_match_dev leaves them; only entry 0 of each row is used, k is passed for the row pitch.  For the queries in
 * ascending r (every rank is a ballot's, no order of arrival decides anything):
 *   query r is matched when index >= 0 and value >= min_value (a NaN value never): out[r] = its label;
 *   otherwise, if every element of the row is finite and a slot is left, it is enrolled: the e-th enrolled row of the call takes slot count + e, its d
 *     floats are copied there bit for bit, d_ids[slot] = issued + e + 1, and out[r] = { that id, min_value } -- the same threshold passes it through
 *     ffgpu_crops_relabel_dev;
 *   otherwise out[r] = { -1, 0.0f } and `dropped` counts it.
 * Afterwards count and issued have grown by the number enrolled.  d_out_labels is nq entries of 8 bytes, every byte written; it must not overlap
 * d_labels.  Two unknown queries of one call are two identities, even if their rows are equal: a call does not match its queries against each other.
 * Ids are positive and never reused (issued < 2^31 is the caller's business).  No synchronisation; at most two launches per call: one workgroup that
 * decides, then a grid that copies.  Rejected like ffgpu_match_dev, and: a NULL d_ids, d_head or output, overlapping labels. */
int ffgpu_gallery_enroll_dev(const ffgpu_gallery *g, const float *d_q, int nq, long q_stride, const void *d_labels, int k, float min_value,
                             void *d_out_labels, void *stream);

/* ---- the detections redacted in the frames on the device ---------------------------------------------------------------------------------------
 * Privacy masking: faces, plates or people blanked or pixelated before a frame is encoded, stored or shown -- or everything BUT them.  What follows
 * replaces the pixels of the selected boxes' regions in u8 BGR and NV12 frames where they lie, in HBM, by a solid colour or a mosaic.  The result is
 * a pure function of the frame's original bytes, the list and the spec: the same bytes on every run (tests/redact/redactref.py restates it in numpy).
 *
 * Covered set S of a target.  A box QUALIFIES by the crop contract's rule: score >= min_score (a NaN score never does) and its class is allowed:
 * every type with classes == NULL, else 0 <= type < nclasses and classes[type] != 0.  Its region is the crop contract's [X0..X1] x [Y0..Y1]: the
 * integer corners (a, b, c, d) of the draw contract (toward zero, saturating, NaN -> 0), grown in 64-bit integers by mx = (c - a + 1) num / den and
 * my = (d - b + 1) num / den, clipped to the target's w x h.  A qualifying box with a > c, b > d, X0 > X1 or Y0 > Y1 contributes nothing.  U is the
 * union of the qualifying boxes' regions; S = U, or with FFGPU_REDACT_OUTSIDE the target's w x h minus U (a list with no qualifying box then redacts
 * the whole target).  Overlapping boxes and the order of the list do not matter.
 * FFGPU_REDACT_FILL.  BGR targets: every pixel of S becomes color[0..2].  NV12 targets (`matrix` is ignored, nothing is converted): Y[y][x] =
 * color[0] for the pixels of S, and chroma sample (i, j) becomes (color[1], color[2]) when ANY of its up to four luma pixels (2i..2i+1, 2j..2j+1)
 * inside w x h is in S -- the draw contract's view of a sample; it errs toward redacting.
 * FFGPU_REDACT_MOSAIC, cell side s.  The cell grid is anchored at the TARGET's pixel (0, 0), not at the boxes: the pattern does not crawl as a box
 * moves from frame to frame.  Cell (i, j) is x in [i s, min((i + 1) s, w) - 1], y in [j s, min((j + 1) s, h) - 1].  For each channel of a cell
 * m = (sum + n / 2) / n in integers, the sum taken over ALL n pixels of the clipped cell in the frame's ORIGINAL bytes, in S or not; every pixel of the
 * cell that is in S becomes m.  A cell with no pixel in S is neither changed nor read.  NV12: luma is one channel of such cells; chroma cell (i, j)
 * has side s / 2 in the ((w + 1) / 2) x ((h + 1) / 2) plane, U and V averaged separately over the clipped chroma cell with the same rounding, written
 * to the samples the FILL rule covers.  s is even there, so the luma pixels of a sample lie in one luma cell.
 * Untouched bytes.  Every byte outside S -- row padding, uncovered pixels and chroma samples, the memory before and behind the target -- stays as it
 * was.  Nothing depends on the order in which the device executes anything: each byte of a target is read and written by exactly one workgroup, and
 * a barrier stands between that workgroup's loads of a cell and its first store to it.  No atomic is used.
 * Ordering.  Redact, then draw: the outlines come out on top (the other way round the outlines are redacted with the rest).  A tile descriptor as a
 * target anchors the grid at the TILE; for tiled pictures use FFGPU_REDACT_MERGED on the whole picture.
 * Targets: as the draw contract takes them (a NULL pixel address = "skip this target", the const pointers are WRITTEN THROUGH, targets of one call
 * must not overlap in memory). */
#define FFGPU_REDACT_FILL    0
#define FFGPU_REDACT_MOSAIC  1
#define FFGPU_REDACT_OUTSIDE 1      /* flags bit 0: redact everything EXCEPT the regions */
typedef struct {
    int   mode;                     /* FFGPU_REDACT_FILL | FFGPU_REDACT_MOSAIC                                                    */
    int   cell;                     /* MOSAIC: 2..64, even for NV12 targets; FILL: 0                                              */
    int   flags;                    /* 0 | FFGPU_REDACT_OUTSIDE; any other bit is rejected                                        */
    int   nclasses;                 /* 0 with NULL classes, else 1..256                                                           */
    const unsigned char *classes;   /* HOST array, as ffgpu_crop_spec                                                             */
    float min_score;
    int   margin_num, margin_den;   /* as ffgpu_crop_spec: den 1..1024, num 0..4 den                                              */
    unsigned char color[4];         /* FILL: B G R 0 / Y U V 0                                                                    */
} ffgpu_redact_spec;                /* 40 bytes: mode 0, cell 4, flags 8, nclasses 12, classes 16, min_score 24, margin_num 28,   */
                                    /* margin_den 32, color 36                                                                    */

/* The operators, on device records and lists with no executor.  d_records, d_lists, list_stride, the HOST array list_first, the clamps of the counts,
 * ntargets >= 1 and the 64 targets per launch (one by-value kernel argument) are the draw operators'; target t is redacted by record t.  targets,
 * list_first, spec and spec->classes are HOST memory and free again on return.  Enqueued on `stream` without synchronising.  Rejected before anything
 * is launched, with the target's index in the message where there is one: NULL records, targets or spec, an unknown mode, unknown flag bits, a cell
 * outside its range (a non-zero cell with FILL, an odd cell on NV12 targets), nclasses inconsistent with classes, a margin outside its range,
 * everything the draw operators reject, and a target of more than 2^23 blocks (s (64 / s) pixels square; FILL: 64). */
int ffgpu_redact_boxes_bgr_dev (const void *d_records, const void *d_lists, int list_stride, const int *list_first,
                                const ffgpu_bgr_frame  *targets, int ntargets, const ffgpu_redact_spec *spec, void *stream);
int ffgpu_redact_boxes_nv12_dev(const void *d_records, const void *d_lists, int list_stride, const int *list_first,
                                const ffgpu_nv12_frame *targets, int ntargets, const ffgpu_redact_spec *spec, void *stream);

#define FFGPU_REDACT_ENTRIES 0   /* entry n's full post-NMS list in targets[n]; ntargets == batch                                        */
#define FFGPU_REDACT_MERGED  1   /* picture g's merged list (last ffgpu_exec_merge_tiles) in targets[g]; ntargets == its nimages          */
/* On an executor: a post-pass like ffgpu_exec_draw_*, enqueued on `stream` (NULL = the executor's own; it must be the stream of the forward or merge
 * it follows) without synchronising.  The captured graph, the records, the full lists, the ring and the host mirror are untouched.  A tracked or
 * relabelled record redacts by object or identity through the operators above: "who" is the record's `type`.  Works on FFGPU_SPLIT2 executors.
 * Rejected like the operators, and: ntargets not as stated, a `which` that is neither, FFGPU_REDACT_MERGED when no merge has run, the wrong stream.
 * A rejected call leaves the executor usable. */
int ffgpu_exec_redact_bgr (ffgpu_exec *ex, int which, const ffgpu_bgr_frame  *targets, int ntargets, const ffgpu_redact_spec *spec, void *stream);
int ffgpu_exec_redact_nv12(ffgpu_exec *ex, int which, const ffgpu_nv12_frame *targets, int ntargets, const ffgpu_redact_spec *spec, void *stream);

/* ---- the detections blurred in the frames on the device ----------------------------------------------------------------------------------------
 * The third form of privacy masking, and the one asked for first: the selected boxes' regions (or everything BUT them) box-blurred in u8 BGR and
 * NV12 frames where they lie.  A blur window reaches into pixels that a neighbour rewrites, so it is not done on one surface: the caller supplies a
 * SCRATCH surface per target, and a pass is two launches -- the first reads the target everywhere and writes the blurred values of the covered set
 * into the scratch, the second copies them back into the target; stream order between the two is the barrier.  The result is a pure function of
 * the frame's bytes, the list and the spec: the same bytes on every run (tests/blur/blurref.py restates it in numpy).
 *
 * Covered set S of a target: the redact contract's, word for word (qualifying boxes, regions, union, FFGPU_BLUR_OUTSIDE = the target's w x h minus
 * the union; a list with no qualifying box then blurs the whole target).  S is computed once per call from the list: every pass covers the same set.
 * One pass, BGR.  Let O be the target's bytes before the pass and r the radius.  For every pixel (x, y) of S and every channel, the window is
 * W = [max(x - r, 0) .. min(x + r, w - 1)] x [max(y - r, 0) .. min(y + r, h - 1)]: it is clipped to the target's w x h, not padded.  With n = |W|
 * the new byte is (sum of O over W + n / 2) / n in integers.  The window takes in pixels outside S: blur mixes, it does not mask.  Every byte outside
 * S stays.
 * Passes.  passes = p applies the pass p times, each reading the whole target as the previous one left it (three passes of a box approximate a
 * Gaussian).
 * NV12 (`matrix` is ignored, nothing is converted).  Luma is one channel with radius r.  The chroma plane is ((w + 1) / 2) x ((h + 1) / 2) samples
 * with radius rc = (r + 1) / 2; U and V are averaged separately with the same rounding, the window clipped to the chroma plane.  The samples written
 * are exactly those the redact FILL rule covers: a sample is written when ANY of its luma pixels inside w x h is in S.  No evenness is required of r.
 * Scratch.  One descriptor per target, of the same type and the same w x h; its pitches are free; it is NULL exactly where the target is NULL.
 * Scratch surfaces must not overlap each other or any target of the call in memory (a surface here is the bytes from the first to the last of each
 * of its planes, row padding included); a host check rejects that with both indices in the message.  After the call the scratch bytes at the
 * positions of S (chroma: of the covered samples) hold the target's final values, and every other scratch byte is unchanged: the scratch is
 * comparable byte for byte too.
 * Untouched bytes.  Every byte outside S -- row padding, uncovered pixels and samples, the memory before and behind the surfaces -- stays as it was,
 * in the target and in the scratch.  Each byte has one owner per launch: a workgroup owns a 64 x 64 block of the launch's destination, anchored at
 * pixel (0, 0); nobody writes a launch's source.  No atomic is used; every load lies inside the source's w x h, every store inside the destination's.
 * Ordering.  Blur, then draw, outline and caption: the overlays lie on top.  A tile descriptor is a legal target, but tiles of one picture overlap:
 * for tiled pictures use FFGPU_BLUR_MERGED on the whole picture, as redaction does.
 * Targets: as the draw contract takes them (a NULL pixel address = "skip this target", the const pointers are WRITTEN THROUGH, targets of one call
 * must not overlap in memory). */
#define FFGPU_BLUR_OUTSIDE 1        /* flags bit 0: blur everything EXCEPT the regions */
typedef struct {
    int   radius;                   /* 1..31: the window is up to (2 radius + 1) pixels square                                    */
    int   passes;                   /* 1..3                                                                                       */
    int   flags;                    /* 0 | FFGPU_BLUR_OUTSIDE; any other bit is rejected                                          */
    int   nclasses;                 /* 0 with NULL classes, else 1..256                                                           */
    const unsigned char *classes;   /* HOST array, as ffgpu_redact_spec                                                           */
    float min_score;
    int   margin_num, margin_den;   /* as ffgpu_redact_spec: den 1..1024, num 0..4 den                                            */
    int   reserved;                 /* must be 0                                                                                  */
} ffgpu_blur_spec;                  /* 40 bytes: radius 0, passes 4, flags 8, nclasses 12, classes 16, min_score 24, margin_num   */
                                    /* 28, margin_den 32, reserved 36                                                             */

/* The operators, on device records and lists with no executor: d_records, d_lists, list_stride, the HOST array list_first, the clamps of the counts
 * and ntargets >= 1 are the redact operators'; target t is blurred by record t through scratch[t].  targets, scratch, list_first, spec and
 * spec->classes are HOST memory and free again on return.  Enqueued on `stream` without synchronising: 2 passes launches per group of targets -- 64
 * BGR targets or 48 NV12 targets travel as one by-value kernel argument (an NV12 target and its scratch are four planes).  Rejected before anything
 * is launched, with the target's index in the message where there is one: everything the redact operators reject (but there is no mode and no
 * cell), and: a radius outside 1..31, passes outside 1..3, unknown flag bits, a non-zero reserved, NULL scratch, a bad scratch descriptor, a scratch
 * whose w x h differs from its target's, a scratch NULL where the target is not or the reverse, the overlaps above, and a target of more than 2^23
 * blocks of 64 x 64 pixels. */
int ffgpu_blur_boxes_bgr_dev (const void *d_records, const void *d_lists, int list_stride, const int *list_first,
                              const ffgpu_bgr_frame  *targets, const ffgpu_bgr_frame  *scratch, int ntargets, const ffgpu_blur_spec *spec, void *stream);
int ffgpu_blur_boxes_nv12_dev(const void *d_records, const void *d_lists, int list_stride, const int *list_first,
                              const ffgpu_nv12_frame *targets, const ffgpu_nv12_frame *scratch, int ntargets, const ffgpu_blur_spec *spec, void *stream);

#define FFGPU_BLUR_ENTRIES 0     /* entry n's full post-NMS list in targets[n]; ntargets == batch                                        */
#define FFGPU_BLUR_MERGED  1     /* picture g's merged list (last ffgpu_exec_merge_tiles) in targets[g]; ntargets == its nimages          */
/* On an executor: a post-pass like ffgpu_exec_redact_*, enqueued on `stream` (NULL = the executor's own; it must be the stream of the forward or
 * merge it follows) without synchronising.  The captured graph, the records, the full lists, the ring and the host mirror are untouched.  Works on
 * FFGPU_SPLIT2 executors.  Rejected like the operators and like the redact forms: ntargets not as stated, a `which` that is neither,
 * FFGPU_BLUR_MERGED when no merge has run, the wrong stream.  A rejected call launches nothing and leaves the executor usable. */
int ffgpu_exec_blur_bgr (ffgpu_exec *ex, int which, const ffgpu_bgr_frame  *targets, const ffgpu_bgr_frame  *scratch, int ntargets,
                         const ffgpu_blur_spec *spec, void *stream);
int ffgpu_exec_blur_nv12(ffgpu_exec *ex, int which, const ffgpu_nv12_frame *targets, const ffgpu_nv12_frame *scratch, int ntargets,
                         const ffgpu_blur_spec *spec, void *stream);

/* ---- zones and lines: identified boxes counted, flagged and gated on the device ----------------------------------------------------------------
 * What a deployment asks of a tracked stream: how many are in this region now, who entered or left it, how many crossed this line and which way,
 * who has been standing here for 200 frames -- and "redact everybody outside the ticketed area", "crop only those who crossed".  What follows is a
 * stateful, per-stream geometry pass over any record laid out like the tracked one; its products are an event row, two flag words per box and a
 * GATED RECORD the draw, crop, redact and track operators take unchanged.  The result is a pure function of its inputs: the same bytes on every run
 * (tests/zones/zoneref.py restates it in numpy).
 *
 * Scene: device memory, one ffgpu_scene per video stream: d_scenes[s] for stream s.  Coordinates are the records' own picture pixels.  `classes` is a
 * bit per class 0..127 (class c: bit c % 32 of word c / 32); all four words zero: every class.  A box of KNOWN class c is ADMITTED by a mask when the
 * mask is all zero or 0 <= c < 128 and its bit is set; a box of UNKNOWN class only by an all-zero mask.  anchor 0: the box's centre, anything else:
 * its bottom centre.  The kernel is total over any bytes: nzones and nlines are clamped to 0..8, a zone with nverts outside 3..8 or with a NaN among
 * its nverts vertices contains nothing, NaN compares false everywhere.  ffgpu_scene_check says what is wrong with a scene before it is uploaded.
 *
 * Arithmetic: fp32, not contracted, no division.
 *   Anchor of a box: px = (x1 + x2) * 0.5f; py = anchor ? y2 : (y1 + y2) * 0.5f.
 *   INSIDE a zone, by the even-odd rule: for every edge i -> j = (i + 1) % nverts with (yi > py) != (yj > py):
 *     d = (xj - xi) * (py - yi) - (px - xi) * (yj - yi); the edge toggles the result when yj > yi ? d > 0 : d < 0.
 *   Side of P of the directed line A -> B: side(P) = ((bx - ax) * (Py - ay) - (by - ay) * (Px - ax)) > 0.
 *   An object with previous anchor P0 and current anchor P1 CROSSES the line A -> B when side(P0) != side(P1) with respect to A -> B and A and B
 *   lie on different sides of P0 -> P1 by the same formula; FORWARD when side(P1) is true, else BACKWARD.
 * On coordinates of an integer grid (or of eighths) every product is exact and a point on an edge shared by two zones is in exactly one of them.
 *
 * Identity (spec.identity): where an object's identity and class come from.  FFGPU_ZONES_NONE: no identity (geometry only), class = type.
 * FFGPU_ZONES_TYPE: identity = the box's type (a tracked or relabelled record), class unknown.  FFGPU_ZONES_IDS: identity = d_ids row t, entry 8 + k
 * for box k of the list (rows of 8 + S ints, exactly what ffgpu_track_boxes_dev writes, S this call's S), class = type.  An identity <= 0 is ANONYMOUS.
 *
 * State, in the caller's device memory (16-byte aligned, ffgpu_zones_state_bytes(nstreams, capacity) bytes; all-zero is the valid empty state, so
 * hipMemsetAsync or ffgpu_zones_reset_dev initialises it): per stream a 144-byte header { int frames, live, reserved[2]; unsigned total_entered[8],
 * total_left[8], total_fwd[8], total_back[8]; } and `capacity` slots ffgpu_zone_slot of 64 bytes.  id == 0 is a free slot and a free slot is all zero.
 * Only bits 0..7 of a slot's `inside` are read.  Frame numbers and counters are 32-bit and wrap; differences of frame numbers are taken modulo 2^32
 * and read as signed.
 *
 * One frame of one stream, in this order (streams, ntargets, time order and -1 entries: exactly as ffgpu_track_boxes_dev; frame = `frames` before 7):
 *   1. Considered boxes.  The record's list is walked in list order (d_lists, list_stride, list_first and the clamps of the draw operators).  A box is
 *      CONSIDERED when score >= min_score (a NaN score never is), until FFGPU_ZONES_DETS boxes are; further qualifying boxes are counted in `dropped`.
 *   2. Geometry.  Every considered box gets its anchor and its `inside` mask: bit z for each zone z < nzones whose class mask admits it and that
 *      contains the anchor.
 *   3. Owners.  A considered box whose identity is > 0 OWNS it, unless an earlier considered box of the frame has the same identity: then it is a
 *      DUPLICATE.  Anonymous, duplicate and (6.) refused boxes have their inside bits and count in the occupancy, but cause no event.
 *   4. Known owners: the identity is the id of a slot (of the lowest such slot).  entered = inside & ~slot.inside, left = slot.inside & ~inside;
 *      since[z] = frame for the entered zones; every line l < nlines whose class mask admits the box is tested with P0 = the slot's point and P1 = the
 *      anchor; the box is LOITERING in every zone z it is inside with dwell_frames > 0 and frame - since[z] >= dwell_frames.  The slot then takes the
 *      anchor and the mask, and last = frame.
 *   5. Frees.  An occupied slot no owner of this frame named, with frame - last > max_missed, is zeroed; every zone in its mask counts one `left`.
 *   6. Fresh owners (owners that are not known) take the lowest free slots in list order, after the frees: id = the identity, the anchor, the mask,
 *      last = frame, since[z] = frame for the zones of the mask and 0 for the others; entered = inside; no line is tested.  An owner that finds no
 *      free slot is REFUSED.
 *   7. The header's totals grow by the frame's entered, left (frees included), fwd and back counts per zone / line; live = the occupied slots;
 *      frames += 1 -- also for a frame without boxes.
 *
 * Outputs per record t; every byte is written, for streams[t] == -1 as zero.  S = list_stride, or FFGPU_MAX_DET when d_lists is NULL.
 *   d_events: row t of FFGPU_ZONES_ROW + 2 S ints: 16 ints { considered, known, fresh, refused, duplicate, anonymous, dropped, freed, live, frame,
 *     0 x 6 }; 8 groups { occupancy, entered, left, loitering }, one per zone (occupancy: the considered boxes inside); 8 groups { fwd, back }, one per
 *     line; then two words per list box k (at FFGPU_ZONES_ROW + 2 k), zero for a box that was not considered.
 *     Word 0: bit z: inside zone z; 8 + z: entered it this frame; 16 + z: left it this frame; 24 + z: loitering in it.
 *     Word 1: bit l: crossed line l forward; 8 + l: backward; 16 known, 17 fresh, 18 refused, 19 duplicate, 20 anonymous.
 *   d_out_records / d_out_lists (may be NULL; list t at box t x S): the GATED RECORD: the n considered boxes SELECTED by the gate, in list order and
 *     unchanged.  A box is selected when (((word0 & gate_zone) | (word1 & gate_line)) != 0) != (flags & FFGPU_ZONES_GATE_INVERT).  It is laid out by
 *     the tracked record's rules: count = min(n, FFGPU_MAX_DET), nfull = n, ncand and overflow bit 0 copied, bit 2 = n > FFGPU_MAX_DET; unused box
 *     slots of the record and of the list are zero.  The outputs must not overlap the inputs.
 * The gated record is the composition point and needs no new code: redact it (OUTSIDE off) to hide who is inside a zone, crop it to look once at who
 * crossed, draw it, track it. */
#define FFGPU_SCENE_ZONES 8
#define FFGPU_SCENE_LINES 8
#define FFGPU_ZONE_VERTS  8
#define FFGPU_ZONES_DETS  128  /* considered boxes per frame at most; also the largest capacity */
#define FFGPU_ZONES_ROW   64   /* ints of an event row in front of the boxes' words */
typedef struct {
    float x[FFGPU_ZONE_VERTS], y[FFGPU_ZONE_VERTS];   /* the polygon's vertices 0 .. nverts-1, either winding                             */
    int   nverts;                   /* 3..8                                                                                         */
    int   dwell_frames;             /* >= 0; 0: nobody loiters here                                                                 */
    unsigned classes[4];            /* a bit per class 0..127; all zero: every class                                                */
    int   reserved[2];              /* 0                                                                                            */
} ffgpu_zone;                       /* 96 bytes: x 0, y 32, nverts 64, dwell_frames 68, classes 72, reserved 88                     */
typedef struct {
    float ax, ay, bx, by;           /* the directed segment A -> B                                                                  */
    unsigned classes[4];
} ffgpu_line;                       /* 32 bytes: ax 0, ay 4, bx 8, by 12, classes 16                                                */
typedef struct {
    ffgpu_zone zone[FFGPU_SCENE_ZONES];
    ffgpu_line line[FFGPU_SCENE_LINES];
    int   nzones, nlines;           /* 0..8 each                                                                                    */
    int   anchor;                   /* 0: the box's centre; 1: its bottom centre                                                    */
    int   reserved;                 /* 0                                                                                            */
} ffgpu_scene;                      /* 1040 bytes: zone 0, line 768, nzones 1024, nlines 1028, anchor 1032, reserved 1036           */

#define FFGPU_ZONES_NONE 0          /* identity: none (every box anonymous); class = type                                           */
#define FFGPU_ZONES_TYPE 1          /* identity = the box's type; class unknown                                                     */
#define FFGPU_ZONES_IDS  2          /* identity = d_ids; class = type                                                               */
#define FFGPU_ZONES_GATE_INVERT 1   /* flags bit 0: the gated record holds the considered boxes the gate does NOT select            */
typedef struct {
    int   capacity;                 /* 1..128: slots per stream (as the state was sized)                                            */
    int   max_missed;               /* 0..2^20: an object survives this many consecutive frames without being seen                  */
    int   identity;                 /* FFGPU_ZONES_NONE | _TYPE | _IDS                                                              */
    int   flags;                    /* 0 | FFGPU_ZONES_GATE_INVERT; any other bit is rejected                                       */
    float min_score;                /* finite, in [0, 1]: a box is considered from this score on                                    */
    unsigned gate_zone, gate_line;  /* the gate's masks over word 0 and word 1 of a box                                             */
    int   reserved;                 /* 0                                                                                            */
} ffgpu_zones_spec;                 /* 32 bytes: capacity 0, max_missed 4, identity 8, flags 12, min_score 16, gate_zone 20,        */
                                    /* gate_line 24, reserved 28                                                                    */
typedef struct {
    int   id;                       /* 0: a free slot (all zero)                                                                    */
    float px, py;                   /* the object's anchor when it was last seen                                                    */
    int   inside;                   /* its zones then (bits 0..7)                                                                   */
    int   last;                     /* the stream's frame number when it was last seen                                              */
    int   reserved[3];              /* 0                                                                                            */
    int   since[FFGPU_SCENE_ZONES]; /* the frame number at which it entered zone z                                                  */
} ffgpu_zone_slot;                  /* 64 bytes, behind each stream's 144-byte header                                               */

/* pure host code: the bytes of the state of nstreams (1..65536) streams of capacity (1..128) slots; 0 for arguments outside their ranges */
size_t ffgpu_zones_state_bytes(int nstreams, int capacity);
/* pure host code: n scenes in HOST memory checked before their upload; 0, or -1 with the message (ffgpu_last_error) naming the scene and what is
 * wrong: nzones or nlines outside 0..8, a used zone's nverts outside 3..8, a non-finite coordinate of a used vertex or line, a used line with A
 * equal to B, a negative dwell_frames, an anchor that is neither 0 nor 1, a reserved field that is not 0. */
int ffgpu_scene_check(const ffgpu_scene *host_scenes, int n);
/* zeroes the state of one stream, or of all with which_stream == -1, in stream order (a memset; no kernel) */
int ffgpu_zones_reset_dev(void *d_state, int nstreams, int capacity, int which_stream, void *stream);

/* The operator, on device records and lists with no executor.  d_records, d_lists, list_stride and the HOST array list_first are the draw operators'.
 * One workgroup per video stream walks that stream's records of the call serially, scene and state in LDS; streams, list_first and spec are HOST memory
 * and free again on return; the tables travel as kernel arguments, 128 records per launch, the launches of one call in order on `stream`.  Enqueued
 * without synchronising.  Rejected before anything is launched, with the entry's index in the message where there is one: NULL records, streams, spec,
 * scenes, state or events, ntargets < 1, nstreams outside 1..65536, a stream index outside -1..nstreams-1, a spec field outside its range, unknown flag
 * bits or reserved != 0, a state that is not 16-byte aligned, a bad list_stride, a negative list start, d_out_lists without d_out_records, and d_ids:
 * it is required exactly when identity == FFGPU_ZONES_IDS (NULL then, or given otherwise, is rejected).  A rejected call leaves the state as it was. */
int ffgpu_zones_boxes_dev(const void *d_records, const void *d_lists, int list_stride, const int *list_first, const int *streams, int ntargets,
                          const ffgpu_zones_spec *spec, const void *d_scenes, void *d_state, int nstreams, const void *d_ids, void *d_events,
                          void *d_out_records, void *d_out_lists, void *stream);

#define FFGPU_ZONES_ENTRIES 0   /* entry n's full post-NMS list is record n; ntargets == batch; S as FFGPU_TRACK_ENTRIES                          */
#define FFGPU_ZONES_MERGED  1   /* picture g's merged list (last ffgpu_exec_merge_tiles) is record g; ntargets == its nimages; S as FFGPU_TRACK_MERGED */
/* On an executor: a post-pass like ffgpu_exec_track, enqueued on `stream` (NULL = the executor's own; it must be the stream of the forward or merge it
 * follows) without synchronising.  The captured graph, the records, the full lists, the ring and the host mirror are untouched; scenes, state, events and
 * the gated records are the caller's, and d_ids is what ffgpu_exec_track wrote for the same `which`.  Works on FFGPU_SPLIT2 executors.  Rejected like the
 * operator, and: ntargets not as stated, a `which` that is neither, FFGPU_ZONES_MERGED when no merge has run, the wrong stream.  A rejected call leaves
 * the state and the executor usable. */
int ffgpu_exec_zones(ffgpu_exec *ex, int which, const int *streams, int ntargets, const ffgpu_zones_spec *spec, const void *d_scenes, void *d_state,
                     int nstreams, const void *d_ids, void *d_events, void *d_out_records, void *d_out_lists, void *stream);

/* ---- captions: names, scores, ids and counters written into the frames on the device ----------------------------------------------------------
 * After the forward a box has a class (or a relabelled class or identity), a score, a track id and zone flags, and the outline of the draw operators
 * shows none of it.  What follows writes "person 93% #12" at the box where the frames and the records already lie: a TEXT PRIMITIVE that rasterises
 * text items lying in device memory into u8 BGR and NV12 frames, a COMPOSER that writes such items from any record (plain, merged, tracked, relabelled,
 * gated), and a composer for the zones' and lines' counters.  The reference program draws rectangles only: the contract is this text, to the bit
 * (tests/captions/textref.py restates it in numpy).  Outlines of the zones' polygons and lines are not part of it.
 *
 * Font: 256 glyphs of 8 x 8 pixels, 2 048 bytes.  Byte g * 8 + r is row r of glyph g, row 0 at the top; bit 7 - c of that byte is column c, column 0
 * at the left; a set bit is ink.  The operators take `d_font`, 2 048 bytes of DEVICE memory (any alignment); NULL selects the built-in font compiled
 * into the library: codes 32..126 are ASCII, every other code is one "unknown" glyph, a hollow box.  Every ASCII glyph keeps column 7 and row 7 empty, so
 * adjacent cells do not touch; space is empty and no other glyph is; the 95 ASCII glyphs are pairwise different.
 *
 * Text items: ffgpu_text_item, 64 bytes each, in device memory (4-byte aligned).  Target t draws items t * items_stride .. t * items_stride +
 * items_stride - 1; items_stride lies in 1..256; unused slots have len == 0; there is no count to read.
 * The pixel set of an item: with s = the clamped scale and n = the clamped len, the item's RECTANGLE is the set of pixels with 0 <= px - x < 8 s n
 * and 0 <= py - y < 8 s, computed as if in 64-bit integers.  A pixel of the rectangle is INK when glyph text[(px - x) / (8 s)] has the bit for column
 * ((px - x) / s) % 8, row (py - y) / s; otherwise it is PAPER.  The item WRITES its ink pixels (value fg) and, with FFGPU_TEXT_OPAQUE, its paper
 * pixels too (value bg).  A pixel outside 0 <= px < w, 0 <= py < h of the target is dropped.
 * A target's result is what drawing its items serially in slot order would leave: a later item overwrites an earlier one.  Only written pixels
 * change; every other byte -- row padding, unwritten pixels, the memory in front of and behind the surface -- stays as it was.  The result does not
 * depend on the order in which the device executes anything: the same bytes on every run.
 * BGR targets: a written pixel becomes the three bytes 0, 1, 2 of fg or bg.  NV12 targets (`matrix` ignored, nothing converted): a written pixel sets
 * Y[py][px] = byte 0; the chroma pair UV[py >> 1][px >> 1] takes its value from the LAST item in slot order that writes any of the sample's up to four
 * luma pixels inside the target: that item's fg (U, V) = bytes 1, 2 if at least one of the luma pixels the item writes in this sample is ink,
 * otherwise its bg (U, V).  Odd widths and heights are legal.
 * The kernel is total over any item bytes: nothing is read outside d_items and the font, nothing is written outside the targets' w x h. */
#define FFGPU_TEXT_MAX    44   /* characters of an item */
#define FFGPU_TEXT_ITEMS  256  /* items per target at most (items_stride) */
#define FFGPU_TEXT_OPAQUE 1    /* flags bit 0: the paper is drawn too */
typedef struct {
    int x, y;                  /* top-left pixel of the first cell, in target pixels; any value */
    unsigned char fg[4];       /* ink:   B G R 0 (BGR targets) / Y U V 0 (NV12 targets) */
    unsigned char bg[4];       /* paper: same byte order */
    unsigned char scale;       /* 1..4: each font pixel is scale x scale target pixels; 0 reads as 1, above 4 as 4 */
    unsigned char flags;       /* FFGPU_TEXT_OPAQUE; other bits ignored */
    unsigned char len;         /* characters used; above FFGPU_TEXT_MAX reads as FFGPU_TEXT_MAX; 0: the item draws nothing */
    unsigned char reserved;
    unsigned char text[FFGPU_TEXT_MAX];  /* glyph codes */
} ffgpu_text_item;             /* 64 bytes: x 0, y 4, fg 8, bg 12, scale 16, flags 17, len 18, text 20 */

/* pure host code: the built-in font's 2 048 bytes */
void ffgpu_font_builtin(unsigned char out[2048]);

/* The rasteriser.  The descriptors, their checks, "a NULL pixel address skips the target" and the no-overlap rule are the draw operators', word for
 * word; the tables travel as by-value kernel arguments, 64 targets per launch; enqueued on `stream` without synchronising.  targets is HOST memory
 * and free again on return.  Rejected before anything is launched, with the target's index in the message where there is one: NULL items or targets,
 * items that are not 4-byte aligned, ntargets < 1, items_stride outside 1..256, a descriptor the draw operators would reject. */
int ffgpu_draw_text_bgr_dev (const void *d_items, int items_stride, const void *d_font,
                             const ffgpu_bgr_frame  *targets, int ntargets, void *stream);
int ffgpu_draw_text_nv12_dev(const void *d_items, int items_stride, const void *d_font,
                             const ffgpu_nv12_frame *targets, int ntargets, void *stream);

/* Box captions.  Records, lists, list_stride, the HOST array list_first and their clamps are the draw operators'; d_ids is what ffgpu_track_boxes_dev
 * wrote (rows of 8 + S ints, S = list_stride, or FFGPU_MAX_DET when d_lists is NULL) and is required exactly when identity == FFGPU_ZONES_IDS.
 * For target t the list is walked in list order; a box is CONSIDERED when score >= min_score (a NaN score never is), until
 * min(FFGPU_CAPTION_DETS, items_stride) boxes are considered; further qualifying boxes get no caption.  The k-th considered box writes item k of the
 * target; every other item of the target's items_stride slots is written as 64 zero bytes: every byte of d_items for the call's targets is written.
 * The item: (a, b, c, d) are the draw contract's integer corners (toward zero, saturating, NaN -> 0).  x = a; y = b - 8 * scale when b >= 8 * scale,
 * else y = b: the tag sits on the box, and where there is no room above, inside its top.  fg = the spec's; bg = palette entry type mod npalette (the
 * non-negative remainder), or `color`: the colour the draw operator outlines that box with; byte 3 of both is written as 0.  scale = the spec's;
 * flags = FFGPU_TEXT_OPAQUE iff FFGPU_CAPTION_OPAQUE is set; reserved and the text bytes behind len are 0.
 * The text is the parts below that are present, in this order, joined by one space and cut to FFGPU_TEXT_MAX characters; no part: len = 0.
 *   Name, with FFGPU_CAPTION_NAME and identity != FFGPU_ZONES_TYPE (with _TYPE the class is unknown, as in zones).  With 0 <= type < nnames: the bytes
 *     of row `type` of d_names up to the first NUL, at most 16, verbatim as glyph codes; an empty row gives an empty part, which is dropped.
 *     Otherwise: `type` in decimal, with - for negatives.
 *   Score, with FFGPU_CAPTION_SCORE: p = (int)(score * 100.0f + 0.5f), in fp32, not contracted, converted as the corners are, then clamped to 0..999;
 *     written in decimal, followed by %.
 *   Id, with FFGPU_CAPTION_ID: v = the box's type under _TYPE; under _IDS entry 8 + k' of row t of d_ids, k' the box's index in its list; under _NONE
 *     0.  v > 0: # and v in decimal.  v < 0: #, -v in decimal (taken in 64 bits) and ?: a track that has not reached min_hits.  v == 0: absent.
 * One workgroup per target; spec (with its palette) and list_first are HOST memory and free again on return; the tables travel as kernel arguments,
 * 128 targets per launch.  Rejected before anything is launched: the draw operators' reasons, NULL spec or items, items that are not 4-byte aligned,
 * items_stride outside 1..256, a non-finite or out-of-range min_score, flags without a part or with unknown bits, identity outside 0..2, scale
 * outside 1..4, npalette inconsistent with palette, nnames < 0 or inconsistent with d_names, d_ids given or missing against the identity rule. */
#define FFGPU_CAPTION_DETS   128  /* captioned boxes per target at most */
#define FFGPU_CAPTION_NAME   1
#define FFGPU_CAPTION_SCORE  2
#define FFGPU_CAPTION_ID     4
#define FFGPU_CAPTION_OPAQUE 8
typedef struct {
    float min_score;               /* finite, in [0, 1] */
    int   flags;                   /* at least one of NAME | SCORE | ID; unknown bits rejected */
    int   identity;                /* FFGPU_ZONES_NONE | _TYPE | _IDS, with the zones contract's meaning */
    int   scale;                   /* 1..4 */
    unsigned char fg[4];           /* ink */
    unsigned char color[4];        /* paper when palette is NULL */
    const unsigned char *palette;  /* HOST, npalette x 4 bytes, or NULL: exactly ffgpu_draw_style's */
    int   npalette;                /* 0 with a NULL palette, else 1..256 */
    int   nnames;                  /* rows of d_names; 0 with NULL */
    const void *d_names;           /* DEVICE, nnames rows of 16 bytes (a NUL ends a shorter name), or NULL */
} ffgpu_caption_spec;              /* 48 bytes: min_score 0, flags 4, identity 8, scale 12, fg 16, color 20, palette 24, npalette 32, nnames 36, */
                                   /* d_names 40 */
int ffgpu_caption_boxes_dev(const void *d_records, const void *d_lists, int list_stride, const int *list_first, int ntargets,
                            const ffgpu_caption_spec *spec, const void *d_ids, void *d_items, int items_stride, void *stream);

#define FFGPU_CAPTION_ENTRIES 0   /* entry n's full post-NMS list captions targets[n]; ntargets == batch; S as FFGPU_TRACK_ENTRIES              */
#define FFGPU_CAPTION_MERGED  1   /* picture g's merged list (last ffgpu_exec_merge_tiles) captions targets[g]; ntargets == its nimages         */
/* On an executor: a compose plus a draw-text, two launches, enqueued on `stream` (NULL = the executor's own; it must be the stream of the forward or
 * merge it follows) without synchronising.  d_items is the caller's scratch of ntargets x items_stride x 64 bytes and also the product: a caller may
 * read it.  d_ids is what ffgpu_exec_track wrote for the same `which`.  The captured graph, the records, the full lists, the ring and the host mirror
 * are untouched.  Redact, then draw, then caption: the tags lie on top.  Works on FFGPU_SPLIT2 executors.  Rejected like the operators, and: ntargets
 * not as stated, a `which` that is neither, FFGPU_CAPTION_MERGED when no merge has run, the wrong stream.  A rejected call leaves the executor usable. */
int ffgpu_exec_caption_bgr (ffgpu_exec *ex, int which, const ffgpu_bgr_frame  *targets, int ntargets, const ffgpu_caption_spec *spec,
                            const void *d_ids, void *d_items, int items_stride, const void *d_font, void *stream);
int ffgpu_exec_caption_nv12(ffgpu_exec *ex, int which, const ffgpu_nv12_frame *targets, int ntargets, const ffgpu_caption_spec *spec,
                            const void *d_ids, void *d_items, int items_stride, const void *d_font, void *stream);

/* Zone and line counters as text items, from the events and the state of ffgpu_zones_boxes_dev; the caller draws them with ffgpu_draw_text_*_dev (no
 * executor form: scenes and state are the caller's).  items_stride lies in 16..256.  events_stride is the ints per event row, FFGPU_ZONES_ROW + 2 S of
 * the zones call that wrote it.  Stream s = streams[t]; -1 gives the target all-zero items.
 *   Item z (0..7) exists for z < nzones (clamped to 0..8 as the zones kernel clamps it) when the zone's nverts is in 3..8.  Its text is "Z<z> <occupancy>",
 *     occupancy = int 16 + 4 z of event row t, read as unsigned decimal.  It sits at ((int)x[0], (int)y[0]) of the zone, by the draw contract's conversion.
 *   Item 8 + l exists for l < nlines (clamped likewise).  Its text is "L<l> <total_fwd[l]>/<total_back[l]>", read from the 144-byte header of stream s of
 *     d_state (the streams lie 144 + 64 x capacity bytes apart).  It sits at ((int)ax, (int)ay).  THE VALUES ARE THE STATE'S WHEN THE KERNEL RUNS: with
 *     several records of one stream in one zones call, every target of that stream shows the final totals.
 *   fg, scale and OPAQUE come from the spec; bg = palette entry z or 8 + l (mod npalette), or `color`.  Every other slot is zero.  The spec's min_score,
 *   part flags, identity and names are ignored here.
 * streams and spec are HOST memory and free again on return; 512 targets per launch.  Rejected before anything is launched: NULL scenes, state,
 * events, streams, spec or items, scenes, state, events or items that are not 4-byte aligned, ntargets < 1, nstreams outside 1..65536, capacity
 * outside 1..128, events_stride below FFGPU_ZONES_ROW, items_stride outside 16..256, a stream outside -1..nstreams-1, scale outside 1..4, npalette
 * inconsistent with palette. */
int ffgpu_caption_scene_dev(const void *d_scenes, const void *d_state, int nstreams, int capacity, const void *d_events, int events_stride,
                            const int *streams, int ntargets, const ffgpu_caption_spec *spec, void *d_items, int items_stride, void *stream);

/* ---- outlines: the zones' polygons, the lines, their forward side and the tested anchors drawn into the frames on the device --------------------
 * The captions write "Z3 5" at a zone's first vertex and "L1 12/7" at a line's A; the polygon the five are inside, the line the twelve crossed, the
 * side that counts as forward and the point of a box that is tested are what follows: a SEGMENT PRIMITIVE that rasterises segment items lying in
 * device memory into u8 BGR and NV12 frames, and a SCENE COMPOSER that writes such items from the scenes, the event rows and the state of
 * ffgpu_zones_boxes_dev.  The reference program draws rectangles only: the contract is this text, to the bit (tests/outlines/lineref.py restates it
 * in numpy).
 *
 * Segment items: ffgpu_seg_item, 32 bytes each, in device memory (4-byte aligned).  Target t draws items t * items_stride .. t * items_stride +
 * items_stride - 1; items_stride lies in 1..FFGPU_SEG_ITEMS; there is no count to read.  An item with thickness 0, or with any coordinate outside
 * -FFGPU_SEG_LIMIT..FFGPU_SEG_LIMIT, draws nothing (every product below then fits 64 bits with room to spare).
 * The pixel set of an item, all in 64-bit integers: dx = x1 - x0, dy = y1 - y0; the item is X-MAJOR when |dx| >= |dy|, otherwise y-major, and for a
 * y-major item x and y exchange their roles in everything that follows.  S is the end point with the smaller major coordinate, E the other one (they have the same
 * major coordinate only when the segment is a single point: then S == E): the set does not depend on the direction the segment was given in.  D = E.x - S.x >= 0, g = E.y - S.y, T = the clamped thickness, lo = (T - 1) / 2, hi = T / 2, d = the clamped
 * dash.  Pixel (px, py) belongs to the item when, with m = px - S.x and r = py - S.y:
 *     0 <= m <= D,  and  d == 0 or ((m >> d) & 1) == 0,  and
 *     if D == 0:  -lo <= r <= hi;   otherwise, with e = 2 m g + D:  2 D (r - hi) <= e < 2 D (r + lo + 1).
 * That is the column S.y + floor((2 m g + D) / (2 D)) of major step m with its lo pixels before and hi pixels behind, the floor taken toward
 * -infinity: a DDA that rounds half up in the canonical direction, the thickness running along the minor axis.  A solid item contains both of its
 * end points.  A pixel outside 0 <= px < w, 0 <= py < h of the target is dropped.
 * A target's result is what drawing its items serially in slot order would leave: a later item overwrites an earlier one.  Only written pixels
 * change; every other byte -- row padding, unwritten pixels, the memory in front of and behind the surface -- stays as it was.  The result does not
 * depend on the order in which the device executes anything: the same bytes on every run.
 * BGR targets: a written pixel becomes the three bytes 0, 1, 2 of `color`.  NV12 targets (`matrix` ignored, nothing converted): a written pixel sets
 * Y[py][px] = byte 0; the chroma pair UV[py >> 1][px >> 1] takes bytes 1, 2 of the LAST item in slot order that writes any of the sample's up to
 * four luma pixels inside the target.  Odd widths and heights are legal.
 * The segment kernel is total over any item bytes: nothing is read outside d_items, nothing is written outside the targets' w x h. */
#define FFGPU_SEG_ITEMS  512      /* items per target at most (items_stride) */
#define FFGPU_SEG_LIMIT  1048576  /* 2^20: an item with a coordinate beyond +- this draws nothing */
typedef struct {
    int x0, y0, x1, y1;          /* 0, 4, 8, 12: the end points, target pixels, any value            */
    unsigned char color[4];      /* 16: B G R 0 (BGR targets) / Y U V 0 (NV12 targets)               */
    unsigned char thickness;     /* 20: 0: the item draws nothing; above 8 reads as 8                */
    unsigned char dash;          /* 21: 0: solid; above 6 reads as 6                                 */
    unsigned char flags;         /* 22: ignored                                                      */
    unsigned char reserved;      /* 23                                                               */
    int reserved2[2];            /* 24                                                               */
} ffgpu_seg_item;                /* 32 bytes: x0 0, y0 4, x1 8, y1 12, color 16, thickness 20, dash 21, flags 22, reserved 23, reserved2 24 */

/* The segment rasteriser.  The descriptors, their checks, "a NULL pixel address skips the target" and the no-overlap rule are the draw operators',
 * word for word; the tables travel as by-value kernel arguments, 64 targets per launch; enqueued on `stream` without synchronising.  targets is HOST
 * memory and free again on return.  Rejected before anything is launched, with the target's index in the message where there is one: NULL items or
 * targets, items that are not 4-byte aligned, ntargets < 1, items_stride outside 1..512, a descriptor the draw operators would reject. */
int ffgpu_draw_segments_bgr_dev (const void *d_items, int items_stride, const ffgpu_bgr_frame  *targets, int ntargets, void *stream);
int ffgpu_draw_segments_nv12_dev(const void *d_items, int items_stride, const ffgpu_nv12_frame *targets, int ntargets, void *stream);

/* The scene as segment items, from the scenes, the events and the state of ffgpu_zones_boxes_dev; the caller draws them with
 * ffgpu_draw_segments_*_dev (no executor form: scenes and state are the caller's).  Its shape is ffgpu_caption_scene_dev's: stream s = streams[t];
 * -1 gives the target all-zero items; events_stride is the ints per event row of the zones call that wrote it; the state's streams lie
 * 144 + 64 x capacity bytes apart.  items_stride lies in FFGPU_OUTLINE_FIXED..512.  Every byte of d_items for the call's targets is written, so the
 * buffer needs no clearing; it is also the product: a caller may add items of their own behind the fixed slots.  THE STATE'S VALUES ARE THE STATE'S
 * WHEN THE KERNEL RUNS: with several records of one stream in one zones call, every target of that stream shows the anchors of the last one.
 * Every coordinate is converted from float by the draw contract's rule (toward zero, saturating, NaN -> 0); anything computed from the converted
 * integers is computed in 64 bits and saturated to int, so a far-off vertex yields items the primitive drops.  Byte 3 of a colour, `flags` and the
 * reserved fields are written as 0.
 *   Slot 8 z + i, with FFGPU_OUTLINE_ZONES: zone z's edge from vertex i to vertex (i + 1) % nverts.  It exists for z < nzones (clamped to 0..8 as
 *     the zones kernel clamps it) and i < nverts, when the zone's nverts is in 3..8 and none of its used vertices is NaN (otherwise the zone contains
 *     nothing and draws nothing).  thickness = the spec's, dash 0; colour = palette entry z mod npalette, or `color`; with FFGPU_OUTLINE_ALARM the
 *     colour is `alarm` when the zone's loitering count, int 16 + 4 z + 3 of event row t, is not 0.
 *   Slot 64 + 2 l, with FFGPU_OUTLINE_LINES: line l's shaft A -> B, for l < nlines (clamped likewise).  thickness = the spec's, dash = line_dash;
 *     colour = palette entry (8 + l) mod npalette, or `color`.
 *   Slot 64 + 2 l + 1, with FFGPU_OUTLINE_TICKS: the forward tick of line l, from M = ((ax + bx) >> 1, (ay + by) >> 1) to
 *     M + (-(by - ay) / 8, (bx - ax) / 8), the shifts arithmetic and the divisions toward zero, on the converted integers.  Solid, thickness 1, the
 *     shaft's colour.  It points to the side on which the zones contract's side(P) is true: where a crossing ends that counts as FORWARD.
 *   Slots 80 + 2 k and 80 + 2 k + 1, with FFGPU_OUTLINE_MARKERS: slot q < capacity of the stream's state is SEEN when id != 0 and last == frames - 1
 *     modulo 2^32, frames the header's.  The k-th seen slot in slot order writes a cross centred on the converted (px, py) = (cx, cy):
 *     (cx - r, cy) -> (cx + r, cy) and (cx, cy - r) -> (cx, cy + r), r = marker; solid, thickness 1; colour = palette entry id mod npalette (the
 *     non-negative remainder), or `color`.  It is written while 80 + 2 k + 1 < items_stride; further seen slots get none.
 *   Every other slot is 32 zero bytes.
 * One workgroup per target; streams and spec (with its palette) are HOST memory and free again on return; 512 targets per launch.  Rejected before
 * anything is launched: ffgpu_caption_scene_dev's reasons, with items_stride outside 80..512 in place of its range, and a spec field outside the
 * ranges below.  Redact, then draw, then outline, then caption: the tags lie on top. */
#define FFGPU_OUTLINE_FIXED   80  /* the slots of the zones' edges (0..63) and of the lines' shafts and ticks (64..79) */
#define FFGPU_OUTLINE_ZONES   1
#define FFGPU_OUTLINE_LINES   2
#define FFGPU_OUTLINE_TICKS   4   /* needs FFGPU_OUTLINE_LINES */
#define FFGPU_OUTLINE_MARKERS 8
#define FFGPU_OUTLINE_ALARM   16  /* needs FFGPU_OUTLINE_ZONES */
typedef struct {
    int flags;                     /* at least one of ZONES | LINES | MARKERS; unknown bits rejected */
    int thickness;                 /* 1..8: zones and line shafts */
    int line_dash;                 /* 0..6: the line shafts' dash */
    int marker;                    /* 0..32: the anchor crosses' arm length; at least 1 with MARKERS */
    unsigned char color[4];        /* the colour when palette is NULL */
    unsigned char alarm[4];        /* the alarm colour */
    const unsigned char *palette;  /* HOST, npalette x 4 bytes, or NULL: exactly ffgpu_draw_style's */
    int npalette;                  /* 0 with a NULL palette, else 1..256 */
    int reserved;                  /* 0 */
} ffgpu_outline_spec;              /* 40 bytes: flags 0, thickness 4, line_dash 8, marker 12, color 16, alarm 20, palette 24, npalette 32, reserved 36 */
/* pure host code: 0, or -1 with the message in ffgpu_last_error */
int ffgpu_outline_spec_check(const ffgpu_outline_spec *spec);
int ffgpu_outline_scene_dev(const void *d_scenes, const void *d_state, int nstreams, int capacity, const void *d_events, int events_stride,
                            const int *streams, int ntargets, const ffgpu_outline_spec *spec, void *d_items, int items_stride, void *stream);

/* ---- track trails: where an identified object has been, kept per stream on the device and composed into segment items -------------------------
 * The zones state holds one anchor per slot, the last.  What follows keeps a HISTORY of anchors per identity and per video stream -- a ring of up to
 * FFGPU_TRAIL_POINTS points behind every slot -- and has two products: TRAIL ITEMS, ffgpu_seg_items the segment primitive above draws, and a MOTION
 * ROW per box (displacement and frame span over the kept history) from which speed and heading follow.  It is a stateful per-stream pass in the shape
 * of ffgpu_zones_boxes_dev, and a pure function of its inputs: the same bytes on every run (tests/trails/trailref.py restates it in numpy).
 *
 * State, in the caller's device memory (16-byte aligned, ffgpu_trails_state_bytes(nstreams, capacity) bytes; all-zero is the valid empty state, so
 * hipMemsetAsync or ffgpu_trails_reset_dev initialises it): per stream a 16-byte header { int frames, live, reserved[2]; } and `capacity` slots
 * ffgpu_trail_slot of 416 bytes.  id == 0 is a free slot and a free slot is all zero, all 416 bytes.  The LIVE POINTS of a slot are ring[(head + j) % 32]
 * for j = 0 .. n - 1, j = 0 the oldest and j = n - 1 the NEWEST; ring entries outside that window keep whatever they held.  Frame numbers are 32-bit
 * and wrap; differences of frame numbers are taken modulo 2^32 and read as signed.  The kernel is total over any state bytes: wherever a slot's n and
 * head are READ, n is clamped to 0..points and head is taken modulo 32 (the non-negative remainder); a known owner's slot gets the clamped values back.
 *
 * One frame of one stream, in this order (streams, ntargets, time order and -1 entries: exactly as ffgpu_zones_boxes_dev; frame = `frames` before 7):
 *   1. Considered boxes.  The record's list is walked in list order (d_lists, list_stride, list_first and the clamps of the draw operators).  A box is
 *      CONSIDERED when score >= min_score (a NaN score never is), until FFGPU_TRAILS_DETS boxes are; further qualifying boxes are counted in `dropped`.
 *   2. Anchor.  In fp32, not contracted, as the zones contract: px = (x1 + x2) * 0.5f; py = anchor ? y2 : (y1 + y2) * 0.5f.  Each coordinate is then
 *      converted to int by the draw contract's rule (toward zero, saturating, NaN -> 0): A = (A.x, A.y).  Everything behind this point is integer.
 *   3. Owners.  The identity is the box's type (FFGPU_ZONES_TYPE) or d_ids row t, entry 8 + k for box k of the list (FFGPU_ZONES_IDS; rows of 8 + S
 *      ints).  An identity <= 0 is ANONYMOUS.  A considered box whose identity is > 0 OWNS it, unless an earlier considered box of the frame has the
 *      same identity: then it is a DUPLICATE.
 *   4. Known owners: the identity is the id of a slot (of the lowest such slot).  With N the slot's newest live point, the anchor is APPENDED when
 *      max(|A.x - N.x|, |A.y - N.y|) >= min_move, in 64-bit integers (min_move 0: always), and also when the slot has no live point (n == 0).
 *      Append with n == points: head = (head + 1) % 32; otherwise n += 1; in both cases ring[(head + n - 1) % 32] = { A.x, A.y, frame }.
 *      cx, cy = A and last = frame are set whether or not a point was appended.
 *   5. Frees.  An occupied slot no owner of this frame named, with frame - last > max_missed, is zeroed, all 416 bytes.
 *   6. Fresh owners (owners that are not known) take the lowest free slots (id == 0) in list order, after the frees: id = the identity, last = frame,
 *      n = 1, head = 0, ring[0] = { A.x, A.y, frame }, cx, cy = A; every other byte of the slot is zero.  An owner that finds no free slot is REFUSED.
 *   7. live = the occupied slots; frames += 1 -- also for a frame without boxes.
 *
 * Outputs per record t.  S = list_stride, or FFGPU_MAX_DET when d_lists is NULL.
 *   d_rows (required): row t of FFGPU_TRAILS_ROW + 4 S ints, every byte written, for streams[t] == -1 as zero: 16 ints { considered, known, fresh,
 *     refused, duplicate, anonymous, dropped, freed, live, frame, appended, drawn, clipped, 0, 0, 0 } (appended: the known owners of 4. that appended a
 *     point), then four ints per list box k (at FFGPU_TRAILS_ROW + 4 k): the MOTION ROW { n, dx, dy, df } of a box that is a known or fresh owner, zero
 *     for every other box.  n = the slot's live points after this frame; with O the slot's oldest live point, dx = cx - O.x and dy = cy - O.y, taken in
 *     64 bits and saturated to int; df = frame - O.frame, modulo 2^32 as signed.
 *   d_items (may be NULL: then items_stride, first_item and nitems must be 0): ffgpu_seg_items, 4-byte aligned, row t of items_stride items
 *     (1..FFGPU_SEG_ITEMS).  The call writes exactly the slots first_item .. first_item + nitems - 1 of row t (first_item >= 0, nitems >= 1,
 *     first_item + nitems <= items_stride): every byte of those slots and no other byte, so ffgpu_outline_scene_dev may write the row first and the
 *     trails the slots behind its markers.  THE ROW SHOWS THE STATE RIGHT AFTER RECORD t: several records of one stream in one call each get their
 *     own trail.  With P = points: a slot is DRAWN when id != 0, n >= 1 and (last == frame or FFGPU_TRAILS_COAST is set).  The k-th drawn slot in slot
 *     order owns the REGION first_item + k P .. first_item + k P + P - 1 while (k + 1) P <= nitems; further drawn slots get nothing and are counted in
 *     `clipped`; `drawn` counts the slots that got a region (with NULL items every drawn slot is clipped).
 *       Region item j < P - 1: the segment from live point j to live point j + 1 (0 = the oldest) when j + 1 < n, otherwise 32 zero bytes.
 *       Region item P - 1, the TIP: the segment from the newest live point to (cx, cy).
 *       Colour = palette entry id mod npalette (the non-negative remainder), or `color`; byte 3, `flags` and the reserved fields are 0.
 *       dash = coast_dash when last != frame, otherwise 0.  thickness T = the spec's; with FFGPU_TRAILS_TAPER the tip keeps T and ring item j gets
 *       1 + ((T - 1) * (j + 1)) / n, the division an integer one.
 *     Every slot of the range outside a region is 32 zero bytes; for streams[t] == -1 all of them are.
 * Redact, then draw, then outline, then trails, then caption. */
#define FFGPU_TRAIL_POINTS   32   /* ring entries per slot */
#define FFGPU_TRAILS_DETS    128  /* considered boxes per frame at most; also the largest capacity */
#define FFGPU_TRAILS_ROW     16   /* header ints of a trail row in front of the boxes' motion rows */
#define FFGPU_TRAILS_COAST   1    /* flags: a slot not seen in this frame is drawn too, dashed with coast_dash */
#define FFGPU_TRAILS_TAPER   2    /* flags: the trail thins out toward its oldest point */
typedef struct { int x, y, frame; } ffgpu_trail_point;   /* 12 bytes */
typedef struct {
    int id;                        /* 0: a free slot (all zero, all 416 bytes) */
    int last;                      /* the stream's frame number when the object was last seen */
    int n;                         /* live points, 0..points */
    int head;                      /* ring index of the oldest live point */
    int cx, cy;                    /* the anchor when last seen, converted */
    int reserved[2];               /* 0 */
    ffgpu_trail_point ring[FFGPU_TRAIL_POINTS];
} ffgpu_trail_slot;                /* 416 bytes: id 0, last 4, n 8, head 12, cx 16, cy 20, reserved 24, ring 32; behind each stream's 16-byte header */
typedef struct {
    int   capacity;                /* 1..128: slots per stream (as the state was sized) */
    int   max_missed;              /* 0..2^20: an object survives this many consecutive frames without being seen */
    int   identity;                /* FFGPU_ZONES_TYPE | _IDS; _NONE is rejected: there is nobody to remember */
    int   flags;                   /* 0 | FFGPU_TRAILS_COAST | FFGPU_TRAILS_TAPER; any other bit is rejected */
    float min_score;               /* finite, in [0, 1]: a box is considered from this score on */
    int   anchor;                  /* 0: the box's centre; 1: its bottom centre (the zones contract's anchor) */
    int   points;                  /* 2..32: the history kept per object */
    int   min_move;                /* 0..2^20: a point is appended from this Chebyshev distance to the newest one on */
    int   thickness;               /* 1..8 */
    int   coast_dash;              /* 0..6: the dash of a slot not seen in this frame */
    unsigned char color[4];        /* the colour when palette is NULL */
    int   reserved0;               /* 0 */
    const unsigned char *palette;  /* HOST, npalette x 4 bytes, or NULL: exactly ffgpu_outline_spec's */
    int   npalette;                /* 0 with a NULL palette, else 1..256 */
    int   reserved;                /* 0 */
} ffgpu_trails_spec;               /* 64 bytes: capacity 0, max_missed 4, identity 8, flags 12, min_score 16, anchor 20, points 24, min_move 28, */
                                   /* thickness 32, coast_dash 36, color 40, reserved0 44, palette 48, npalette 56, reserved 60 */

/* pure host code: the bytes of the state of nstreams (1..65536) streams of capacity (1..128) slots; 0 for arguments outside their ranges */
size_t ffgpu_trails_state_bytes(int nstreams, int capacity);
/* pure host code: 0, or -1 with the message in ffgpu_last_error */
int ffgpu_trails_spec_check(const ffgpu_trails_spec *spec);
/* zeroes the state of one stream, or of all with which_stream == -1, in stream order (a memset; no kernel) */
int ffgpu_trails_reset_dev(void *d_state, int nstreams, int capacity, int which_stream, void *stream);

/* The operator, on device records and lists with no executor.  d_records, d_lists, list_stride and the HOST array list_first are the draw operators'.
 * One workgroup per video stream walks that stream's records of the call serially, the slots' 32-byte heads in LDS and the rings in global memory;
 * streams, list_first and spec (with its palette) are HOST memory and free again on return; the tables and the palette travel as kernel arguments,
 * 64 records per launch, the launches of one call in order on `stream`, the state passing through memory between them.  Enqueued without
 * synchronising.  Rejected before anything is launched, with the entry's index in the message where there is one: the reasons of
 * ffgpu_zones_boxes_dev that apply (NULL records, streams, spec, state or rows, ntargets < 1, nstreams outside 1..65536, a stream index outside
 * -1..nstreams-1, a state that is not 16-byte aligned, a bad list_stride, a negative list start), a spec field outside its range, identity
 * FFGPU_ZONES_NONE, unknown flag bits, a reserved field that is not 0, npalette not matching palette, d_ids (required exactly when identity ==
 * FFGPU_ZONES_IDS: NULL then, or given otherwise, is rejected), and the items: NULL with items_stride, first_item or nitems not 0; otherwise not
 * 4-byte aligned, items_stride outside 1..512, first_item < 0, nitems < 1, first_item + nitems > items_stride.  A rejected call leaves the state as
 * it was. */
int ffgpu_trails_boxes_dev(const void *d_records, const void *d_lists, int list_stride, const int *list_first, const int *streams, int ntargets,
                           const ffgpu_trails_spec *spec, void *d_state, int nstreams, const void *d_ids, void *d_rows, void *d_items, int items_stride,
                           int first_item, int nitems, void *stream);

#define FFGPU_TRAILS_ENTRIES 0   /* entry n's full post-NMS list is record n; ntargets == batch; S as FFGPU_TRACK_ENTRIES                          */
#define FFGPU_TRAILS_MERGED  1   /* picture g's merged list (last ffgpu_exec_merge_tiles) is record g; ntargets == its nimages; S as FFGPU_TRACK_MERGED */
/* On an executor: a post-pass like ffgpu_exec_zones, with its stream, FFGPU_SPLIT2 and FFGPU_TRAILS_MERGED rules, enqueued on `stream` (NULL = the
 * executor's own; it must be the stream of the forward or merge it follows) without synchronising.  The captured graph, the records, the full lists,
 * the ring and the host mirror are untouched; state, rows and items are the caller's, and d_ids is what ffgpu_exec_track wrote for the same `which`.
 * Rejected like the operator, and: ntargets not as stated, a `which` that is neither, FFGPU_TRAILS_MERGED when no merge has run, the wrong stream.  A
 * rejected call leaves the state and the executor usable. */
int ffgpu_exec_trails(ffgpu_exec *ex, int which, const int *streams, int ntargets, const ffgpu_trails_spec *spec, void *d_state, int nstreams,
                      const void *d_ids, void *d_rows, void *d_items, int items_stride, int first_item, int nitems, void *stream);

/* ---- heat maps: where the boxes have been, accumulated per stream on the device and blended into the frames -----------------------------------
 * The zones state keeps one anchor per object and the trails state 32; nothing is kept per PLACE.  What follows keeps, per video stream, a grid of
 * cells in the caller's device memory into which the considered boxes of any record (plain, merged, tracked, relabelled or gated) are accumulated
 * with an integer decay -- a stateful per-stream pass in the shape of ffgpu_zones_boxes_dev / ffgpu_trails_boxes_dev -- and a per-pixel operator
 * that colour-maps the grid and ALPHA-BLENDS it into u8 BGR and NV12 frames where they lie: the first frame writer that mixes a colour into the
 * picture instead of replacing bytes.  Integers throughout, except the fp32 anchor; no atomics; one owner per written byte; the same bytes on every
 * run (tests/heat/heatref.py restates both in numpy).
 *
 * State, in the caller's device memory (16-byte aligned, ffgpu_heat_state_bytes(nstreams, gw, gh) bytes; all-zero is the valid empty state, so
 * hipMemsetAsync or ffgpu_heat_reset_dev initialises it): per stream a 16-byte header { int frames; unsigned peak; int reserved[2]; } then gw * gh
 * cells of unsigned, row-major, the stream's block rounded up to 16 bytes.  The geometry comes from the spec, as capacity does for tracks: the cell
 * side is c = 1 << cell_log2, the grid is anchored at picture pixel (0, 0), cell (i, j) covers x in [i c, (i + 1) c - 1] and y in [j c, (j + 1) c - 1],
 * and the grid's EXTENT is gw c x gh c pixels; it need not match any frame's size.  The kernels are total over any state bytes: a cell is read as
 * unsigned and clamped to FFGPU_HEAT_MAX where it is read, and so is peak where the blend reads it.  The grid is a documented, readable product: a
 * dashboard copies it out as it is.  The reserved words of the header are never written.
 *
 * ACCUMULATE.  One frame of one stream, in this order (streams, ntargets, time order, -1 entries, list_first and the clamps of the counts: exactly
 * as ffgpu_zones_boxes_dev):
 *   1. Considered boxes.  The list is walked in list order.  A box QUALIFIES by the redact contract's rule: score >= min_score (a NaN score never
 *      qualifies; with a NaN min_score nothing does) and its type allowed by the HOST array classes / nclasses (NULL allows every type).  Boxes are
 *      considered until FFGPU_HEAT_DETS are; further qualifying boxes are counted in `dropped`.
 *   2. Decay.  With decay_shift k in 1..16 every cell becomes v - ((v + (1 << k) - 1) >> k): the rounding is up, so a non-zero cell loses at least
 *      1 per frame and old heat reaches exactly zero.  k = 0 means no decay.  Decay also runs for a frame without boxes.
 *   3. Deposit.  Every considered box adds to the cells of its footprint; sums are taken in 64 bits and the cell is min(sum, FFGPU_HEAT_MAX) --
 *      saturating sums of non-negative terms do not depend on order.
 *      FFGPU_HEAT_ANCHOR: the anchor is computed and converted exactly as in step 2 of the trails contract (fp32, not contracted: px = (x1 + x2) *
 *        0.5f; py = anchor ? y2 : (y1 + y2) * 0.5f; then the draw contract's conversion): A.  If A lies outside [0, gw c - 1] x [0, gh c - 1] the box
 *        deposits nothing and is counted in `outside`.  Otherwise, with (i, j) = (A.x >> cell_log2, A.y >> cell_log2), every grid cell at Chebyshev
 *        distance d <= spread from (i, j) receives gain >> d; cells beyond the grid are simply not there.
 *      FFGPU_HEAT_BOX: the integer corners (a, b, c, d) of the draw contract, clipped to the extent: X0 = max(a, 0), Y0 = max(b, 0), X1 = min(c,
 *        gw c - 1), Y1 = min(d, gh c - 1).  If a > c, b > d, or the clipped region is empty, the box is counted in `outside`.  Otherwise every cell
 *        from (X0 >> k, Y0 >> k) to (X1 >> k, Y1 >> k) receives gain.  spread must be 0.
 *   4. Finish.  peak = the largest cell; frames += 1 (modulo 2^32).
 *   d_rows (required): row t of FFGPU_HEAT_ROW ints, every byte written, for streams[t] == -1 as zero: { considered, dropped, outside, frame, peak,
 *     saturated, 0, 0 }; frame is `frames` before step 4 and saturated the number of cells at FFGPU_HEAT_MAX.
 *
 * BLEND.  Target t shows the grid of stream streams[t] AS IT IS WHEN THE LAUNCH RUNS IN STREAM ORDER: several frames of one stream in one call all
 * show the same map.  streams[t] == -1 leaves the target untouched.  Targets are as the draw contract takes them (a NULL pixel address skips the
 * target, the const pointers are written through, targets must not overlap).  For a pixel (x, y) inside the target's w x h, with k = cell_log2:
 *   Outside the extent: a pixel with x >= gw c or y >= gh c is untouched.
 *   Cell level: F = full_scale when full_scale >= 1; with full_scale == 0 F is the stream's peak, and a peak of 0 draws nothing in that target.
 *     L(i, j) = min(255, (cell(i, j) * 255) / F), in 64-bit integers, rounded down.
 *   Pixel level: FFGPU_HEAT_NEAREST: L(x >> k, y >> k).  FFGPU_HEAT_SMOOTH is bilinear between cell centres, in integers, with h = c / 2:
 *     i0 = (x - h) >> k, an arithmetic shift, so i0 may be -1; fx = (x - h) & (c - 1); j0 and fy are formed likewise; the indices i0, i0 + 1, j0,
 *     j0 + 1 are each clamped to the grid; level = (L00 (c - fx)(c - fy) + L10 fx (c - fy) + L01 (c - fx) fy + L11 fx fy + c c / 2) >> (2 k).
 *   Alpha: a pixel with level < max(floor, 1) is not written.  Otherwise a = opacity; with FFGPU_HEAT_RAMP_ALPHA a = (level * opacity + 127) / 255,
 *     and a == 0 is not written.
 *   Byte: new = (old (255 - a) + pal[level][ch] a + 127) / 255.
 *   NV12: luma is blended per pixel with pal[level][0].  Chroma sample (i, j) takes the level and alpha of luma pixel (2 i, 2 j), which is always
 *     inside w x h; it blends U with pal[..][1] and V with pal[..][2] and is not written when that pixel is not.
 *   Untouched bytes: every byte that is not written stays -- row padding, pixels below the floor or outside the extent, memory before and behind
 *     the target.  The state is only read.
 * The built-in palette (a NULL `palette`; ffgpu_heat_palette fills it) is a piecewise-linear ramp in integers through the (B, G, R) anchors
 * (255, 0, 0) at level 0, (255, 255, 0) at 64, (0, 255, 0) at 128, (0, 255, 255) at 192 and (0, 0, 255) at 255; between anchors v0 < v1:
 * ch = (c0 (v1 - v) + c1 (v - v0) + (v1 - v0) / 2) / (v1 - v0).  For NV12 each entry is converted, with >> arithmetic and a clamp to 0..255:
 * Y = (29 B + 150 G + 77 R + 128) >> 8, U = ((128 B - 85 G - 43 R + 128) >> 8) + 128, V = ((-21 B - 107 G + 128 R + 128) >> 8) + 128.
 * Redact and blur first, then the heat blend, then draw, outline, trails and caption: the overlays lie on top of the map. */
#define FFGPU_HEAT_MAX        0x7fffffff  /* what a cell saturates at, and what a cell or peak above it reads as */
#define FFGPU_HEAT_DETS       128  /* considered boxes per frame at most */
#define FFGPU_HEAT_ROW        8    /* ints of a row */
#define FFGPU_HEAT_ANCHOR     0    /* mode: a box deposits round its anchor's cell */
#define FFGPU_HEAT_BOX        1    /* mode: a box deposits into every cell its clipped region touches */
#define FFGPU_HEAT_NEAREST    0    /* sampling: a pixel takes its cell's level */
#define FFGPU_HEAT_SMOOTH     1    /* sampling: bilinear between cell centres */
#define FFGPU_HEAT_RAMP_ALPHA 1    /* blend flags: the alpha grows with the level */
typedef struct {
    int   gw, gh;                  /* 1..128 each: the grid, as the state was sized */
    int   cell_log2;               /* 1..8: a cell is 1 << cell_log2 pixels wide and high */
    int   mode;                    /* FFGPU_HEAT_ANCHOR | FFGPU_HEAT_BOX */
    int   flags;                   /* 0: no flag is defined, any bit is rejected */
    int   anchor;                  /* 0: the box's centre; 1: its bottom centre (the zones contract's anchor); read by FFGPU_HEAT_ANCHOR */
    int   spread;                  /* 0..4: the Chebyshev radius, in cells, of an anchor's footprint; 0 with FFGPU_HEAT_BOX */
    int   gain;                    /* 1..65536: what a box adds to a cell */
    int   decay_shift;             /* 0..16: 0 = no decay */
    float min_score;               /* any value: a box qualifies from this score on (NaN: none does) */
    const unsigned char *classes;  /* HOST, nclasses bytes, non-zero = allowed; NULL: every type */
    int   nclasses;                /* 0 with NULL classes, else 1..256 */
    int   reserved;                /* 0 */
} ffgpu_heat_spec;                 /* 56 bytes: gw 0, gh 4, cell_log2 8, mode 12, flags 16, anchor 20, spread 24, gain 28, decay_shift 32, */
                                   /* min_score 36, classes 40, nclasses 48, reserved 52 */
typedef struct {
    int   gw, gh, cell_log2;       /* the grid's geometry, as ffgpu_heat_spec's */
    int   full_scale;              /* >= 1: the cell value shown as level 255; 0: the stream's peak */
    int   floor;                   /* 0..255: a pixel below max(floor, 1) is not written */
    int   opacity;                 /* 1..255 */
    int   sampling;                /* FFGPU_HEAT_NEAREST | FFGPU_HEAT_SMOOTH */
    int   flags;                   /* 0 | FFGPU_HEAT_RAMP_ALPHA; any other bit is rejected */
    const unsigned char *palette;  /* HOST, 256 x 4 bytes: B G R 0 (BGR targets) or Y U V 0 (NV12 targets), byte 3 ignored, nothing is converted; */
                                   /* NULL: the built-in palette of the target's format */
    int   reserved[2];             /* 0 */
} ffgpu_heat_blend_spec;           /* 48 bytes: gw 0, gh 4, cell_log2 8, full_scale 12, floor 16, opacity 20, sampling 24, flags 28, palette 32, reserved 40 */

/* pure host code: the bytes of the state of nstreams (1..65536) streams of gw x gh (1..128 each) cells; 0 for arguments outside their ranges */
size_t ffgpu_heat_state_bytes(int nstreams, int gw, int gh);
/* pure host code: 0, or -1 with the message in ffgpu_last_error */
int ffgpu_heat_spec_check(const ffgpu_heat_spec *spec);
int ffgpu_heat_blend_spec_check(const ffgpu_heat_blend_spec *spec);
/* pure host code: the built-in palette, 256 x 4 bytes, B G R 0 (nv12 == 0) or Y U V 0 (nv12 != 0); -1 for a NULL out */
int ffgpu_heat_palette(int nv12, unsigned char out[1024]);
/* zeroes the state of one stream, or of all with which_stream == -1, in stream order (a memset; no kernel) */
int ffgpu_heat_reset_dev(void *d_state, int nstreams, int gw, int gh, int which_stream, void *stream);

/* The accumulate operator, on device records and lists with no executor.  d_records, d_lists, list_stride and the HOST array list_first are the draw
 * operators'.  One workgroup per video stream walks that stream's records of the launch serially with the stream's grid in LDS, loaded once and
 * stored once; streams, list_first and spec (with its classes) are HOST memory and free again on return; the tables travel as a kernel argument,
 * 64 records per launch, the launches of one call in order on `stream`, the state passing through memory between them.  Enqueued without
 * synchronising.  Rejected before anything is launched, with the entry's index in the message where there is one: the reasons of
 * ffgpu_zones_boxes_dev that apply (NULL records, streams, spec, state or rows, ntargets < 1, nstreams outside 1..65536, a stream index outside
 * -1..nstreams-1, a state that is not 16-byte aligned, a bad list_stride, a negative list start), every spec field outside its range, an unknown
 * mode, any flag bit, a reserved field that is not 0, nclasses inconsistent with classes, a non-zero spread with FFGPU_HEAT_BOX.  A rejected call
 * leaves the state as it was. */
int ffgpu_heat_boxes_dev(const void *d_records, const void *d_lists, int list_stride, const int *list_first, const int *streams, int ntargets,
                         const ffgpu_heat_spec *spec, void *d_state, int nstreams, void *d_rows, void *stream);

#define FFGPU_HEAT_ENTRIES 0   /* entry n's full post-NMS list is record n; ntargets == batch                                          */
#define FFGPU_HEAT_MERGED  1   /* picture g's merged list (last ffgpu_exec_merge_tiles) is record g; ntargets == its nimages            */
/* On an executor: a post-pass like ffgpu_exec_zones, with its stream, FFGPU_SPLIT2 and FFGPU_HEAT_MERGED rules, enqueued on `stream` (NULL = the
 * executor's own; it must be the stream of the forward or merge it follows) without synchronising.  The captured graph, the records, the full lists,
 * the ring and the host mirror are untouched; state and rows are the caller's.  Rejected like the operator, and: ntargets not as stated, a `which`
 * that is neither, FFGPU_HEAT_MERGED when no merge has run, the wrong stream.  A rejected call leaves the state and the executor usable. */
int ffgpu_exec_heat(ffgpu_exec *ex, int which, const int *streams, int ntargets, const ffgpu_heat_spec *spec, void *d_state, int nstreams,
                    void *d_rows, void *stream);

/* The blend operators.  There is no executor form: the blend reads state, not records.  streams and spec (with its palette) are HOST memory and free
 * again on return; the palette, the targets and their streams travel as ONE by-value kernel argument, 64 targets per launch (more targets: more
 * launches, in order on `stream`).  A workgroup owns a 64 x 64 pixel block of its target anchored at (0, 0), computes the levels of the cells the
 * block can reach first and leaves without loading a pixel when every one is below max(floor, 1).  Enqueued without synchronising.  Rejected before
 * anything is launched, with the target's index where there is one: everything the draw operators reject about targets, NULL state, streams, spec or
 * targets, ntargets < 1, nstreams outside 1..65536, a stream index outside -1..nstreams-1, a state that is not 16-byte aligned, a field outside its
 * range, an unknown sampling, unknown flag bits, a reserved field that is not 0, a negative full_scale. */
int ffgpu_heat_blend_bgr_dev(const void *d_state, int nstreams, const int *streams, const ffgpu_bgr_frame *targets, int ntargets,
                             const ffgpu_heat_blend_spec *spec, void *stream);
int ffgpu_heat_blend_nv12_dev(const void *d_state, int nstreams, const int *streams, const ffgpu_nv12_frame *targets, int ntargets,
                              const ffgpu_heat_blend_spec *spec, void *stream);

/* ---- motion maps: a per-stream background model of the frames' luma, the cells that changed, and a gate on the boxes that move ------------------
 * Every pass above starts from the boxes.  This family is the first that reads WHOLE FRAMES over time: per video stream it keeps a background model
 * of the luma in the caller's device memory, counts per cell the pixels of the stream's last frame that differ from it, and gates any record (plain,
 * merged, tracked, relabelled) by whether a box lies on cells that move -- a poster, a parked car or a reflection the detector fires on in every
 * frame does not.  (The trails family's "motion row" is a different thing: displacement of an identified anchor over its kept history.  The family
 * here is named `motion`: pixels over time.)  Integers throughout; no atomics; one owner per written byte; the same bytes on every run; total over
 * any state bytes (tests/motion/motionref.py restates it in numpy).
 *
 * Geometry, from the spec: frames and model are w x h pixels; a cell is c = 1 << cell_log2 pixels wide and high, anchored at pixel (0, 0); the grid
 * is gw = ceil(w / c) by gh = ceil(h / c) cells, the last column and row partial where c does not divide w or h.
 *
 * State, in the caller's device memory (16-byte aligned, ffgpu_motion_state_bytes(nstreams, w, h, cell_log2) bytes; all-zero is the valid empty
 * state, so hipMemsetAsync or ffgpu_motion_reset_dev initialises it).  Per stream, in this order:
 *   1. a header { int frames; int reserved[3]; } (the reserved words are never written);
 *   2. the background PLANE: h rows of ALIGN(w, 8) unsigned short, row-major, luma in 8.8 fixed point; the padding shorts of a row are never written;
 *   3. gw * gh unsigned CELLS, row-major, rounded up to 16 bytes (the rounding bytes are never written): the number of changed pixels of the cell in
 *      the stream's last frame.
 * Plane and cells are documented, readable products.
 *
 * UPDATE.  One frame of one stream.  Luma y of a pixel: NV12: the Y byte (the UV plane is not read); BGR: y = (29 B + 150 G + 77 R + 128) >> 8.
 * For every pixel, with cur = y << 8, bg the stored short (any value) and d = cur - bg as int:
 *   If the header's `frames` is 0 the pixel is not changed and bg = cur.
 *   Otherwise the pixel is CHANGED when |d| > threshold << 8; k = learn_shift_changed for a changed pixel, learn_shift for any other;
 *     k == 0: bg = cur (plain frame differencing); k in 1..15: bg += sgn(d) * ((|d| + (1 << k) - 1) >> k) -- the rounding is up, so the model reaches
 *     cur exactly; k == 16: bg stays.
 *   cell(i, j) = the changed pixels with x >> cell_log2 == i and y >> cell_log2 == j.  Every cell of the stream is written.
 * Then frames += 1 (modulo 2^32), and row t of FFGPU_MOTION_ROW ints, every byte written: { frame (frames before the increment), changed (pixels),
 * active (cells with count >= min_pixels), x0, y0, x1, y1, warm, 0 x 8 }.  The bounding box of the active cells is in pixels: x0 = c * min i,
 * x1 = min(c * (max i + 1), w) - 1, likewise y; with no active cell it is (0, 0, -1, -1).  warm = (frames after the increment) > warmup.
 * Targets: streams[t] == -1 or a NULL pixel address leaves the state alone, and the row is zero (the size of such a target is not looked at).  Any
 * other target whose w or h differ from the spec's is rejected.  A stream may appear several times in one call; its frames are then in time
 * order, and the result is byte for byte what one call per frame leaves.
 *
 * GATE.  Only reads the state, AS IT IS WHEN THE LAUNCH RUNS IN STREAM ORDER.  Per record t of stream streams[t]:
 *   Considered boxes: step 1 of the heat contract with the cap FFGPU_MOTION_DETS; further qualifying boxes are counted in `dropped`.
 *   For a considered box, the integer corners (a, b, c, d) of the draw contract clipped to w x h: X0 = max(a, 0), Y0 = max(b, 0), X1 = min(c, w - 1),
 *     Y1 = min(d, h - 1).  If a > c, b > d or the clip is empty the box is counted in `outside` and touched = active = 0.  Otherwise touched = the
 *     cells from (X0 >> k, Y0 >> k) to (X1 >> k, Y1 >> k), k = cell_log2, and active = those among them with count >= min_pixels.
 *   The stream is WARM when frames > warmup.  Warm: a box is MOVING when touched >= 1 and active * 256 >= cover * touched.  Not warm: every
 *     considered box is MOVING -- the gate fails open, so no detection is lost while the model learns.
 *   d_words (required): row t of 8 + 2 S ints (S = the list stride), every byte written: { considered, dropped, outside, moving, warm, frames, 0, 0 },
 *     then { touched, active } per list box, zero for a box that was not considered.
 *   d_out_records / d_out_lists (may be NULL): the considered boxes with MOVING != (flags & FFGPU_MOTION_GATE_INVERT), in list order and unchanged,
 *     laid out by the zones gated record's rules word for word (count = min(n, FFGPU_MAX_DET), nfull = n, ncand and overflow bit 0 copied, bit 2 =
 *     n > FFGPU_MAX_DET; unused box slots of the record and of the list are zero).  The outputs must not overlap the inputs.
 *   streams[t] == -1: every output byte of the entry is written, as zero.
 * The composition: update, forward, gate, then track, redact, draw or heat ON THE GATED RECORD.  FFGPU_MOTION_GATE_INVERT gives the boxes that
 * stand still. */
#define FFGPU_MOTION_DETS        128  /* considered boxes per record at most */
#define FFGPU_MOTION_ROW         16   /* ints of an update row */
#define FFGPU_MOTION_WORDS       8    /* ints in front of a gate row's { touched, active } pairs */
#define FFGPU_MOTION_GATE_INVERT 1    /* flags bit 0: the gated record holds the considered boxes that are NOT moving */
#define FFGPU_MOTION_MAX_SIDE    8192 /* w and h at most */
typedef struct {
    int   w, h;                    /* 1..8192: the size of the stream's frames and of the model */
    int   cell_log2;               /* 2..6: a cell is c = 1 << cell_log2 pixels wide and high */
    int   threshold;               /* 1..255: a pixel is changed when |luma - background| exceeds it */
    int   learn_shift;             /* 0..16: the model's learning rate at an unchanged pixel (0: take the frame, 16: keep the model) */
    int   learn_shift_changed;     /* 0..16: the same at a changed pixel */
    int   min_pixels;              /* 1..c c: a cell is active from this many changed pixels on */
    int   cover;                   /* 1..256: a box moves when active * 256 >= cover * touched */
    int   warmup;                  /* 0..65535: the gate fails open until the stream has seen more frames than this */
    int   flags;                   /* 0 | FFGPU_MOTION_GATE_INVERT; any other bit is rejected */
    float min_score;               /* any value: a box qualifies from this score on (NaN: none does); read by the gate */
    int   nclasses;                /* 0 with NULL classes, else 1..256 */
    const unsigned char *classes;  /* HOST, nclasses bytes, non-zero = allowed; NULL: every type; read by the gate */
    int   reserved[2];             /* 0 */
} ffgpu_motion_spec;               /* 64 bytes: w 0, h 4, cell_log2 8, threshold 12, learn_shift 16, learn_shift_changed 20, min_pixels 24, cover 28, */
                                   /* warmup 32, flags 36, min_score 40, nclasses 44, classes 48, reserved 56 */

/* pure host code: the bytes of the state of nstreams (1..65536) streams of w x h (1..8192 each) pixels with cells of 1 << cell_log2 (2..6); 0 for
 * arguments outside their ranges */
size_t ffgpu_motion_state_bytes(int nstreams, int w, int h, int cell_log2);
/* pure host code: 0, or -1 with the message in ffgpu_last_error */
int ffgpu_motion_spec_check(const ffgpu_motion_spec *spec);
/* zeroes the state of one stream, or of all with which_stream == -1, in stream order (a memset; no kernel) */
int ffgpu_motion_reset_dev(void *d_state, int nstreams, int w, int h, int cell_log2, int which_stream, void *stream);

/* The update operators.  targets (the frames, as the draw operators take them; only read), streams and spec are HOST memory and free again on
 * return.  The host enqueues ROUND r -- the r-th occurrence of every stream in the call -- behind round r - 1: stream order is the barrier.  A round
 * is two launches per 64 targets: k_motion_update, in which a workgroup owns a tile of 64 x 64 pixels -- whole cells at every legal cell size --
 * reads the frame's bytes and the plane once, writes the plane once and stores each of its cells from one lane; then a small launch, one workgroup
 * per target, that reduces the stream's cells to the row and writes `frames`.  The update launch only reads `frames`.  No atomics.  Enqueued
 * without synchronising.  Rejected before anything is enqueued, with the target's index where there is one: everything the draw operators reject
 * about targets, NULL targets, streams, spec, state or rows, ntargets < 1, nstreams outside 1..65536, a stream index outside -1..nstreams-1, a state
 * that is not 16-byte aligned, every spec field outside its range, unknown flag bits, a reserved field that is not 0, nclasses inconsistent with
 * classes, a target whose size is not the spec's.  A rejected call leaves the state as it was. */
int ffgpu_motion_update_bgr_dev(const ffgpu_bgr_frame *targets, int ntargets, const int *streams, const ffgpu_motion_spec *spec, void *d_state,
                                int nstreams, void *d_rows, void *stream);
int ffgpu_motion_update_nv12_dev(const ffgpu_nv12_frame *targets, int ntargets, const int *streams, const ffgpu_motion_spec *spec, void *d_state,
                                 int nstreams, void *d_rows, void *stream);

/* The gate operator, on device records and lists with no executor.  d_records, d_lists, list_stride and the HOST array list_first are the draw
 * operators'; streams and spec (with its classes) are HOST memory and free again on return.  One workgroup per record, 64 records per launch, the
 * tables travelling as a kernel argument.  Enqueued without synchronising.  Rejected before anything is launched: the reasons of
 * ffgpu_heat_boxes_dev that apply (with NULL words for NULL rows), the spec as above, d_out_lists without d_out_records, outputs that are the
 * inputs. */
int ffgpu_motion_gate_dev(const void *d_records, const void *d_lists, int list_stride, const int *list_first, const int *streams, int ntargets,
                          const ffgpu_motion_spec *spec, const void *d_state, int nstreams, void *d_words, void *d_out_records, void *d_out_lists,
                          void *stream);

#define FFGPU_MOTION_ENTRIES 0   /* entry n's full post-NMS list is record n; ntargets == batch; S = ffgpu_exec_cand_capacity               */
#define FFGPU_MOTION_MERGED  1   /* picture g's merged list (last ffgpu_exec_merge_tiles) is record g; ntargets == its nimages; S as FFGPU_ZONES_MERGED */
/* On an executor: a post-pass like ffgpu_exec_heat, with its stream, FFGPU_SPLIT2 and FFGPU_MOTION_MERGED rules, enqueued on `stream` (NULL = the
 * executor's own; it must be the stream of the forward or merge it follows) without synchronising.  The captured graph, the records, the full lists,
 * the ring and the host mirror are untouched; the state is only read; words and the gated records are the caller's, pitched by S as the zones pass's.
 * Rejected like the operator, and: ntargets not as stated, a `which` that is neither, FFGPU_MOTION_MERGED when no merge has run, the wrong stream,
 * lists longer than 2^24 boxes.  A rejected call leaves the state and the executor usable. */
int ffgpu_exec_motion_gate(ffgpu_exec *ex, int which, const int *streams, int ntargets, const ffgpu_motion_spec *spec, const void *d_state, int nstreams,
                           void *d_words, void *d_out_records, void *d_out_lists, void *stream);

/* ---- preview surfaces: frames scaled by area averaging into panes, several streams composed into one wall on the device --------------------------
 * Every operator above leaves a frame at its decoded size.  What a deployment shows is smaller: an operator's wall of 16 or 64 cameras, a thumbnail,
 * a low-bitrate substream.  This family scales a source region of a frame into a PANE of a destination surface; a wall is several panes whose
 * destinations name the same surface.  There is no format conversion: BGR to BGR, NV12 to NV12.  Integers throughout; no atomics; one owner per
 * written byte; the same bytes on every run (tests/preview/previewref.py restates it in numpy).
 *
 * RESOLVE (ffgpu_preview_rect: out = { sx, sy, sw, sh, X0, Y0, ow, oh }).  The defaults first: sw == sh == 0 is the whole frame (sx, sy must be 0),
 * dw == dh == 0 the whole surface (dx, dy must be 0).  Then the source region must lie inside the source frame and the pane inside the destination
 * surface, every side 1..FFGPU_PREVIEW_MAX_SIDE; NV12 requires sx, sy, dx and dy even.  FFGPU_PREVIEW_STRETCH: ow = dw, oh = dh, ox = oy = 0.
 * FFGPU_PREVIEW_FIT, in 64-bit integers: if sw dh >= sh dw then ow = dw and oh = clamp((2 sh dw + sw) / (2 sw), 1, dh), otherwise oh = dh and
 * ow = clamp((2 sw dh + sh) / (2 sh), 1, dw); ox = (dw - ow) >> 1, oy = (dh - oh) >> 1, for NV12 both rounded down to even.  X0 = dx + ox,
 * Y0 = dy + oy.  The IMAGE is the ow x oh rectangle at (X0, Y0); the BARS are the rest of the pane.
 *
 * RESAMPLE: one rule for every ratio, down or up.  A plane of sw x sh samples becomes ow x oh.  Destination sample (i, j) covers
 * [i sw, (i + 1) sw) horizontally, in units of 1 / ow source samples; source sample x covers [x ow, (x + 1) ow); wx(i, x) is the length of their
 * intersection, so the wx of a destination sample add up to sw; wy(j, y) likewise with sh and oh.  With D = sw sh:
 *     out(i, j) = (sum_y wy(j, y) * sum_x wx(i, x) * v(x, y) + (D >> 1)) / D, rounded down.
 * The inner sum fits 32 bits (255 * 8192 < 2^21); the outer sum is taken in 64 bits once 255 D >= 2^32; the division is exact, not a float
 * reciprocal.  What follows from the rule: ow == sw and oh == sh gives a byte copy; integer ratios k x l give the rounded mean of each k x l block;
 * a constant plane stays constant; mirroring the source mirrors the image.
 *
 * BGR: the three channels are resampled independently, as three interleaved planes.
 * NV12: the Y plane is resampled as above.  The UV plane is resampled as two planes, U and V: the source region is ((sw + 1) / 2) x ((sh + 1) / 2) at
 * (sx / 2, sy / 2), the destination region ((ow + 1) / 2) x ((oh + 1) / 2) at (X0 / 2, Y0 / 2), the same rule with those sizes.  Ownership of
 * chroma: destination chroma sample (i, j) is written by the pane whose rectangle holds luma pixel (2 i, 2 j) -- as image when that pixel lies in
 * the IMAGE, as bar otherwise.  `matrix` of the frames is not read.
 *
 * Bars take `fill`: B G R per pixel, or Y per luma pixel with U V per owned chroma sample.  With FFGPU_PREVIEW_KEEP_BARS they are not written.
 * Untouched: every byte of a destination surface outside the panes, row padding, memory before and behind the surfaces, every source byte, kept
 * bars.  A pane whose source or destination pixel address (bgr / y) is NULL is skipped; its sizes are not looked at.  The gaps of a wall are the
 * caller's memset: the operator writes panes only.  One-pixel outlines survive area averaging only as faint lines: draw with a thickness near the
 * ratio before scaling. */
#define FFGPU_PREVIEW_STRETCH    0   /* fit: the source region fills the pane */
#define FFGPU_PREVIEW_FIT        1   /* fit: aspect kept, the image centred in the pane, bars round it */
#define FFGPU_PREVIEW_KEEP_BARS  1   /* flags bit 0: the bars' bytes are not written */
#define FFGPU_PREVIEW_MAX_SIDE   8192
#define FFGPU_PREVIEW_MAX_PANES  4096
typedef struct {
    int sx, sy, sw, sh;            /* source region; sw == sh == 0: the whole frame (sx, sy must be 0) */
    int dx, dy, dw, dh;            /* pane in the destination surface; dw == dh == 0: the whole surface (dx, dy must be 0) */
} ffgpu_preview_pane;              /* 32 bytes: sx 0, sy 4, sw 8, sh 12, dx 16, dy 20, dw 24, dh 28 */
typedef struct {
    int fit;                       /* FFGPU_PREVIEW_STRETCH or FFGPU_PREVIEW_FIT */
    int flags;                     /* 0 | FFGPU_PREVIEW_KEEP_BARS; any other bit is rejected */
    unsigned char fill[4];         /* B G R 0 or Y U V 0, byte 3 must be 0 */
    int reserved;                  /* 0 */
} ffgpu_preview_spec;              /* 16 bytes: fit 0, flags 4, fill 8, reserved 12 */

/* pure host code: 0, or -1 with the message in ffgpu_last_error */
int ffgpu_preview_spec_check(const ffgpu_preview_spec *spec);
/* pure host code: RESOLVE for one pane of a src_w x src_h frame into a dst_w x dst_h surface */
int ffgpu_preview_rect(int src_w, int src_h, int dst_w, int dst_h, const ffgpu_preview_pane *pane, const ffgpu_preview_spec *spec, int nv12, int out[8]);
/* pure host code: lays out a wall and fills dx, dy, dw, dh of npanes panes, the source fields zero.  rows = ceil(npanes / cols);
 * cw = (dst_w - (cols + 1) gap) / cols and ch = (dst_h - (rows + 1) gap) / rows; pane k lies at column k % cols and row k / cols:
 * dx = gap + col (cw + gap), dy = gap + row (ch + gap).  For NV12 the gap must be even, and cw and ch are rounded down to even.  Rejected: npanes or
 * cols below 1, cols above npanes, gap below 0, cw or ch below 1. */
int ffgpu_preview_grid(int npanes, int cols, int dst_w, int dst_h, int gap, int nv12, ffgpu_preview_pane *out);
/* pure host code: out = { the columns and the rows of a workgroup's tile of destination samples, the planes one launch takes } */
int ffgpu_preview_tile(int out[3]);

/* The operators.  srcs, dsts, panes and spec are HOST arrays, free again on return; pane p reads srcs[p] and writes into dsts[p] (the const pointers
 * of the destinations are written through); frames are described exactly as the draw operators take them.  A workgroup owns a tile of destination
 * samples of one pane, anchored at the pane's origin, image and bars alike, and is the only writer of those bytes; it reads the source bytes under
 * its tile once with aligned loads, takes the horizontal sums once per source row into LDS and runs the vertical sums over them.  The planes
 * travel as a kernel argument, 32 per launch; more panes are more launches, in order on `stream`.  Enqueued without synchronising; stream order is
 * the only barrier.  There is no executor form: the operator reads frames, not records.  Rejected before anything is launched, with the pane's
 * index: everything the draw operators reject about a frame description, for sources and destinations; NULL arrays or spec; npanes outside
 * 1..FFGPU_PREVIEW_MAX_PANES; an unknown fit, unknown flag bits, fill[3] != 0, reserved != 0; a half-defaulted region; a region outside its frame
 * or a side above 8192; odd sx, sy, dx or dy for NV12; a pane whose source and destination pixel addresses are equal; two panes with the same
 * destination pixel address whose rectangles intersect (both indices).  Any other overlap of memory is the caller's responsibility. */
int ffgpu_preview_bgr_dev(const ffgpu_bgr_frame *srcs, const ffgpu_bgr_frame *dsts, const ffgpu_preview_pane *panes, int npanes,
                          const ffgpu_preview_spec *spec, void *stream);
int ffgpu_preview_nv12_dev(const ffgpu_nv12_frame *srcs, const ffgpu_nv12_frame *dsts, const ffgpu_preview_pane *panes, int npanes,
                           const ffgpu_preview_spec *spec, void *stream);

/* ---- warp surfaces: frames dewarped, rotated and rectified through a mesh of source positions on the device --------------------------------------
 * Every operator above keeps the camera's geometry.  This family maps a source frame through a coarse MESH of source positions into a destination
 * frame: a lens undistorted, a camera mounted on its side turned upright, a floor plane rectified.  There is no format conversion: BGR to BGR,
 * NV12 to NV12.  It sits in front of the motion update and the forward: decode, warp, motion update, forward, post-passes, preview.  Integers
 * throughout on the device; no atomics; one owner per written byte; the same bytes on every run (tests/warp/warpref.py restates it in numpy).
 *
 * MESH.  A destination frame of dw x dh pixels and a cell of c = 1 << s pixels, c one of 8, 16, 32, 64, have a mesh of
 * mw = (dw - 1) / c + 2 by mh = (dh - 1) / c + 2 points.  Point (ci, cj) is a pair of int32 (x, y): the source position of destination pixel
 * (ci c, cj c) in units of 1 / 256 source pixel (FFGPU_WARP_MESH_ONE); an integer position is the centre of that source pixel.  The mesh lives
 * in DEVICE memory, built once per camera, 8-byte aligned, rows of mw pairs.  Any int32 value is legal: the kernel never reads a byte outside
 * the source frame, whatever the mesh holds.
 *
 * INTERPOLATION.  For destination pixel (i, j): ci = i >> s, a = i & (c - 1), cj = j >> s, b = j & (c - 1); P00, P10, P01, P11 are the points at
 * (ci, cj), (ci + 1, cj), (ci, cj + 1), (ci + 1, cj + 1).  In 64-bit integers, for x and for y alike:
 *     S  = (c - b) * ((c - a) * P00 + a * P10) + b * ((c - a) * P01 + a * P11)
 *     X8 = (S + (1 << (2 s - 1))) >> (2 s)        (the shift is arithmetic)
 *     x5 = (X8 + 4) >> 3                          (in 1 / 32 pixel, FFGPU_WARP_SUB)
 * Neighbouring cells share points, so the map is continuous.
 *
 * SAMPLING.  FFGPU_WARP_BILINEAR: x0 = x5 >> 5, fx = x5 & 31, and likewise for y; the taps are (x0, y0), (x0 + 1, y0), (x0, y0 + 1),
 * (x0 + 1, y0 + 1), and per channel
 *     out = ((32 - fy) * ((32 - fx) * v00 + fx * v10) + fy * ((32 - fx) * v01 + fx * v11) + 512) >> 10.
 * FFGPU_WARP_NEAREST: the one tap ((x5 + 16) >> 5, (y5 + 16) >> 5).  Border FFGPU_WARP_FILL: a tap outside the source frame has the fill
 * colour's channel as its value, so an edge is a blend and a pixel whose taps are all outside is the fill.  Border FFGPU_WARP_CLAMP: each tap
 * coordinate is clamped to 0 .. sw - 1 and 0 .. sh - 1.
 *
 * BGR: the three channels share the position.
 * NV12: the Y plane is sampled as above.  Destination chroma sample (i, j) takes the mesh at luma pixel (2 i, 2 j), which is always inside the
 * mesh; its position in the chroma plane is xc5 = (X8 + 8) >> 4, yc5 likewise; it samples U and V as two channels of a plane of
 * ((sw + 1) / 2) x ((sh + 1) / 2) under the same filter and border.  The fill is Y U V.  `matrix` of the frames is not read; chroma is treated
 * as co-sited, as the NV12 conversion above treats it.
 *
 * What follows from the rule: the identity mesh is a byte copy; the eight orientations permute bytes exactly; an integer translation shifts the
 * frame and fills; a constant plane stays constant under CLAMP; NEAREST writes only source bytes or the fill.  The operator does no area
 * averaging: strong minification aliases, so scale down with the preview operator afterwards.
 * Untouched: row padding, memory round the destination, every source byte, the mesh. */
#define FFGPU_WARP_MESH_ONE   256   /* mesh units per source pixel */
#define FFGPU_WARP_SUB        32    /* sampling positions per source pixel */
#define FFGPU_WARP_BILINEAR   0     /* filter */
#define FFGPU_WARP_NEAREST    1
#define FFGPU_WARP_FILL       0     /* border */
#define FFGPU_WARP_CLAMP      1
#define FFGPU_WARP_MAX_SIDE   8192
#define FFGPU_WARP_MAX_JOBS   4096
#define FFGPU_WARP_LENS_BROWN        0
#define FFGPU_WARP_LENS_EQUIDISTANT  1
typedef struct {
    const int *xy;                 /* mh rows of mw (x, y) pairs, 8-byte aligned; device memory for the operators, host memory for ffgpu_warp_point */
    int mw, mh;                    /* must equal the formula for the job's destination */
    int cell;                      /* 8, 16, 32 or 64 */
    int reserved;                  /* 0 */
} ffgpu_warp_mesh;                 /* 24 bytes: xy 0, mw 8, mh 12, cell 16, reserved 20 */
typedef struct {
    int filter;                    /* FFGPU_WARP_BILINEAR or FFGPU_WARP_NEAREST */
    int border;                    /* FFGPU_WARP_FILL or FFGPU_WARP_CLAMP */
    unsigned char fill[4];         /* B G R 0 or Y U V 0, byte 3 must be 0 */
    int reserved;                  /* 0 */
} ffgpu_warp_spec;                 /* 16 bytes: filter 0, border 4, fill 8, reserved 12 */
typedef struct {
    int model;                     /* FFGPU_WARP_LENS_BROWN or FFGPU_WARP_LENS_EQUIDISTANT */
    int reserved;                  /* 0 */
    double dst[4];                 /* fx fy cx cy of the destination, the ideal pinhole image; fx and fy finite and above 0 */
    double src[4];                 /* fx fy cx cy of the source, the camera as it is */
    double k[4];                   /* radial coefficients k1 .. k4 (BROWN reads k1 .. k3) */
    double p[2];                   /* tangential coefficients p1 p2 (BROWN only) */
} ffgpu_warp_lens;                 /* 120 bytes: model 0, reserved 4, dst 8, src 40, k 72, p 104 */

/* Pure host code, every function below: 0, or -1 with the message in ffgpu_last_error.  The builders write the mh x mw pairs of a mesh into HOST
 * memory `xy` (the caller copies them to the device).  Doubles are evaluated in the order written, without contraction; each coordinate is
 * floor(v * 256 + 0.5) saturated to int32; a non-finite value or a non-positive perspective denominator gives INT32_MIN, which lands outside
 * the frame. */
int ffgpu_warp_spec_check(const ffgpu_warp_spec *spec);
/* out = { mw, mh } for a destination of dst_w x dst_h (1..FFGPU_WARP_MAX_SIDE each) and a cell of 8, 16, 32 or 64 */
int ffgpu_warp_mesh_size(int dst_w, int dst_h, int cell, int out[2]);
/* The eight orientations of a src_w x src_h frame.  orient 0..3 is a clockwise rotation by 0, 90, 180, 270 degrees; orient 4..7 mirrors the
 * source left to right first and then rotates by orient - 4.  out_dst_wh = { dw, dh }: the source's sizes, exchanged for odd orient.  Destination
 * pixel (i, j) is source pixel (x, y), with W = src_w and H = src_h:
 *     0: (i, j)   1: (j, H - 1 - i)   2: (W - 1 - i, H - 1 - j)   3: (W - 1 - j, i)
 *     4: (W - 1 - i, j)   5: (W - 1 - j, H - 1 - i)   6: (i, H - 1 - j)   7: (j, i)
 * The points are exact integers (256 times the formula at (ci c, cj c)).  xy may be NULL to ask for the sizes only.  The inverse of orient 1 is
 * 3 and of 3 is 1; every other orient is its own inverse. */
int ffgpu_warp_mesh_orient(int src_w, int src_h, int orient, int cell, int out_dst_wh[2], int *xy);
/* A homography h[9], row-major, from destination pixel (i, j) to the source position:
 *     x = ((h0 i + h1 j) + h2) / ((h6 i + h7 j) + h8),  y = ((h3 i + h4 j) + h5) / ((h6 i + h7 j) + h8).
 * An affine map is h6 = h7 = 0, h8 = 1.  A denominator that is not above 0 gives INT32_MIN for both coordinates of the point. */
int ffgpu_warp_mesh_homography(int dst_w, int dst_h, int cell, const double h[9], int *xy);
/* A lens: the destination is the ideal pinhole image, the source the camera's.  For the mesh point at destination pixel (i, j):
 *     xn = (i - dst_cx) / dst_fx,  yn = (j - dst_cy) / dst_fy,  r2 = xn xn + yn yn
 * FFGPU_WARP_LENS_BROWN, radial 1 + k1 r^2 + k2 r^4 + k3 r^6 plus tangential p1, p2:
 *     rad = 1 + ((k3 r2 + k2) r2 + k1) r2
 *     xd = xn rad + ((2 p1) (xn yn) + p2 (r2 + (2 xn) xn)),  yd = yn rad + (p1 (r2 + (2 yn) yn) + (2 p2) (xn yn))
 * FFGPU_WARP_LENS_EQUIDISTANT, the fisheye:
 *     r = sqrt(r2),  theta = atan(r),  t2 = theta theta,  theta_d = theta (1 + ((((k4 t2 + k3) t2 + k2) t2 + k1) t2))
 *     scale = theta_d / r, or 1 where r is 0;  xd = xn scale,  yd = yn scale
 * then x = src_fx xd + src_cx, y = src_fy yd + src_cy. */
int ffgpu_warp_mesh_lens(int dst_w, int dst_h, int cell, const ffgpu_warp_lens *lens, int *xy);
/* The interpolation rule for destination pixel (i, j) on a HOST copy of the mesh: out = { X8, Y8 }.  For hit-testing and the tests. */
int ffgpu_warp_point(const ffgpu_warp_mesh *mesh_on_host, int dst_w, int dst_h, int i, int j, int out[2]);
/* out = { the columns and the rows of a workgroup's tile of destination pixels, the bytes of LDS the staged form may fill, the jobs one launch takes } */
int ffgpu_warp_tile(int out[4]);

/* The operators.  srcs, dsts, meshes and spec are HOST arrays, free again on return; job n reads srcs[n] through meshes[n] into the WHOLE of
 * dsts[n] (the const pointers of the destinations are written through); frames are described exactly as the draw operators take them; a pane of a
 * larger surface is a frame descriptor into it, as with the tiles.  A workgroup owns a tile of destination pixels and is the only writer of those
 * bytes.  The tile's taps lie inside the bounding box of the mesh points of the cells the tile touches, plus one pixel; where that box, clipped to
 * the frame, fits the LDS budget, the workgroup loads it once with aligned loads and samples from LDS (staged); where not, every lane loads its taps'
 * bytes from global memory (direct).  The choice is uniform per workgroup and both forms give the same bytes.  BGR frames have both forms; the planes
 * of NV12 frames are always read directly (measured: DESIGN 5.33).  The jobs travel as a by-value table inside a kernel
 * argument, 64 per launch; more jobs are more launches, in order on `stream`.  Enqueued without synchronising; stream order is the only barrier.
 * There is no executor form: the operator reads frames, not records.  A job whose source or destination pixel address (bgr / y) is NULL is
 * skipped; its sizes and its mesh are not looked at.  Rejected before anything is launched, with the job's index: everything the draw operators
 * reject about a frame description, for sources and destinations; NULL arrays or spec; njobs outside 1..FFGPU_WARP_MAX_JOBS; a side above
 * FFGPU_WARP_MAX_SIDE; an unknown filter or border, fill[3] != 0, reserved != 0; a NULL, misaligned or wrongly sized mesh, or a bad cell; a job
 * whose source and destination pixel addresses are equal; two jobs with the same destination pixel address (both indices).  Any other overlap of
 * memory is the caller's responsibility. */
int ffgpu_warp_bgr_dev(const ffgpu_bgr_frame *srcs, const ffgpu_bgr_frame *dsts, const ffgpu_warp_mesh *meshes, int njobs,
                       const ffgpu_warp_spec *spec, void *stream);
int ffgpu_warp_nv12_dev(const ffgpu_nv12_frame *srcs, const ffgpu_nv12_frame *dsts, const ffgpu_warp_mesh *meshes, int njobs,
                        const ffgpu_warp_spec *spec, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FFCNN_AMD_FFCNN_HIP_H */
