// ffgpu_exec.hip -- device executor of the ffcnn forward path + the C-ABI of ffcnn_hip.h.
//
// The reference walks its layer list once per frame, malloc()ing every output
// tensor and free()ing inputs as a per-forward refcount drops to zero
// (ffcnn.c:476-520).  Here the same liveness information is used ONCE, at plan
// time: every tensor of a batch gets a fixed offset in a single HBM arena
// (first-fit over lifetime intervals), the layer list becomes a static list of
// kernel launches, and that list is captured into a HIP graph so a forward is a
// single graph launch.  Plan-time rewrites (all disabled by FFGPU_NO_FUSE and
// by FFGPU_KEEP_ALL):
//   * dropout is a pointer alias (as in ffcnn.c:412-416),
//   * a route with one source is an alias; a multi-source route becomes
//     "concat in place": its sources are allocated inside the route's buffer
//     (a CNHW channel concat is a concatenation of whole blocks),
//   * conv -> [dropout] -> shortcut: the residual add moves into the conv epilogue.
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "ffgpu_dev.hpp"
#include "ffgpu_knobs.hpp"
#include "ffgpu_plan.hpp"
#include "conv.h"

// --------------------------------------------------------------------------
static thread_local char g_err[512] = "";

extern "C" void ffgpu_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    if (knob_set(K_VERBOSE)) fprintf(stderr, "ffgpu: %s\n", g_err);
}

extern "C" const char *ffgpu_last_error(void) { return g_err; }

extern "C" const char *ffgpu_build_info(void)
{
#ifdef FFGPU_DIAG
    return "libffcnn_hip gfx950 (CDNA4) HIP DIAG (lab build: launch-dropping switches compiled in) " __DATE__ " " __TIME__;
#else
    return "libffcnn_hip gfx950 (CDNA4) HIP " __DATE__ " " __TIME__;
#endif
}

extern "C" int ffgpu_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

bool ffgpu_no_device(const char *what)
{
    if (ffgpu_device_count() > 0) return false;
    ffgpu_set_error("%s: no HIP device visible: libffcnn_hip has no CPU fallback", what);
    return true;
}

extern "C" int ffgpu_set_device(int ordinal)
{
    FFGPU_CHECK(hipSetDevice(ordinal));
    return 0;
}

// -------------------------------------------------------------------------- host <-> device transfers
// Rule (round 3): the GPU never reads or writes a page of the CALLER's heap.  A copy from / to pageable
// memory makes the runtime map those pages for the device (hipHostRegister explicitly, a large hipMemcpy implicitly), and mapping
// and unmapping malloc pages that glibc hands out again, trims and re-grows took the process down about once in ten to thirty
// load / plan / run / free sequences ("Memory access fault by GPU ... on address <a heap address>", GPUTEST_r02's abort).  Every
// transfer between caller memory and the device therefore goes through page-locked memory that the HIP runtime itself allocated
// (hipHostMalloc) and this library owns: the input tensor of a NET, an executor's / node's staging buffers, or the process-wide
// bounce buffer below.  Memory handed out by ffgpu_host_alloc is recognised and copied from directly (one DMA).
namespace {
struct PinnedRange { const char *p; size_t bytes; };
std::mutex g_pin_mu;
std::vector<PinnedRange> g_pinned;

bool pinned_ours(const void *ptr, size_t bytes)
{
    const char *c = static_cast<const char *>(ptr);
    std::lock_guard<std::mutex> lk(g_pin_mu);
    for (const PinnedRange &r : g_pinned) if (c >= r.p && c + bytes <= r.p + r.bytes) return true;
    return false;
}

constexpr size_t BOUNCE_BYTES = (size_t)16 << 20;
// one staging buffer (and lock) per DEVICE, allocated on first use and kept for the life of the process: readers / writers of
// different GPUs (the node path, one thread per device in a caller) do not queue behind each other
struct Bounce { std::mutex mu; char *p = nullptr; };
Bounce g_bounces[32];

Bounce &bounce_cur()
{
    int dev = 0;
    (void)hipGetDevice(&dev);
    return g_bounces[(unsigned)dev % 32u];
}

int bounce_ready(Bounce &b)          // (call with b.mu held)
{
    if (b.p) return 0;
    FFGPU_CHECK(hipHostMalloc((void **)&b.p, BOUNCE_BYTES, hipHostMallocPortable));
    return 0;
}
}

// synchronous copies between caller memory and device memory, in chunks through the bounce buffer
static int copy_h2d(void *d_dst, const void *h_src, size_t bytes)
{
    if (bytes == 0) return 0;
    if (pinned_ours(h_src, bytes)) { FFGPU_CHECK(hipMemcpy(d_dst, h_src, bytes, hipMemcpyHostToDevice)); return 0; }
    Bounce &bn = bounce_cur();
    std::lock_guard<std::mutex> lk(bn.mu);
    if (bounce_ready(bn)) return -1;
    char *const g_bounce = bn.p;
    for (size_t off = 0; off < bytes; off += BOUNCE_BYTES) {
        const size_t n = std::min(BOUNCE_BYTES, bytes - off);
        memcpy(g_bounce, static_cast<const char *>(h_src) + off, n);
        FFGPU_CHECK(hipMemcpy(static_cast<char *>(d_dst) + off, g_bounce, n, hipMemcpyHostToDevice));
    }
    return 0;
}

static int copy_d2h(void *h_dst, const void *d_src, size_t bytes)
{
    if (bytes == 0) return 0;
    if (pinned_ours(h_dst, bytes)) { FFGPU_CHECK(hipMemcpy(h_dst, d_src, bytes, hipMemcpyDeviceToHost)); return 0; }
    Bounce &bn = bounce_cur();
    std::lock_guard<std::mutex> lk(bn.mu);
    if (bounce_ready(bn)) return -1;
    char *const g_bounce = bn.p;
    for (size_t off = 0; off < bytes; off += BOUNCE_BYTES) {
        const size_t n = std::min(BOUNCE_BYTES, bytes - off);
        FFGPU_CHECK(hipMemcpy(g_bounce, static_cast<const char *>(d_src) + off, n, hipMemcpyDeviceToHost));
        memcpy(static_cast<char *>(h_dst) + off, g_bounce, n);
    }
    return 0;
}

// --------------------------------------------------------------------------
#define FFGPU_INTERNAL_CHILD 0x40000000   /* executor flag used only inside this file: a half of a split executor */

enum StepKind { S_CONV, S_POOL, S_UPSAMPLE, S_ADD, S_COPY, S_YOLO, S_NMS, S_CLEAR, S_TOCNHW, S_IRB, S_FRONT, S_DWPW, S_STAGE };

struct Step {
    StepKind kind;
    int      layer;          // reference layer index this step belongs to (-1: none)
    int      ltype;          // LAYER_TYPE_* for profiling
    ConvDesc conv;           // S_CONV (in == nullptr: patched to the batch input at launch); S_DWPW: the depthwise layer
    ConvDesc conv2;          // S_DWPW: the pointwise layer behind it
    bool     in_is_input;    // S_CONV / S_POOL / S_UPSAMPLE / S_TOCNHW read the batch input
    bool     b_is_input;     // S_ADD: the `from` side is the batch input
    const float *a, *b;      // generic sources
    float   *out;
    long     n;              // element count (ADD/COPY) or planes
    int      w, h, c, fs, stride, flag;
    YoloHead head;
    IrbDesc  irb;            // S_IRB: fused expand -> depthwise -> project [+ shortcut]
    std::vector<IrbDesc> run; // S_STAGE: the blocks of a run merged into one launch (ffgpu_irb_stage.inc), each with its own plan and packed image
    float   *out2[2];        // S_POOL: further stride-1 max pools of the same tensor merged into this launch (fs2[k] != 0)
    int      fs2[2];
    int      lane;           // 0: main stream, 1: side stream (a detection head that runs beside the rest of the net)
    int     *sp_ctr;         // S_YOLO: the counter of the head's quad list where its input layer runs in the sparse form (sparse_heads), else NULL -- k_yolo zeroes it
};

struct ffgpu_netdev {
    NET   *net = nullptr;
    std::mutex mu;                     // guards execs (executors may be created / destroyed from several threads)
    std::vector<ffgpu_exec *> execs;   // every live executor of this net (they hold packings derived from d_weights)
    double us_acc[LAYER_TYPE_TOTOAL] = {};   // FFCNN_PROFILE=1: device time per layer kind, accumulated over net_forward calls
    float *d_weights = nullptr;
    size_t weight_bytes = 0;
    int    device = 0;
    ffgpu_exec *exec1 = nullptr;
};

// Where a forward's batch comes from: a value the entry points build and hand down (forward_on -> push_params / capture -> issue_*), never executor
// state.  `form` says which form of the first kernel runs and so which graph slot serves the forward; the members beside it are what that form reads:
// frames (IN_F32), bgr / bgr_frame / bgr_pitch (IN_U8), ftab (the two frame-table forms -- and the staged route of those entry points, which is
// IN_F32 with the table beside it: k_nms takes each frame's box scale from it), mean / norm (every u8 form).
struct InputSrc {
    InputForm form;
    const float *frames;
    const unsigned char *bgr; long bgr_frame; int bgr_pitch;
    const FrameDesc *ftab;
    float mean[3], norm[3];
    // the source of the c-th part of a split executor: part_frames frames of part_floats floats in all
    InputSrc slice(int c, int part_frames, size_t part_floats) const
    {
        InputSrc p = *this;
        if (frames) p.frames = frames + c * part_floats;
        if (bgr) p.bgr = bgr + (long)c * part_frames * bgr_frame;
        if (ftab) p.ftab = ftab + (size_t)c * part_frames;
        return p;
    }
};
static InputSrc fp32_src(const float *d_frames) { InputSrc in = {}; in.frames = d_frames; return in; }
static InputSrc u8_src(InputForm form, const float mean[3], const float norm[3])
{
    InputSrc in = {};
    in.form = form;
    for (int k = 0; k < 3; k++) { in.mean[k] = mean[k]; in.norm[k] = norm[k]; }
    return in;
}

struct ffgpu_exec {
    NET *net = nullptr;
    ffgpu_netdev *dev = nullptr;
    int  N = 1, flags = 0, device = 0;
    int  in_c = 0, in_h = 0, in_w = 0;
    std::vector<Step>   steps;
    NetLayout layout;                  // tensors, aliases, lifetimes, side lane and arena offsets (ffgpu_plan.hpp)
    float *arena = nullptr;            // layout.arena_floats floats
    float *d_input = nullptr;          // own staging buffer for host / bgr entry points
    float *d_pack = nullptr;           // packed constants of the fused blocks (derived from the weights)
    int   *d_sparse = nullptr;         // sparse heads (sparse_heads): per head 64 ints with the counter in front (zero between forwards), then the list of P / 4 quads
    BBOX  *d_cand = nullptr;           // cand_cap candidate slots per frame: one per anchor of every head cell
    int   *d_cand_key = nullptr, *d_ncand = nullptr;
    int    cand_cap = 1, bbox_max = 1;
    BBOX  *d_full = nullptr;           // every box that survives NMS, score order, cand_cap slots per frame
    void  *d_nms_scratch = nullptr;    // k_nms work arrays when they do not fit LDS
    ExecParams *d_prm = nullptr;       // device parameter block: input pointer + box scale of the forward being enqueued
    bool   indirect = false;           // every launch that reads the batch input does so through d_prm->frames
    ExecParams prm_sent = {}; hipStream_t prm_stream = nullptr; bool prm_valid = false;      // what d_prm holds (or will, on prm_stream)
    InputSrc last = {};                // input of the last forward (read_layer(-1))
    ffgpu_frame_dets *d_dets = nullptr;
    ffgpu_frame_dets *h_dets = nullptr, *h_dets_dev = nullptr;   // FFGPU_HOST_DETS: pinned mirror and its device address
    // the frame-table entry points: the device table of per-frame descriptors (one entry per frame, what d_prm->frames_tab names during such a
    // forward; a split executor's halves read their parts of their parent's)
    FrameDesc *d_ftab = nullptr;
    std::vector<FrameDesc> ftab_sent; hipStream_t ftab_stream = nullptr;      // what d_ftab holds (or will, on ftab_stream)
    float *h_stage = nullptr;          // ffgpu_exec_forward_host from caller memory: page-locked staging of one batch (on first use)
    // ffgpu_exec_merge_tiles (allocated by the first call): merged records and full lists (picture g's list at cand_cap x mrg_off[g]), the work arrays
    // of unions beyond LDS, and the device tile table with what it holds (or will, on mtab_stream)
    ffgpu_frame_dets *d_merged = nullptr; BBOX *d_merged_full = nullptr; void *d_merge_scratch = nullptr; int *d_mtab = nullptr;
    std::vector<int> mtab_sent, mrg_off; hipStream_t mtab_stream = nullptr;
    ffgpu_frame_dets *ring = nullptr; int ring_slots = 0; int *d_ringctr = nullptr;   // ffgpu_exec_set_ring
    int ring_stride = 0;               // records per ring slot (the parent's batch for the halves of a split executor)
    static constexpr int MAXPART = 8;
    ffgpu_exec *child[MAXPART] = {};   // FFGPU_SPLIT2: part-batch executors that run as parallel graph branches
    int nchild = 0;
    hipStream_t part_stream[MAXPART] = {}; hipEvent_t part_ev[MAXPART] = {};   // branch c >= 1 runs on part_stream[c]
    bool is_child = false;             // records / mirror / ring belong to the parent
    int    s1 = 1, s2 = 1;
    hipStream_t own_stream = nullptr, last_stream = nullptr;
    hipStream_t side_stream = nullptr;              // second graph branch
    hipEvent_t  ev_fork = nullptr, ev_join = nullptr;
    // ONE instantiated graph per input form: the input pointer and the box scale reach the kernels through d_prm, and the forms differ in
    // the first kernel alone.  IN_F32's is captured when the executor is created, a u8 form's on its first use.  Only a
    // net whose first layer has no kernel that reads through the slot (indirect == false: e.g. a pool or a pointwise conv
    // straight on the input) falls back to graphs keyed by the input pointer, least recently used one evicted.
    hipGraphExec_t graph[IN_FORMS] = {};
    struct Keyed { const float *in; hipGraphExec_t g; unsigned long stamp; };
    std::vector<Keyed> graphs;
    unsigned long graph_stamp = 0;
    int captures = 0;                  // graphs captured + instantiated so far (ffgpu_exec_graph_captures)
    int kernel_count = 0;
};

static float *tensor_ptr(const ffgpu_exec *ex, int t) { return ex->arena + ex->layout.offset_of(t); }

// -------------------------------------------------------------------------- planning
// plan() = the layout (ffgpu_plan.hpp: pure host code), the arena, the step list built from the layout, the rewrites of that list, the packed
// constants' places, and whether the captured graph is free of the input pointer.
// the one place the planner's switches are read: the flags, and the environment at every create
// runs of small-plane blocks merge into one launch (ffgpu_irb_stage.inc) only where that launch's one workgroup per frame has company: several chains
// in flight and at least 32 frames each.  A single chain of 64 workgroups on 256 CUs would lose against the per-block launches' two tiles per frame.
static bool stage_wanted(int N, int flags)
{
    return (flags & FFGPU_CONCURRENT) && !(flags & (FFGPU_KEEP_ALL | FFGPU_NO_FUSE)) && N >= 32 && knob(K_IRB_STAGE) != 0;
}

static PlanOptions plan_options(const ffgpu_exec *ex)
{
    PlanOptions o;
    o.batch = ex->N;
    o.keep_all = ex->flags & FFGPU_KEEP_ALL;
    o.fuse = !(ex->flags & FFGPU_NO_FUSE);
    // The head branch is OPT-IN (FFGPU_BRANCH=1).  MEASURED (r01): 2 % faster than the single chain once the head kernels were latency-sized (0.766 vs
    // 0.782 ms per 64-frame batch), slower in an FFGPU_CONCURRENT plan (0.489 vs 0.455 ms: the other chains fill those gaps).  A forked graph runs on
    // internal streams of the runtime (ROCm 7.0), its fragile part (an arena's worth of memory kept per destroyed graph, one
    // SIGSEGV inside hipGraphLaunch in 30 runs of 630 create / launch / destroy cycles): 2 % of ONE chain's latency is not worth a process.  Never
    // inside the halves of a split executor: a fork nested in a forked stream crashes graph capture there.
    o.branch = knob(K_BRANCH) && !ex->is_child;
    o.no_irb = knob(K_NO_IRB); o.irb_min_ec = knob(K_IRB_MIN_EC);
    o.dwpw = knob(K_DWPW);
    o.stage = stage_wanted(ex->N, ex->flags);
    return o;
}

static ConvDesc layer_desc(const ffgpu_exec *ex, int i, int flag_mask = FFGPU_COMPAT_V6)
{
    ConvDesc d{};
    const LAYER &a = ex->net->layer_list[i], &b = ex->net->layer_list[i + 1];
    const int N = ex->N;
    d.N = N; d.iw = a.w; d.ih = a.h; d.ic = a.c; d.ow = b.w; d.oh = b.h; d.oc = b.c;
    d.fs = a.fs; d.stride = a.stride; d.pad = a.pad; d.groups = a.groups; d.act = a.activation;
    d.flags = ex->flags & flag_mask;
    d.in_cs = (long)N * a.w * a.h; d.in_ns = (long)a.w * a.h;
    d.out_cs = (long)N * b.w * b.h; d.out_ns = (long)b.w * b.h;
    return d;
}

// geometry, activations, flags and res_act of the block of layers p0 .. p0 + 2 (the step adds the pointers)
static IrbDesc irb_desc(const ffgpu_exec *ex, int p0)
{
    IrbDesc d{};
    const LAYER *ll = ex->net->layer_list;
    const LAYER &a = ll[p0], &b = ll[p0 + 1], &c = ll[p0 + 2];
    const int sc = ex->layout.fused_into[p0 + 2];
    d.N = ex->N; d.H = a.h; d.W = a.w; d.OH = ll[p0 + 3].h; d.OW = ll[p0 + 3].w;
    d.ic = a.c; d.ec = a.fn; d.oc = c.fn; d.stride = b.stride; d.flags = ex->flags & FFGPU_CONCURRENT;
    d.act1 = a.activation; d.actd = b.activation; d.act2 = c.activation;
    d.res_act = sc >= 0 ? ll[sc].activation : 0;
    return d;
}

// stage 1: the layout.  What the kernels say of a block decides with it; the planned descriptors stay for the step builder (layer p0 + 2 -> its block's).
static int plan_layout(ffgpu_exec *ex, std::vector<IrbDesc> &irb_planned)
{
    const PlanOptions opt = plan_options(ex);
    irb_planned.assign(ex->net->layer_num, IrbDesc{});
    auto block_ok = [&](int p0) {
        IrbDesc d = irb_desc(ex, p0);
        if (!ffgpu_irb_plan(d) || (d.ec < opt.irb_min_ec && d.plan.family != IRB_THIN)) return false;   // thin blocks take the streaming fused kernel
        irb_planned[p0 + 2] = d;
        return true;
    };
    auto pair_ok = [&](int p0) { return ffgpu_dwpw_ok(layer_desc(ex, p0), layer_desc(ex, p0 + 1)); };
    static_assert(FFGPU_STAGE_MAX_BLOCKS == IRBS_MAXB, "the layout's longest run is the stage kernel's");
    auto run_ok = [&](const std::vector<int> &tails) {              // (the blocks' last layers: their planned descriptors are in irb_planned by now)
        std::vector<IrbDesc> run;
        for (int t : tails) run.push_back(irb_planned[t]);
        return ffgpu_irb_stage_ok(run.data(), (int)run.size());
    };
    return ffgpu_net_layout(ex->net->layer_list, ex->net->layer_num, opt, block_ok, pair_ok, run_ok, ex->layout);
}

// stage 2
static int plan_arena(ffgpu_exec *ex)
{
    const size_t bytes = ex->layout.arena_floats * sizeof(float);
    if (hipMalloc(&ex->arena, bytes) != hipSuccess) { ffgpu_set_error("arena hipMalloc(%zu bytes) failed", bytes); return -1; }
    return 0;
}

// stage 3: one pass over the layers, every tensor at arena + offset_of
static int plan_steps(ffgpu_exec *ex, const std::vector<IrbDesc> &irb_planned)
{
    const NetLayout &nl = ex->layout;
    const LAYER *ll = ex->net->layer_list;
    const int L = ex->net->layer_num, N = ex->N;
    std::vector<Step> &S = ex->steps;
    S.clear();
    { Step c{}; c.kind = S_CLEAR; c.layer = -1; c.ltype = LAYER_TYPE_YOLO; S.push_back(c); }
    int key_base = 0;
    float *cnhw_input = nullptr;     // set when the first layer cannot read the frame-major input directly
    bool bad_chain = false;
    auto ptr = [&](int t) { return tensor_ptr(ex, t); };
    auto weights = [&](int i) { return ex->dev->d_weights + (ll[i].filter - ex->net->weight_buf); };
    auto in_ptr = [&](int i, bool *is_input) -> const float * {
        const int t = nl.src(i - 1);
        *is_input = t == -1;
        if (t < -1) bad_chain = true;            // e.g. a conv chained directly behind a yolo head
        return t >= 0 ? ptr(t) : nullptr;
    };
    for (int i = 0; i < L; i++) {
        const LAYER &a = ll[i];
        Step st{};
        st.layer = i; st.ltype = a.type;
        bool from_input = false;
        switch (a.type) {
        case LAYER_TYPE_CONV: {
            if (nl.canon[i] == -3) break;                           // expanded tensors of a fused block; blocks inside a merged run
            if (nl.stage_first[i] >= 0) {                           // the last block of a merged run: the run's one launch
                st.kind = S_STAGE;
                for (int t = nl.stage_first[i] + 2; t <= i; t++) {
                    if (nl.irb_tail[t] < 0) continue;
                    IrbDesc d = irb_planned[t];
                    d.w1 = weights(nl.irb_tail[t]); d.wd = weights(nl.irb_tail[t] + 1); d.w2 = weights(nl.irb_tail[t] + 2);
                    st.run.push_back(d);
                }
                st.run.front().in = ptr(nl.src(nl.stage_first[i] - 1));
                st.run.back().out = ptr(nl.canon[i]);
            } else if (nl.irb_tail[i] >= 0) {
                const int p0 = nl.irb_tail[i];
                IrbDesc &d = st.irb = irb_planned[i];
                st.kind = S_IRB;
                d.in = ptr(nl.src(p0 - 1));
                d.out = ptr(nl.canon[i]);
                d.w1 = weights(p0); d.wd = weights(p0 + 1); d.w2 = weights(p0 + 2);
                if (nl.fused_into[i] >= 0) d.residual = ptr(nl.src(ll[nl.fused_into[i]].depend_list[0]));
            } else if (nl.dwpw_tail[i] >= 0) {                      // depthwise (p0) + this pointwise layer: one launch
                const int p0 = nl.dwpw_tail[i];
                st.kind = S_DWPW;
                st.conv = layer_desc(ex, p0); st.conv2 = layer_desc(ex, i);
                st.conv.in = ptr(nl.src(p0 - 1));
                st.conv.filt = weights(p0); st.conv2.filt = weights(i);
                st.conv2.out = ptr(nl.canon[i]);
            } else {
                ConvDesc &d = st.conv = layer_desc(ex, i, FFGPU_COMPAT_V6 | FFGPU_BF16_PW);
                st.kind = S_CONV;
                d.in = in_ptr(i, &st.in_is_input);
                d.filt = weights(i);
                d.out = ptr(nl.canon[i]);
                if (st.in_is_input) { d.in_cs = (long)a.w * a.h; d.in_ns = (long)a.c * a.w * a.h; }     // frame-major batch input
                if (nl.fused_into[i] >= 0) {
                    const LAYER &sc = ll[nl.fused_into[i]];
                    d.residual = ptr(nl.src(sc.depend_list[0]));
                    d.res_act = sc.activation; d.res_cs = d.out_cs; d.res_ns = d.out_ns;
                }
            }
            S.push_back(st);
            break; }
        case LAYER_TYPE_AVGPOOL: case LAYER_TYPE_MAXPOOL: case LAYER_TYPE_UPSAMPLE: case LAYER_TYPE_SHORTCUT: {
            if (nl.canon[i] == -3) break;                           // a shortcut inside a merged run: added on chip
            if (a.type == LAYER_TYPE_SHORTCUT && i > 0 && nl.canon[i - 1] == i) break;     // absorbed by the producing conv (the last of a merged run: its other side has no tensor)
            const float *src = in_ptr(i, &from_input);
            // a shortcut whose OTHER side is the net input (from = a dropout in front of every other layer)
            const bool b_input = a.type == LAYER_TYPE_SHORTCUT && nl.src(a.depend_list[0]) == -1;
            if (a.type == LAYER_TYPE_SHORTCUT && nl.src(a.depend_list[0]) < -1) { bad_chain = true; break; }
            if ((from_input || b_input) && N > 1) {          // needs CNHW order: convert the input once
                if (!cnhw_input) {
                    const LAYER &l0 = ll[0];
                    if (hipMalloc(&cnhw_input, (size_t)l0.w * l0.h * l0.c * N * sizeof(float)) != hipSuccess) { ffgpu_set_error("hipMalloc failed"); return -1; }
                    Step cv{}; cv.kind = S_TOCNHW; cv.layer = -1; cv.ltype = a.type; cv.out = cnhw_input; cv.c = l0.c; cv.w = l0.w; cv.h = l0.h; cv.in_is_input = true;
                    S.push_back(cv);
                }
                if (from_input) { src = cnhw_input; from_input = false; }
            }
            st.in_is_input = from_input;
            st.a = src;
            if (a.type == LAYER_TYPE_SHORTCUT) {
                st.kind = S_ADD;
                st.b = b_input ? cnhw_input : ptr(nl.src(a.depend_list[0]));      // (batch 1: patched to the frames at launch)
                st.b_is_input = b_input && N == 1;
                st.out = ptr(nl.canon[i]);
                st.n = (long)ll[i + 1].w * ll[i + 1].h * ll[i + 1].c * N; st.flag = a.activation;
            } else {
                st.kind = a.type == LAYER_TYPE_UPSAMPLE ? S_UPSAMPLE : S_POOL;
                st.out = ptr(nl.canon[i]);
                st.c = a.c; st.w = a.w; st.h = a.h; st.fs = a.fs; st.stride = a.stride;
                st.flag = a.type == LAYER_TYPE_MAXPOOL;
            }
            S.push_back(st);
            break; }
        case LAYER_TYPE_ROUTE: {
            if (nl.canon[i] != i || nl.route_inplace[i]) break;     // alias / concat in place
            long off = 0;
            for (int k = 0; k < a.depend_num; k++) {
                const int t = nl.src(a.depend_list[k]);
                if (t < 0) { ffgpu_set_error("route %d: unsupported source", i); return -1; }
                const LAYER &o = ll[a.depend_list[k] + 1];
                Step cp{}; cp.kind = S_COPY; cp.layer = i; cp.ltype = a.type;
                cp.a = ptr(t); cp.out = ptr(i) + off; cp.n = (long)o.w * o.h * o.c * N;
                S.push_back(cp);
                off += cp.n;
            }
            break; }
        case LAYER_TYPE_YOLO: {
            st.kind = S_YOLO;
            YoloHead &hd = st.head;
            hd.in = in_ptr(i, &from_input);
            if (from_input) { ffgpu_set_error("yolo head directly on the input is not supported"); return -1; }
            hd.w = a.w; hd.h = a.h; hd.classes = a.class_num;
            memcpy(hd.anchors, a.anchor_list, sizeof hd.anchors);
            hd.thresh = a.ignore_thres; hd.scale_xy = a.scale_x_y; hd.key_base = key_base;
            key_base += a.w * a.h * 3;
            S.push_back(st);
            break; }
        default: break;                                             // dropout
        }
    }
    if (bad_chain) { ffgpu_set_error("a layer consumes the (non-existent) output of a yolo head"); return -1; }
    return 0;
}

// stage 4: the rewrites of the step list
// first layer + the thin block behind it -> one streaming kernel (ffgpu_front.inc): the 8-channel tensor between them
// is never written (its arena space stays reserved; read_layer refuses it like the inside of a fused block)
static void fuse_front(ffgpu_exec *ex)
{
    std::vector<Step> &S = ex->steps;
    for (size_t k = 0; k + 1 < S.size(); k++) {
        Step &c0 = S[k];
        const Step &b0 = S[k + 1];
        if (c0.kind != S_CONV || b0.kind != S_IRB || c0.layer < 0 || ex->layout.nuses[c0.layer] != 1) continue;
        if (!ffgpu_front_ok(c0.conv, b0.irb)) continue;
        c0.kind = S_FRONT; c0.irb = b0.irb;
        ex->layout.readable[c0.layer] = 0;
        S.erase(S.begin() + k + 1);
        break;
    }
}

// stride-1 max pools of one tensor that follow each other (the routes between them are aliases: an SPP block) become one launch
static void merge_spp(std::vector<Step> &S)
{
    for (size_t i = 0; i + 1 < S.size(); i++) {
        Step &a = S[i];
        if (a.kind != S_POOL || !a.flag || a.stride != 1 || a.in_is_input || (long)a.w * a.h > 8192) continue;
        int k = 0;
        while (k < 2 && i + 1 < S.size()) {
            const Step &b = S[i + 1];
            if (b.kind != S_POOL || !b.flag || b.stride != 1 || b.in_is_input || b.a != a.a || b.c != a.c || b.w != a.w || b.h != a.h) break;
            a.out2[k] = b.out; a.fs2[k] = b.fs; k++;
            S.erase(S.begin() + i + 1);
        }
    }
}

// The pointwise layer in front of a yolo head computes 3 (5 + classes) channels for every cell and k_yolo reads the class scores of the few (cell, anchor)
// whose objectness can pass.  Where that layer runs on k_conv_x3's pointwise form and the head is its only reader, its launch becomes the SPARSE form
// (ffgpu_conv_x3.inc): box rows everywhere, class rows on the listed quads.  The layer stays planned as it was (kernel, MT, the regular image); its tensor
// is no longer whole, so read_layer and hash_layers refuse it like the inside of a fused block.  Same rule as k_irb_stage: FFGPU_CONCURRENT executors only (a single chain
// measured 0.8 % slower with the form: the second launch costs it more than the class rows did, profiles/sparse_head_ab.txt), never under FFGPU_KEEP_ALL /
// FFGPU_NO_FUSE; FFGPU_SPARSE_HEAD=0: never.  Every head of every executor (each half of a split one) has its own list and counter.
static bool sparse_head_wanted(int flags) { return (flags & FFGPU_CONCURRENT) && !(flags & (FFGPU_KEEP_ALL | FFGPU_NO_FUSE)) && knob(K_SPARSE_HEAD) != 0; }

static void sparse_heads(ffgpu_exec *ex)
{
    if (!sparse_head_wanted(ex->flags)) return;
    std::vector<Step> &S = ex->steps;
    for (Step &y : S) {
        if (y.kind != S_YOLO) continue;
        for (Step &c : S) {
            // the layer straight in front of the head, its own tensor, the head its only reader
            if (c.kind != S_CONV || c.layer < 0 || c.layer != y.layer - 1 || ex->layout.canon[c.layer] != c.layer || ex->layout.nuses[c.layer] != 1 ||
                c.in_is_input || c.conv.out != y.head.in) continue;
            if (!ffgpu_conv_sparse_head_ok(c.conv, y.head.classes)) continue;
            c.conv.sp_classes = y.head.classes; c.conv.sp_thresh = y.head.thresh;
            ex->layout.readable[c.layer] = 0;
        }
    }
}

// the lists and counters of the steps sparse_heads marked (zeroed once: k_yolo leaves every counter at zero behind a forward)
static int place_sparse(ffgpu_exec *ex)
{
    size_t tot = 0;
    for (const Step &st : ex->steps) if (st.kind == S_CONV && st.conv.sp_classes) tot += 64 + (size_t)st.conv.N * st.conv.oh * st.conv.ow / 4;
    if (!tot) return 0;
    if (hipMalloc(&ex->d_sparse, tot * sizeof(int)) != hipSuccess || hipMemsetAsync(ex->d_sparse, 0, tot * sizeof(int), ex->own_stream) != hipSuccess) { ffgpu_set_error("hipMalloc(sparse heads) failed"); return -1; }
    size_t off = 0;
    for (Step &st : ex->steps) {
        if (st.kind != S_CONV || !st.conv.sp_classes) continue;
        st.conv.sp_ctr = ex->d_sparse + off; st.conv.sp_list = ex->d_sparse + off + 64;
        for (Step &y : ex->steps) if (y.kind == S_YOLO && y.layer - 1 == st.layer) y.sp_ctr = st.conv.sp_ctr;
        off += 64 + (size_t)st.conv.N * st.conv.oh * st.conv.ow / 4;
    }
    return 0;
}

static void rewrite_steps(ffgpu_exec *ex)
{
    std::vector<Step> &S = ex->steps;
    const bool fuse = !(ex->flags & FFGPU_NO_FUSE);
    if (fuse) { fuse_front(ex); merge_spp(S); }
    // with a detection head in the net no clear launch is needed: k_nms zeroes the candidate counters it has consumed
    // (they start zeroed) and the first head counts the forward for the record ring
    const auto head = std::find_if(S.begin(), S.end(), [](const Step &t) { return t.kind == S_YOLO; });
    if (head != S.end() && fuse) {
        head->flag = 1;
        S.erase(std::remove_if(S.begin(), S.end(), [](const Step &t) { return t.kind == S_CLEAR; }), S.end());
    }
    { Step nm{}; nm.kind = S_NMS; nm.layer = -1; nm.ltype = LAYER_TYPE_YOLO; S.push_back(nm); }
    sparse_heads(ex);
    const NetLayout &nl = ex->layout;
    for (Step &st : S) st.lane = (nl.side_lo >= 0 && st.layer >= nl.side_lo && st.layer <= nl.side_hi) ? 1 : 0;
}

// stage 5: kernel choice frozen with the plan, and the constants of the fused blocks and packed pointwise layers placed in one image (repack fills it)
static size_t pack_floats(const Step &st)
{
    if (st.kind == S_IRB) return ffgpu_irb_pack_floats(st.irb);
    if (st.kind == S_STAGE) { size_t n = 0; for (const IrbDesc &d : st.run) n += ffgpu_irb_pack_floats(d); return n; }
    if (st.kind == S_DWPW) return ffgpu_dwpw_pack_floats(st.conv, st.conv2);
    if (st.kind == S_CONV) return ffgpu_pw_pack_floats(st.conv);
    return 0;
}

static int place_constants(ffgpu_exec *ex)
{
    size_t tot = 0;
    for (Step &st : ex->steps) {
        if (st.kind == S_CONV) {                              // kernel choice, split-K and k_conv_x3's MT
            if (st.in_is_input) st.conv.flags |= FFGPU_F_BATCH_INPUT;
            ffgpu_conv_plan(st.conv);
        }
        tot += pack_floats(st);
    }
    if (!tot) return 0;
    if (hipMalloc(&ex->d_pack, tot * sizeof(float)) != hipSuccess) { ffgpu_set_error("hipMalloc(pack) failed"); return -1; }
    size_t off = 0;
    for (Step &st : ex->steps) {
        const size_t n = pack_floats(st);
        if (st.kind == S_IRB) st.irb.pk = ex->d_pack + off;
        else if (st.kind == S_STAGE) { size_t o = off; for (IrbDesc &d : st.run) { d.pk = ex->d_pack + o; o += ffgpu_irb_pack_floats(d); } }
        else if (st.kind == S_DWPW) st.conv2.wpack = ex->d_pack + off;
        else if (st.kind == S_CONV && n) st.conv.wpack = ex->d_pack + off;
        off += n;
    }
    return 0;
}

// stage 6: launches that read the batch input take its address from the parameter block when their kernel can (the first conv
// of every darknet cfg: dense KxK from 3 channels): the captured graph is then independent of the input buffer
static void decide_indirect(ffgpu_exec *ex)
{
    ex->indirect = !knob(K_NO_INDIRECT);             // tests: the keyed fallback
    for (const Step &st : ex->steps)
        if (st.b_is_input || (st.in_is_input && !(st.kind == S_FRONT || (st.kind == S_CONV && ffgpu_conv_supports_ind(st.conv))))) ex->indirect = false;
    if (ex->indirect)
        for (Step &st : ex->steps) if (st.in_is_input) st.conv.in_ind = reinterpret_cast<const float *const *>(ex->d_prm);   // &d_prm->frames
}

static int plan(ffgpu_exec *ex)
{
    std::vector<IrbDesc> irb_planned;
    if (plan_layout(ex, irb_planned) || plan_arena(ex) || plan_steps(ex, irb_planned)) return -1;
    rewrite_steps(ex);
    if (place_constants(ex) || place_sparse(ex)) return -1;
    decide_indirect(ex);
    ex->kernel_count = (int)ex->steps.size();
    for (const Step &st : ex->steps) if (st.kind == S_CONV && st.conv.sp_list) ex->kernel_count++;      // (a sparse head's step is two launches)
    return 0;
}

static int repack(ffgpu_exec *ex, hipStream_t s)
{
    for (const Step &st : ex->steps) {
        if (st.kind == S_IRB && ffgpu_irb_pack(st.irb, const_cast<float *>(st.irb.pk), s)) return -1;
        if (st.kind == S_STAGE) for (const IrbDesc &d : st.run) if (ffgpu_irb_pack(d, const_cast<float *>(d.pk), s)) return -1;
        if (st.kind == S_DWPW && ffgpu_dwpw_pack(st.conv, st.conv2, const_cast<float *>(st.conv2.wpack), s)) return -1;
        if (st.kind == S_CONV && st.conv.wpack && ffgpu_pw_pack(st.conv, const_cast<float *>(st.conv.wpack), s)) return -1;
    }
    return 0;
}

// -------------------------------------------------------------------------- running
static int issue_step(ffgpu_exec *ex, const Step &st, const InputSrc &in, hipStream_t s)
{
    const float *const d_frames = in.frames;
#ifdef FFGPU_DIAG
    // tuning only (tools/ablate_layers.py): FFGPU_DBG_SKIP="lo:hi" drops the launches of layers lo..hi -- wrong results,
    // but the change in frames/s is what that stretch of the net costs with several batches in flight
    // (FFGPU_DBG_KEEP="lo:hi" is the complement: only that stretch runs -- tools/saturate_layers.py)
    if (knob_text(K_DBG_SKIP) || knob_text(K_DBG_KEEP)) {
        static bool warned = false;
        if (!warned) { warned = true; fprintf(stderr, "libffcnn_hip: FFGPU_DBG_SKIP / FFGPU_DBG_KEEP set -- launches are being dropped, RESULTS ARE WRONG (tuning only)\n"); }
    }
    if (const char *sk = knob_text(K_DBG_SKIP)) {
        int lo = -1, hi = -1;
        if (sscanf(sk, "%d:%d", &lo, &hi) == 2 && st.layer >= lo && st.layer <= hi && st.kind != S_NMS) return 0;
    }
    if (const char *sk = knob_text(K_DBG_KEEP)) {
        int lo = -1, hi = -1;
        if (sscanf(sk, "%d:%d", &lo, &hi) == 2 && (st.layer < lo || st.layer > hi) && st.kind != S_NMS) return 0;
    }
#endif
    switch (st.kind) {
    case S_CLEAR:
        return ffgpu_launch_clear(ex->d_ncand, ex->N, ex->d_ringctr, s);
    case S_CONV: {
        ConvDesc d = st.conv;
        if (st.in_is_input && !d.in_ind) d.in = d_frames;
        return ffgpu_launch_conv(d, FFGPU_K_AUTO, s); }
    case S_POOL:
        if (st.fs2[0]) {
            float *const outs[3] = { st.out, st.out2[0], st.out2[1] };
            const int fss[3] = { st.fs, st.fs2[0], st.fs2[1] };
            return ffgpu_launch_spp(st.a, outs, fss, st.fs2[1] ? 3 : 2, (long)ex->N * st.c, st.w, st.h, s);
        }
        return ffgpu_launch_pool(st.in_is_input ? d_frames : st.a, st.out, ex->N, st.c, st.w, st.h, st.fs, st.stride, st.flag, s);
    case S_UPSAMPLE:
        return ffgpu_launch_upsample(st.in_is_input ? d_frames : st.a, st.out, (long)ex->N * st.c, st.w, st.h, st.stride, s);
    case S_ADD:
        return ffgpu_launch_add_act(st.in_is_input ? d_frames : st.a, st.b_is_input ? d_frames : st.b, st.out, st.n, st.flag, s);
    case S_COPY:
        return ffgpu_launch_copy(st.a, st.out, st.n, s);
    case S_TOCNHW: {
        // frame-major -> CNHW: a 1x1 "identity" regrouping expressed as strided plane copies
        const long plane = (long)st.w * st.h;
        for (int c = 0; c < st.c; c++)
            FFGPU_CHECK(hipMemcpy2DAsync(st.out + (long)c * ex->N * plane, plane * sizeof(float),
                                         d_frames + (long)c * plane, (size_t)st.c * plane * sizeof(float),
                                         plane * sizeof(float), ex->N, hipMemcpyDeviceToDevice, s));
        return 0; }
    case S_IRB:
        return ffgpu_launch_irb(st.irb, s);
    case S_STAGE:
        return ffgpu_launch_irb_stage(st.run.data(), (int)st.run.size(), s);
    case S_DWPW:
        return ffgpu_launch_dwpw(st.conv, st.conv2, st.conv2.wpack, s);
    case S_FRONT: {
        ConvDesc d = st.conv;
        if (st.in_is_input && !d.in_ind) d.in = d_frames;
        return ffgpu_launch_front(d, st.irb, in.form, s); }
    case S_YOLO:
        return ffgpu_launch_yolo(st.head, ex->N, ex->in_w, ex->in_h, ex->d_cand, ex->d_cand_key, ex->d_ncand, ex->cand_cap,
                                 st.flag ? ex->d_ringctr : nullptr, st.sp_ctr, s);          // forwards are counted whether or not a ring is attached
    case S_NMS:
        return ffgpu_launch_nms(ex->d_cand, ex->d_cand_key, ex->d_ncand, ex->cand_cap, ex->d_full, ex->d_nms_scratch,
                                ex->d_dets, ex->h_dets_dev, ex->d_ringctr, ex->N, 0.5f, 1, ex->d_prm, s);
    }
    return -1;
}

static int issue_all(ffgpu_exec *ex, const InputSrc &in, hipStream_t s)
{
    bool forked = false, joined = true;
    for (const Step &st : ex->steps) {
        if (st.lane == 1) {
            // (the branch's stream exists only in plans that have one: every stream takes a share of the device's four hardware queues)
            if (!ex->side_stream) FFGPU_CHECK(hipStreamCreateWithFlags(&ex->side_stream, hipStreamNonBlocking));
            if (!forked) {                                   // fork: the side branch starts where the main one is now
                FFGPU_CHECK(hipEventRecord(ex->ev_fork, s));
                FFGPU_CHECK(hipStreamWaitEvent(ex->side_stream, ex->ev_fork, 0));
                forked = true; joined = false;
            }
            if (issue_step(ex, st, in, ex->side_stream) != 0) return -1;
            continue;
        }
        if (st.kind == S_NMS && !joined) {                   // join before the candidates are consumed
            FFGPU_CHECK(hipEventRecord(ex->ev_join, ex->side_stream));
            FFGPU_CHECK(hipStreamWaitEvent(s, ex->ev_join, 0));
            joined = true;
        }
        if (issue_step(ex, st, in, s) != 0) return -1;
    }
    if (!joined) {
        FFGPU_CHECK(hipEventRecord(ex->ev_join, ex->side_stream));
        FFGPU_CHECK(hipStreamWaitEvent(s, ex->ev_join, 0));
    }
    return 0;
}

// FFGPU_SPLIT2: the two halves of the batch are two independent chains of the same 40-odd launches; issued on two
// streams they become two parallel branches of one graph.  Most of the launches are bound by a wave's serial chain and
// a few microseconds of launch / first-load latency, not by a pipe: the second chain fills those gaps.
static int issue_split(ffgpu_exec *ex, const InputSrc &in, hipStream_t s)
{
    const int pn = ex->child[0]->N;
    const size_t part = (size_t)pn * ex->in_c * ex->in_h * ex->in_w;
    FFGPU_CHECK(hipEventRecord(ex->ev_fork, s));
    for (int c = 1; c < ex->nchild; c++) FFGPU_CHECK(hipStreamWaitEvent(ex->part_stream[c], ex->ev_fork, 0));
    for (int c = 0; c < ex->nchild; c++)
        if (issue_all(ex->child[c], in.slice(c, pn, part), c ? ex->part_stream[c] : s) != 0) return -1;
    for (int c = 1; c < ex->nchild; c++) {
        FFGPU_CHECK(hipEventRecord(ex->part_ev[c], ex->part_stream[c]));
        FFGPU_CHECK(hipStreamWaitEvent(s, ex->part_ev[c], 0));
    }
    return 0;
}

// the parameter block of this forward, written in stream order in front of the launches that read it; skipped when the
// block already holds (or, on the same stream, will hold by then) the same values
static int push_params(ffgpu_exec *ex, const InputSrc &in, hipStream_t s)
{
    if (ex->child[0]) {
        const int pn = ex->child[0]->N;
        const size_t part = (size_t)pn * ex->in_c * ex->in_h * ex->in_w;
        for (int c = 0; c < ex->nchild; c++) {
            ffgpu_exec *ch = ex->child[c];
            ch->s1 = ex->s1; ch->s2 = ex->s2; ch->bbox_max = ex->bbox_max; ch->last_stream = s;
            if (push_params(ch, in.slice(c, pn, part), s)) return -1;      // (each half reads its own half of the frames / the table)
        }
        return 0;
    }
    ex->last = in;
    ExecParams v;
    memset(&v, 0, sizeof v);
    v.frames = in.frames; v.s1 = ex->s1; v.s2 = ex->s2;
    v.bgr = in.bgr; v.bgr_frame = in.bgr_frame; v.bgr_pitch = in.bgr_pitch;
    for (int k = 0; k < 3; k++) { v.mean[k] = in.mean[k]; v.norm[k] = in.norm[k]; }
    v.frames_tab = in.ftab;
    v.bbox_max = ex->bbox_max;
    v.ring = ex->ring; v.ring_slots = ex->ring_slots; v.ring_stride = ex->ring_stride ? ex->ring_stride : ex->N;
    if (ex->prm_valid && ex->prm_stream == s && memcmp(&v, &ex->prm_sent, sizeof v) == 0) return 0;
    if (ffgpu_launch_set_params(ex->d_prm, v, s)) return -1;
    ex->prm_sent = v; ex->prm_stream = s; ex->prm_valid = true;
    return 0;
}

static bool graph_pointer_free(const ffgpu_exec *ex)
{
    if (!ex->child[0]) return ex->indirect;
    for (int c = 0; c < ex->nchild; c++) if (!ex->child[c]->indirect) return false;
    return true;
}

static int capture(ffgpu_exec *ex, const InputSrc &in, hipGraphExec_t *out)
{
    hipGraph_t graph = nullptr;
    hipGraphExec_t gexec = nullptr;
    // capture on the executor's own stream (a user stream may be the legacy
    // null stream, which cannot be captured); replay goes to the caller's stream
    hipStream_t cs = ex->own_stream;
    FFGPU_CHECK(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
    const int rc = ex->child[0] ? issue_split(ex, in, cs) : issue_all(ex, in, cs);
    hipError_t e = hipStreamEndCapture(cs, &graph);
    if (rc != 0) { if (graph) (void)hipGraphDestroy(graph); return -1; }
    if (e != hipSuccess) { ffgpu_set_error("hipStreamEndCapture: %s", hipGetErrorString(e)); return -1; }
    e = hipGraphInstantiate(&gexec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) { ffgpu_set_error("hipGraphInstantiate: %s", hipGetErrorString(e)); return -1; }
    ex->captures++;
    *out = gexec;
    return 0;
}

static void drop_graphs(ffgpu_exec *ex)                       // caller has synchronised the streams the graphs ran on
{
    for (hipGraphExec_t &g : ex->graph) if (g) { (void)hipGraphExecDestroy(g); g = nullptr; }
    for (auto &g : ex->graphs) (void)hipGraphExecDestroy(g.g);
    ex->graphs.clear();
}

// The launch list is captured into its graph when the executor is created (the input pointer travels through the parameter
// block, so no buffer has to be known).  That is a saving, not what keeps launches and packed constants together: plan() freezes
// every kernel choice, tile split and image layout that the FFGPU_* tuning switches influence into the steps themselves
// (ConvDesc::kernel / nsplit / x3_mt, IrbDesc::plan), and every later issue of a step -- the graphs captured on first use of a
// u8 form or per input pointer, eager FFGPU_NO_GRAPH forwards, ffgpu_exec_profile and _profile_steps, the repack of
// ffgpu_net_weights_commit -- reads them, never the environment.
static int capture_at_create(ffgpu_exec *ex)
{
    if ((ex->flags & FFGPU_NO_GRAPH) || !graph_pointer_free(ex)) return 0;
    return capture(ex, fp32_src(nullptr), &ex->graph[IN_F32]);
}

static int forward_on(ffgpu_exec *ex, const InputSrc &in, hipStream_t s)
{
    const float *const d_frames = in.frames;
    ex->last_stream = s;
    if (push_params(ex, in, s)) return -1;
    if (ex->flags & FFGPU_NO_GRAPH) return ex->child[0] ? issue_split(ex, in, s) : issue_all(ex, in, s);
    if (graph_pointer_free(ex)) {                            // the usual case: the form's graph, whatever the input buffer / scale
        hipGraphExec_t &g1 = ex->graph[in.form];
        if (!g1 && capture(ex, in, &g1)) return -1;
        FFGPU_CHECK(hipGraphLaunch(g1, s));
        return 0;
    }
    // fallback (the first layer's kernel cannot read through the parameter block): graphs keyed by the input pointer
    ffgpu_exec::Keyed *hit = nullptr;
    for (auto &g : ex->graphs) if (g.in == d_frames) hit = &g;
    if (!hit) {
        if (ex->graphs.size() >= 8) {                        // evict the least recently used one -- after its last launch ended
            size_t lru = 0;
            for (size_t i = 1; i < ex->graphs.size(); i++) if (ex->graphs[i].stamp < ex->graphs[lru].stamp) lru = i;
            FFGPU_CHECK(hipDeviceSynchronize());             // (it may have run on another stream than this call's)
            (void)hipGraphExecDestroy(ex->graphs[lru].g);
            ex->graphs.erase(ex->graphs.begin() + lru);
        }
        hipGraphExec_t g = nullptr;
        if (capture(ex, in, &g)) return -1;
        ex->graphs.push_back({ d_frames, g, 0 });
        hit = &ex->graphs.back();
    }
    hit->stamp = ++ex->graph_stamp;
    FFGPU_CHECK(hipGraphLaunch(hit->g, s));
    return 0;
}

// -------------------------------------------------------------------------- C-ABI: executor
// an executor whose NET was freed first (net_free orphans it) keeps its device buffers until ffgpu_exec_destroy, but its
// layer table and weights are gone: every entry point that would touch them fails instead
static bool alive(const ffgpu_exec *ex, const char *what)
{
    if (!ex) { ffgpu_set_error("%s: NULL executor", what); return false; }
    if (!ex->dev) { ffgpu_set_error("%s: the NET of this executor has been freed (destroy executors before net_free)", what); return false; }
    return true;
}

// "is there an executor", for the entry points that can be the first call of a process: without one, the missing device is the better message
static bool exec_ok(const ffgpu_exec *ex, const char *what)
{
    if (!ex && ffgpu_no_device(what)) return false;
    return alive(ex, what);
}

static ffgpu_netdev *netdev_of(NET *net)
{
    if (!net) { ffgpu_set_error("NULL net"); return nullptr; }
    ffcnn_ext *ext = ffcnn_ext_of(net);
    if (!ext || !ext->dev) { ffgpu_set_error("net was not created by this library's net_load"); return nullptr; }
    return (ffgpu_netdev *)ext->dev;
}

static ffgpu_exec *exec_create_on(ffgpu_netdev *dev, NET *net, int batch, int flags);
extern "C" ffgpu_exec *ffgpu_exec_create(NET *net, int batch, int flags)
{
    ffgpu_netdev *dev = netdev_of(net);
    if (!dev) return nullptr;
    return exec_create_on(dev, net, batch, flags);
}

// (an executor lives on ONE device: that of the ffgpu_netdev -- the device copy of the weights -- it is planned on; a
//  multi-GPU node holds one netdev + executor per device, ffgpu_node.inc)
static ffgpu_exec *exec_create_on(ffgpu_netdev *dev, NET *net, int batch, int flags)
{
    if (batch < 1) { ffgpu_set_error("batch must be >= 1"); return nullptr; }
    if (hipSetDevice(dev->device) != hipSuccess) { ffgpu_set_error("hipSetDevice failed"); return nullptr; }
    if (knob(K_COMPAT_V6)) flags |= FFGPU_COMPAT_V6;
    if (knob(K_NO_GRAPH)) flags |= FFGPU_NO_GRAPH;
    if (knob(K_BF16_PW)) flags |= FFGPU_BF16_PW;
    if (knob(K_NO_FUSE)) flags |= FFGPU_NO_FUSE;
    const bool split = (flags & FFGPU_SPLIT2) && batch >= 2 && batch % 2 == 0 && !(flags & FFGPU_KEEP_ALL);
    const bool as_child = (flags & FFGPU_INTERNAL_CHILD) != 0;
    flags &= ~(FFGPU_SPLIT2 | FFGPU_INTERNAL_CHILD);
    ffgpu_exec *ex = new ffgpu_exec();
    ex->net = net; ex->dev = dev; ex->device = dev->device; ex->N = batch; ex->flags = flags; ex->is_child = as_child;
    ex->in_c = net->layer_list[0].c; ex->in_h = net->layer_list[0].h; ex->in_w = net->layer_list[0].w;
    // candidate slots per frame: one per anchor of every head cell, so the decode can never overflow; the reference's own
    // cap (bbox_max candidates in emission order, ffcnn.c:243,463) is applied by k_nms
    long slots = 0;
    for (int i = 0; i < net->layer_num; i++)
        if (net->layer_list[i].type == LAYER_TYPE_YOLO) slots += 3L * net->layer_list[i].w * net->layer_list[i].h;
    if (slots > (1L << 24) || slots * batch > (1L << 28)) { ffgpu_set_error("executor: %ld candidate slots per frame x %d frames is too many", slots, batch); delete ex; return nullptr; }
    ex->cand_cap = (int)std::max(slots, 1L);
    ex->bbox_max = std::max(net->bbox_max, 1);
    int cap_p2 = 1;
    while (cap_p2 < ex->cand_cap) cap_p2 <<= 1;
    const size_t ncs = (size_t)ex->cand_cap * (size_t)batch;
    bool ok = hipStreamCreateWithFlags(&ex->own_stream, hipStreamNonBlocking) == hipSuccess
           && hipEventCreateWithFlags(&ex->ev_fork, hipEventDisableTiming) == hipSuccess
           && hipEventCreateWithFlags(&ex->ev_join, hipEventDisableTiming) == hipSuccess
           && hipMalloc(&ex->d_cand, sizeof(BBOX) * ncs) == hipSuccess
           && hipMalloc(&ex->d_cand_key, sizeof(int) * ncs) == hipSuccess
           && hipMalloc(&ex->d_full, sizeof(BBOX) * ncs) == hipSuccess
           && hipMalloc(&ex->d_prm, sizeof(ExecParams)) == hipSuccess && hipMemset(ex->d_prm, 0, sizeof(ExecParams)) == hipSuccess
           && (ffgpu_nms_in_lds(cap_p2) || hipMalloc(&ex->d_nms_scratch, (size_t)13 * cap_p2 * batch) == hipSuccess)
           && hipMalloc(&ex->d_ncand, sizeof(int) * (size_t)batch) == hipSuccess && hipMemset(ex->d_ncand, 0, sizeof(int) * (size_t)batch) == hipSuccess
           && hipMalloc(&ex->d_dets, sizeof(ffgpu_frame_dets) * (size_t)batch) == hipSuccess
           && hipMalloc(&ex->d_ringctr, sizeof(int)) == hipSuccess && hipMemset(ex->d_ringctr, 0, sizeof(int)) == hipSuccess
           && hipMemset(ex->d_dets, 0, sizeof(ffgpu_frame_dets) * (size_t)batch) == hipSuccess
           // hipMemset of device memory is asynchronous on the NULL stream, and every stream this executor works on is
           // non-blocking (not ordered with it): wait here, or a late memset may clear counters a forward has begun to use
           && hipStreamSynchronize(nullptr) == hipSuccess;
    if (ok && (flags & FFGPU_HOST_DETS)) {
        ok = hipHostMalloc(&ex->h_dets, sizeof(ffgpu_frame_dets) * (size_t)batch, hipHostMallocMapped) == hipSuccess
          && hipHostGetDevicePointer((void **)&ex->h_dets_dev, ex->h_dets, 0) == hipSuccess;
        if (ok) memset(ex->h_dets, 0, sizeof(ffgpu_frame_dets) * (size_t)batch);
    }
    if (!ok) { ffgpu_set_error("executor buffers: %s", hipGetErrorString(hipGetLastError())); ffgpu_exec_destroy(ex); return nullptr; }
    ex->last_stream = ex->own_stream;
    if (split) {
        // the parent owns the records (and their mirror / ring); each part plans its own arena and writes its slice
        int K = 2;
        const int parts = knob(K_SPLIT_PARTS);                   // tuning: 2 (default), 4 or 8 parallel chains
        if ((parts == 4 || parts == 8) && batch % parts == 0) K = parts;
        for (int c = 0; c < K; c++) {
            ffgpu_exec *ch = exec_create_on(dev, net, batch / K, (flags & ~FFGPU_HOST_DETS) | FFGPU_INTERNAL_CHILD);
            if (!ch) { ffgpu_exec_destroy(ex); return nullptr; }
            (void)hipFree(ch->d_dets); (void)hipFree(ch->d_full);
            ch->d_dets = ex->d_dets + (size_t)c * (batch / K);
            ch->d_full = ex->d_full + (size_t)c * (batch / K) * ex->cand_cap;
            ch->h_dets_dev = ex->h_dets_dev ? ex->h_dets_dev + (size_t)c * (batch / K) : nullptr;
            ex->child[c] = ch; ex->nchild = c + 1;
            ex->kernel_count += ch->kernel_count;
            ex->layout.arena_floats += ch->layout.arena_floats;
            if (c && (hipStreamCreateWithFlags(&ex->part_stream[c], hipStreamNonBlocking) != hipSuccess ||
                      hipEventCreateWithFlags(&ex->part_ev[c], hipEventDisableTiming) != hipSuccess)) {
                ffgpu_set_error("split executor: stream / event creation failed"); ffgpu_exec_destroy(ex); return nullptr; }
        }
        { std::lock_guard<std::mutex> lk(dev->mu); dev->execs.push_back(ex); }
        if (capture_at_create(ex)) { ffgpu_exec_destroy(ex); return nullptr; }
        return ex;
    }
    if (plan(ex) != 0 || repack(ex, ex->own_stream) != 0 || hipStreamSynchronize(ex->own_stream) != hipSuccess) { ffgpu_exec_destroy(ex); return nullptr; }
    { std::lock_guard<std::mutex> lk(dev->mu); dev->execs.push_back(ex); }
    if (!as_child && capture_at_create(ex)) { ffgpu_exec_destroy(ex); return nullptr; }
    return ex;
}

extern "C" void ffgpu_exec_destroy(ffgpu_exec *ex)
{
    if (!ex) return;
    int cur_dev = ex->device;
    (void)hipGetDevice(&cur_dev);
    if (cur_dev != ex->device) (void)hipSetDevice(ex->device);      // (a node's executors live on other devices than the caller's)
    if (ex->last_stream) (void)hipStreamSynchronize(ex->last_stream);
    // a graph with a forked branch (the head branch) keeps ~its arena's worth of device memory if its exec is destroyed after
    // a sync of the launch stream alone (ROCm 7.0; tools/leak_check.py: +27 MB per create / forward / destroy cycle) --
    // a device-wide sync first lets the runtime retire the branch's internal streams
    if (!ex->is_child) (void)hipDeviceSynchronize();
    for (int c = 0; c < ffgpu_exec::MAXPART; c++) {
        if (ex->child[c]) { ffgpu_exec_destroy(ex->child[c]); ex->child[c] = nullptr; }
        if (ex->part_stream[c]) (void)hipStreamDestroy(ex->part_stream[c]);
        if (ex->part_ev[c]) (void)hipEventDestroy(ex->part_ev[c]);
    }
    if (ex->is_child) { ex->d_dets = nullptr; ex->d_full = nullptr; }      // slices of the parent's buffers
    if (ex->dev) {
        std::lock_guard<std::mutex> lk(ex->dev->mu);
        ex->dev->execs.erase(std::remove(ex->dev->execs.begin(), ex->dev->execs.end(), ex), ex->dev->execs.end());
    }
    drop_graphs(ex);
    for (const Step &st : ex->steps) if (st.kind == S_TOCNHW) (void)hipFree(st.out);
    (void)hipFree(ex->arena); (void)hipFree(ex->d_input); (void)hipFree(ex->d_pack); (void)hipFree(ex->d_sparse); (void)hipFree(ex->d_cand);
    (void)hipFree(ex->d_cand_key); (void)hipFree(ex->d_ncand); (void)hipFree(ex->d_dets);
    (void)hipFree(ex->d_full); (void)hipFree(ex->d_prm); (void)hipFree(ex->d_nms_scratch); (void)hipFree(ex->d_ftab);
    (void)hipFree(ex->d_merged); (void)hipFree(ex->d_merged_full); (void)hipFree(ex->d_merge_scratch); (void)hipFree(ex->d_mtab);
    if (ex->h_dets) (void)hipHostFree(ex->h_dets);
    if (ex->h_stage) (void)hipHostFree(ex->h_stage);
    (void)hipFree(ex->d_ringctr);
    if (ex->own_stream) (void)hipStreamDestroy(ex->own_stream);
    if (ex->side_stream) (void)hipStreamDestroy(ex->side_stream);
    if (ex->ev_fork) (void)hipEventDestroy(ex->ev_fork);
    if (ex->ev_join) (void)hipEventDestroy(ex->ev_join);
    if (cur_dev != ex->device) (void)hipSetDevice(cur_dev);
    delete ex;
}

extern "C" int ffgpu_exec_batch(const ffgpu_exec *ex) { return ex ? ex->N : 0; }
extern "C" size_t ffgpu_exec_arena_bytes(const ffgpu_exec *ex) { return ex ? ex->layout.arena_floats * sizeof(float) : 0; }
extern "C" int ffgpu_exec_kernel_count(const ffgpu_exec *ex) { return ex ? ex->kernel_count : 0; }

// What one forward of this plan MUST move and compute: per launch the tensors it reads and writes once each (input,
// output, residual, filter rows; nothing for the tensors a fused launch keeps on chip), summed over the launch list; and
// 2 x multiply-adds of every conv layer of the net (fused or not).  bench.py prices the measured time per batch against
// these two numbers (HBM peak, fp32 matrix peak).
// what one step of the plan must move between HBM and the chip, as a model: its input tensor(s) + output tensor + filter rows, each once
static double step_model_bytes(const ffgpu_exec *ex, const Step &st)
{
    const double N = ex->N;
    auto rows = [](const ConvDesc &d) { return (double)d.oc * (conv_k4(d) + 4); };
    switch (st.kind) {
    case S_CONV: { const ConvDesc &d = st.conv;
        return 4.0 * (N * d.ic * d.ih * d.iw + N * d.oc * d.oh * d.ow * (d.residual ? 2 : 1) + rows(d)); }
    case S_IRB: { const IrbDesc &d = st.irb;
        return 4.0 * (N * d.ic * d.H * d.W + N * d.oc * d.OH * d.OW * (d.residual ? 2 : 1) + (double)d.ec * (d.ic + 4 + 16) + (double)d.oc * (d.ec + 4)); }
    case S_STAGE: { const IrbDesc &d = st.run.front();           // the frame in, the frame out, every block's filter rows; nothing in between leaves the chip
        return 4.0 * (N * d.ic * d.H * d.W + N * d.oc * d.OH * d.OW + (double)st.run.size() * ((double)d.ec * (d.ic + 4 + 16) + (double)d.oc * (d.ec + 4))); }
    case S_DWPW: { const ConvDesc &a = st.conv, &b = st.conv2;
        return 4.0 * (N * a.ic * a.ih * a.iw + N * b.oc * b.oh * b.ow + rows(a) + rows(b)); }
    case S_FRONT: { const ConvDesc &c = st.conv; const IrbDesc &d = st.irb;
        return 4.0 * (N * c.ic * c.ih * c.iw + N * d.oc * d.OH * d.OW + rows(c)); }
    case S_POOL: { const int np = 1 + (st.fs2[0] != 0) + (st.fs2[1] != 0);
        return 4.0 * N * st.c * ((double)st.w * st.h + (double)np * (st.w / st.stride) * (st.h / st.stride)); }
    case S_UPSAMPLE: return 4.0 * N * st.c * (double)st.w * st.h * (1 + st.stride * st.stride);
    case S_ADD: return 4.0 * 3 * st.n;
    case S_COPY: return 4.0 * 2 * st.n;
    case S_TOCNHW: return 4.0 * 2 * N * st.c * (double)st.w * st.h;
    case S_YOLO: return 4.0 * N * 3 * (5 + st.head.classes) * (double)st.head.w * st.head.h;
    default: return 0.0;
    }
}

/* the same model step by step (tools/net_traffic.py sets the counters of a rocprofv3 --pmc pass beside it): layer_of[i] / hbm_bytes[i] of step i */
extern "C" int ffgpu_exec_step_model(const ffgpu_exec *ex, int *layer_of, double *hbm_bytes, int cap)
{
    if (!ex || !ex->net || !layer_of || !hbm_bytes) { ffgpu_set_error("step_model: bad argument"); return -1; }
    if (ex->child[0]) { ffgpu_set_error("step_model: not available on a split executor"); return -1; }
    const int n = (int)std::min<size_t>(ex->steps.size(), (size_t)(cap > 0 ? cap : 0));
    for (int i = 0; i < n; i++) { layer_of[i] = ex->steps[i].layer; hbm_bytes[i] = step_model_bytes(ex, ex->steps[i]); }
    return n;
}

extern "C" int ffgpu_exec_work_model(const ffgpu_exec *ex, double *hbm_bytes, double *flops)
{
    if (!ex || !ex->net) { ffgpu_set_error("work_model: bad executor"); return -1; }
    double by = 0, fl = 0;
    if (ex->child[0]) {
        for (int c = 0; c < ex->nchild; c++) {
            double b1 = 0, f1 = 0;
            if (ffgpu_exec_work_model(ex->child[c], &b1, &f1)) return -1;
            by += b1; fl += f1;
        }
    } else {
        const double N = ex->N;
        for (const Step &st : ex->steps) by += step_model_bytes(ex, st);
        const LAYER *ll = ex->net->layer_list;
        for (int i = 0; i < ex->net->layer_num; i++)
            if (ll[i].type == LAYER_TYPE_CONV)
                fl += 2.0 * N * ll[i].fs * ll[i].fs * (ll[i].c / ll[i].groups) * (double)ll[i + 1].c * ll[i + 1].w * ll[i + 1].h;
    }
    if (hbm_bytes) *hbm_bytes = by;
    if (flops) *flops = fl;
    return 0;
}

extern "C" int ffgpu_exec_set_scale(ffgpu_exec *ex, int s1, int s2)
{
    if (!ex || s2 == 0) { ffgpu_set_error("set_scale: bad arguments"); return -1; }
    ex->s1 = s1; ex->s2 = s2;
    return 0;
}

extern "C" int ffgpu_exec_forward_dev(ffgpu_exec *ex, const float *d_frames, void *stream)
{
    if (!alive(ex, "forward_dev")) return -1;
    if (!d_frames) { ffgpu_set_error("forward_dev: NULL argument"); return -1; }
    return forward_on(ex, fp32_src(d_frames), stream ? (hipStream_t)stream : ex->own_stream);
}

static int ensure_input(ffgpu_exec *ex)
{
    if (ex->d_input) return 0;
    FFGPU_CHECK(hipMalloc(&ex->d_input, sizeof(float) * (size_t)ex->N * ex->in_c * ex->in_h * ex->in_w));
    return 0;
}

extern "C" int ffgpu_exec_forward_host(ffgpu_exec *ex, const float *h_frames)
{
    if (!alive(ex, "forward_host")) return -1;
    if (!h_frames) { ffgpu_set_error("forward_host: NULL argument"); return -1; }
    if (ensure_input(ex)) return -1;
    const size_t bytes = sizeof(float) * (size_t)ex->N * ex->in_c * ex->in_h * ex->in_w;
    if (pinned_ours(h_frames, bytes)) {                          // (a NET's input tensor: one DMA, in stream order with the forward)
        FFGPU_CHECK(hipMemcpyAsync(ex->d_input, h_frames, bytes, hipMemcpyHostToDevice, ex->own_stream));
    } else {
        // caller memory: through the executor's own page-locked staging buffer (allocated on the first such call)
        if (!ex->h_stage) FFGPU_CHECK(hipHostMalloc((void **)&ex->h_stage, bytes, hipHostMallocDefault));
        memcpy(ex->h_stage, h_frames, bytes);                    // (the previous forward_host of this executor ended with a stream sync)
        FFGPU_CHECK(hipMemcpyAsync(ex->d_input, ex->h_stage, bytes, hipMemcpyHostToDevice, ex->own_stream));
    }
    if (forward_on(ex, fp32_src(ex->d_input), ex->own_stream)) return -1;
    FFGPU_CHECK(hipStreamSynchronize(ex->own_stream));
    return 0;
}

// the plan's first launch is k_front reading through the parameter block (every leaf of a split executor alike) -- and, for the
// resizing forms, that kernel has three columns per lane (ffgpu_front_nc)
static bool front_fused(const ffgpu_exec *ex, bool resizing)
{
    if (ex->child[0]) {
        for (int c = 0; c < ex->nchild; c++) if (!front_fused(ex->child[c], resizing)) return false;
        return true;
    }
    for (const Step &st : ex->steps)
        if (st.in_is_input) return st.kind == S_FRONT && st.conv.in_ind != nullptr && ex->indirect && (!resizing || ffgpu_front_nc(st.irb) == 3);
    return false;
}

// this forward may use the u8 form `form` of the first kernel: no fp32 batch in between.  FFGPU_NO_U8_FRONT (tuning / tests): always the two-kernel path
static bool front_takes(const ffgpu_exec *ex, InputForm form)
{
    return !knob_set(K_NO_U8_FRONT) && front_fused(ex, form != IN_U8) && (form != IN_NV12_FRAMES || ffgpu_front_nv12_fused());
}

extern "C" int ffgpu_exec_forward_bgr_dev(ffgpu_exec *ex, const unsigned char *d_bgr, int w, int h,
                                          const float mean[3], const float norm[3], void *stream)
{
    if (!alive(ex, "forward_bgr_dev")) return -1;
    if (!d_bgr || w <= 0 || h <= 0 || ex->in_c != 3) { ffgpu_set_error("forward_bgr_dev: bad arguments"); return -1; }
    hipStream_t s = stream ? (hipStream_t)stream : ex->own_stream;
    const int W = ex->in_w, H = ex->in_h;
    int sw, sh;
    letterbox(w, h, W, H, &sw, &sh, &ex->s1, &ex->s2);
    if (w == W && h == H && (reinterpret_cast<uintptr_t>(d_bgr) & 3) == 0 && front_takes(ex, IN_U8)) {
        // no resize (net_input copies pixel for pixel): the first kernel converts the bytes itself
        InputSrc in = u8_src(IN_U8, mean, norm);
        in.bgr = d_bgr; in.bgr_pitch = (w * 3 + 3) & ~3; in.bgr_frame = (long)in.bgr_pitch * h;
        return forward_on(ex, in, s);
    }
    if (ensure_input(ex)) return -1;
    if (ffgpu_launch_input_bgr(d_bgr, ex->d_input, ex->N, w, h, W, H, sw, sh, ex->s1, ex->s2, mean, norm, s)) return -1;
    return forward_on(ex, fp32_src(ex->d_input), s);
}

// The two frame-table entry points.  Per frame net_input's letterbox arithmetic on the host; the table written in stream order in front of the
// forward -- skipped when it holds these values already; a BGR table and an NV12 one never compare equal (FrameDesc::fmt, uv) -- then either the
// resizing k_front reads the bytes itself (plans that start with it) or k_input4 writes the fp32 batch the ordinary graph consumes.  The
// executor's own scale stays as it was: k_nms takes each frame's s1 / s2 from the table.
static bool frames_args_ok(ffgpu_exec *ex, const char *what, const void *frames, int nframes, const float *mean, const float *norm)
{
    if (!exec_ok(ex, what)) return false;
    if (!frames || !mean || !norm) { ffgpu_set_error("%s: NULL argument", what); return false; }
    if (nframes != ex->N) { ffgpu_set_error("%s: %d frames for an executor of batch %d", what, nframes, ex->N); return false; }
    if (ex->in_c != 3) { ffgpu_set_error("%s: the net's input has %d channels, not 3", what, ex->in_c); return false; }
    return true;
}

static int forward_frames(ffgpu_exec *ex, const std::vector<FrameDesc> &tab, InputForm form, const float mean[3], const float norm[3], hipStream_t s)
{
    if (!ex->d_ftab) FFGPU_CHECK(hipMalloc(&ex->d_ftab, sizeof(FrameDesc) * (size_t)ex->N));
    if (!(ex->ftab_stream == s && ex->ftab_sent.size() == tab.size() && memcmp(ex->ftab_sent.data(), tab.data(), sizeof(FrameDesc) * tab.size()) == 0)) {
        ex->ftab_sent.clear();
        if (ffgpu_launch_set_frames(ex->d_ftab, tab.data(), (int)tab.size(), s)) return -1;
        ex->ftab_sent = tab; ex->ftab_stream = s;
    }
    InputSrc in = u8_src(form, mean, norm);
    if (!front_takes(ex, form)) {                                    // staged: the fp32 batch, then the ordinary graph
        if (ensure_input(ex) || ffgpu_launch_input_frames(ex->d_ftab, form == IN_NV12_FRAMES, ex->d_input, ex->N, ex->in_w, ex->in_h, mean, norm, s)) return -1;
        in = fp32_src(ex->d_input);
    }
    in.ftab = ex->d_ftab;
    return forward_on(ex, in, s);
}

// the caller's descriptors checked (role FRAME_FORWARD) into the table, each with its letterbox
template <class Frame>
static int forward_frames_dev(ffgpu_exec *ex, const char *what, InputForm form, const Frame *frames, int nframes, const float mean[3], const float norm[3], void *stream)
{
    if (!frames_args_ok(ex, what, frames, nframes, mean, norm)) return -1;
    std::vector<FrameDesc> tab;
    if (ffgpu_frame_table(what, FRAME_FORWARD, frames, nframes, tab)) return -1;
    for (FrameDesc &d : tab) letterbox(d.w, d.h, ex->in_w, ex->in_h, &d.sw, &d.sh, &d.s1, &d.s2);
    return forward_frames(ex, tab, form, mean, norm, stream ? (hipStream_t)stream : ex->own_stream);
}

extern "C" int ffgpu_exec_forward_bgr_frames_dev(ffgpu_exec *ex, const ffgpu_bgr_frame *frames, int nframes,
                                                 const float mean[3], const float norm[3], void *stream)
{
    return forward_frames_dev(ex, "forward_bgr_frames_dev", IN_BGR_FRAMES, frames, nframes, mean, norm, stream);
}

// NV12 frames: the same table with the second plane, its pitch and the matrix (FrameDesc::fmt != 0); the pixel is converted where it is sampled
extern "C" int ffgpu_exec_forward_nv12_frames_dev(ffgpu_exec *ex, const ffgpu_nv12_frame *frames, int nframes,
                                                  const float mean[3], const float norm[3], void *stream)
{
    return forward_frames_dev(ex, "forward_nv12_frames_dev", IN_NV12_FRAMES, frames, nframes, mean, norm, stream);
}

extern "C" int ffgpu_exec_dets_dev(ffgpu_exec *ex, void **dev_ptr, size_t *bytes)
{
    if (!ex) { ffgpu_set_error("NULL executor"); return -1; }
    if (dev_ptr) *dev_ptr = ex->d_dets;
    if (bytes) *bytes = sizeof(ffgpu_frame_dets) * (size_t)ex->N;
    return 0;
}

extern "C" int ffgpu_exec_set_ring_strided(ffgpu_exec *ex, void *dev_ring, int slots, int slot_records)
{
    if (!ex || (dev_ring && (slots < 1 || slot_records < ex->N))) { ffgpu_set_error("set_ring: bad arguments"); return -1; }
    FFGPU_CHECK(hipStreamSynchronize(ex->last_stream));          // (the ring travels in the parameter block: the graph stays)
    ex->ring = (ffgpu_frame_dets *)dev_ring; ex->ring_slots = dev_ring ? slots : 0; ex->ring_stride = slot_records;
    FFGPU_CHECK(hipMemset(ex->d_ringctr, 0, sizeof(int)));
    for (int c = 0; c < ex->nchild; c++) {                      // each part writes its slice of every slot
        ffgpu_exec *ch = ex->child[c];
        ch->ring = dev_ring ? ex->ring + (size_t)c * ch->N : nullptr; ch->ring_slots = ex->ring_slots; ch->ring_stride = slot_records;
        FFGPU_CHECK(hipMemset(ch->d_ringctr, 0, sizeof(int)));
    }
    FFGPU_CHECK(hipStreamSynchronize(nullptr));                  // (the memsets above run on the NULL stream; forwards do not)
    return 0;
}

extern "C" int ffgpu_exec_set_ring(ffgpu_exec *ex, void *dev_ring, int slots)
{
    if (!ex) { ffgpu_set_error("set_ring: NULL executor"); return -1; }
    return ffgpu_exec_set_ring_strided(ex, dev_ring, slots, ex->N);
}

extern "C" const ffgpu_frame_dets *ffgpu_exec_dets_host(ffgpu_exec *ex)
{
    if (!ex) { ffgpu_set_error("NULL executor"); return nullptr; }
    if (!ex->h_dets) ffgpu_set_error("executor was not created with FFGPU_HOST_DETS");
    return ex->h_dets;
}

extern "C" int ffgpu_exec_read_dets(ffgpu_exec *ex, ffgpu_frame_dets *host_out, int max_frames)
{
    if (!ex || !host_out) { ffgpu_set_error("read_dets: NULL argument"); return -1; }
    const int n = std::max(0, std::min(max_frames, ex->N));
    FFGPU_CHECK(hipStreamSynchronize(ex->last_stream));
    if (ex->h_dets) memcpy(host_out, ex->h_dets, sizeof(ffgpu_frame_dets) * (size_t)n);
    else { if (copy_d2h(host_out, ex->d_dets, sizeof(ffgpu_frame_dets) * (size_t)n)) return -1; }
    return n;
}

extern "C" int ffgpu_exec_cand_capacity(const ffgpu_exec *ex) { return ex ? ex->cand_cap : 0; }
extern "C" int ffgpu_exec_graph_captures(const ffgpu_exec *ex)
{
    if (!ex) return 0;
    int n = ex->captures;
    for (int c = 0; c < ex->nchild; c++) n += ex->child[c]->captures;
    return n;
}

extern "C" int ffgpu_exec_read_boxes(ffgpu_exec *ex, int frame, BBOX *host_out, int cap)
{
    if (!ex || frame < 0 || frame >= ex->N || cap < 0 || (cap > 0 && !host_out)) { ffgpu_set_error("read_boxes: bad arguments"); return -1; }
    FFGPU_CHECK(hipStreamSynchronize(ex->last_stream));
    int nfull = 0;
    if (copy_d2h(&nfull, &ex->d_dets[frame].nfull, sizeof(int))) return -1;
    const int n = std::min(nfull, cap);
    if (n > 0 && copy_d2h(host_out, ex->d_full + (size_t)frame * ex->cand_cap, sizeof(BBOX) * (size_t)n)) return -1;
    return nfull;
}

// -------------------------------------------------------------------------- tiled detection (include/ffcnn_hip.h; kernel: ffgpu_merge.inc)
// A post-pass behind the forward on the forward's stream: reads the records and full lists k_nms left (a split executor's parent owns both), writes
// buffers of its own.  The table is uploaded in front of the merge unless the device table holds (or will hold, on this stream) these values already.
extern "C" int ffgpu_exec_merge_tiles(ffgpu_exec *ex, const ffgpu_tile *tiles, int ntiles, int nimages, void *stream)
{
    if (!exec_ok(ex, "merge_tiles")) return -1;
    if (!tiles) { ffgpu_set_error("merge_tiles: NULL tile table"); return -1; }
    if (ntiles != ex->N) { ffgpu_set_error("merge_tiles: %d tiles for an executor of batch %d", ntiles, ex->N); return -1; }
    const hipStream_t s = stream ? (hipStream_t)stream : ex->own_stream;
    if (s != ex->last_stream) { ffgpu_set_error("merge_tiles: the merge must be enqueued on the stream of the forward it follows"); return -1; }
    std::vector<int> tab, off;
    if (ffgpu_merge_build_tab("merge_tiles", tiles, ntiles, nimages, tab, &off)) return -1;
    if (!ex->d_merged) {
        const size_t n = (size_t)ex->N, cap = (size_t)ex->cand_cap;
        const size_t work = ffgpu_merge_tiles_scratch_bytes(ex->N, ex->cand_cap) - ffgpu_merge_tab_bytes(ex->N);
        if (hipMalloc(&ex->d_merged_full, sizeof(BBOX) * cap * n) != hipSuccess || hipMalloc(&ex->d_merge_scratch, work) != hipSuccess ||
            hipMalloc(&ex->d_mtab, ffgpu_merge_tab_bytes(ex->N)) != hipSuccess || hipMalloc(&ex->d_merged, sizeof(ffgpu_frame_dets) * n) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(ex->d_merged_full); (void)hipFree(ex->d_merge_scratch); (void)hipFree(ex->d_mtab);
            ex->d_merged_full = nullptr; ex->d_merge_scratch = nullptr; ex->d_mtab = nullptr; ex->d_merged = nullptr;
            ffgpu_set_error("merge_tiles: out of device memory for the merge buffers");
            return -1;
        }
    }
    if (!(ex->mtab_stream == s && ex->mtab_sent == tab)) {
        ex->mtab_sent.clear();
        if (ffgpu_launch_set_ints(ex->d_mtab, tab.data(), (int)tab.size(), s)) return -1;
        ex->mtab_sent = tab; ex->mtab_stream = s;
    }
    ex->mrg_off = off;
    return ffgpu_launch_merge_tiles(ex->d_mtab, tab, ex->d_dets, ex->d_full, ex->cand_cap, 0.5f, 1, ex->d_merged, ex->d_merged_full, ex->d_merge_scratch, s);
}

static bool merged_ok(const ffgpu_exec *ex, const char *what)
{
    if (!ex) { ffgpu_set_error("%s: NULL executor", what); return false; }
    if (!ex->d_merged || ex->mrg_off.empty()) { ffgpu_set_error("%s: no ffgpu_exec_merge_tiles has run on this executor", what); return false; }
    return true;
}

extern "C" int ffgpu_exec_merged_dev(ffgpu_exec *ex, void **dev_ptr, size_t *bytes)
{
    if (!merged_ok(ex, "merged_dev")) return -1;
    if (dev_ptr) *dev_ptr = ex->d_merged;
    if (bytes) *bytes = sizeof(ffgpu_frame_dets) * (ex->mrg_off.size() - 1);
    return 0;
}

extern "C" int ffgpu_exec_read_merged(ffgpu_exec *ex, ffgpu_frame_dets *host_out, int max_images)
{
    if (!merged_ok(ex, "read_merged")) return -1;
    if (!host_out) { ffgpu_set_error("read_merged: NULL argument"); return -1; }
    const int n = std::max(0, std::min(max_images, (int)ex->mrg_off.size() - 1));
    FFGPU_CHECK(hipStreamSynchronize(ex->last_stream));
    if (n > 0 && copy_d2h(host_out, ex->d_merged, sizeof(ffgpu_frame_dets) * (size_t)n)) return -1;
    return n;
}

extern "C" int ffgpu_exec_read_merged_boxes(ffgpu_exec *ex, int image, BBOX *host_out, int cap)
{
    if (!merged_ok(ex, "read_merged_boxes")) return -1;
    if (image < 0 || image >= (int)ex->mrg_off.size() - 1 || cap < 0 || (cap > 0 && !host_out)) { ffgpu_set_error("read_merged_boxes: bad arguments"); return -1; }
    FFGPU_CHECK(hipStreamSynchronize(ex->last_stream));
    int nfull = 0;
    if (copy_d2h(&nfull, &ex->d_merged[image].nfull, sizeof(int))) return -1;
    const int n = std::min(nfull, cap);
    if (n > 0 && copy_d2h(host_out, ex->d_merged_full + (size_t)ex->cand_cap * ex->mrg_off[image], sizeof(BBOX) * (size_t)n)) return -1;
    return nfull;
}

// -------------------------------------------------------------------------- post-passes that read the boxes: draw, crop, track, relabel, redact
// What the five post-passes that read boxes share: `which` as the executor's records and lists (ffgpu_source_exec) and the stream, which must be the
// one the forward or merge ran on.  src.stride, the kernels' clamp of a list's length, comes from src.longest by the family's rule: where nothing is
// pitched by it, a list too long for the kernel's int is clamped; where it is also the pitch of ids, rows or the caller's output lists, a list above 2^24
// boxes is refused.
enum StrideRule { STRIDE_CLAMPED, STRIDE_REFUSED };
static int exec_source(ffgpu_exec *ex, const char *what, const char *family, const char *noun, StrideRule rule, int which, int ntargets, void *stream, DetSource &src,
                       hipStream_t *s)
{
    if (ffgpu_source_exec(what, family, which, ntargets, ex->N, ex->cand_cap, ex->d_merged ? &ex->mrg_off : nullptr, src)) return -1;
    *s = stream ? (hipStream_t)stream : ex->own_stream;
    if (*s != ex->last_stream) { ffgpu_set_error("%s: the %s must be enqueued on the stream of the forward or merge it follows", what, noun); return -1; }
    src.recs = which ? ex->d_merged : ex->d_dets;
    src.lists = which ? ex->d_merged_full : ex->d_full;
    if (rule == STRIDE_REFUSED && src.longest > (1 << 24)) { ffgpu_set_error("%s: lists of up to %lld boxes are too long", what, src.longest); return -1; }
    src.stride = (int)std::min(src.longest, (long long)0x7fffffff);
    return 0;
}

// -------------------------------------------------------------------------- the detections drawn into the frames (include/ffcnn_hip.h; kernel: ffgpu_draw.inc)
// A post-pass like the merge, on the stream of the forward or merge it follows: reads the records and full lists (per entry, or the merged ones),
// writes the caller's frames and nothing of the executor's.
template <class Frame>
static int exec_draw(ffgpu_exec *ex, const char *what, int which, const Frame *targets, int ntargets, const ffgpu_draw_style *style, void *stream)
{
    if (!exec_ok(ex, what)) return -1;
    if (!targets) { ffgpu_set_error("%s: NULL targets", what); return -1; }
    unsigned pal[256];
    int npal = 0;
    if (ffgpu_draw_style_check(what, style, pal, &npal)) return -1;
    DetSource src;
    hipStream_t s;
    if (exec_source(ex, what, "DRAW", "draw", STRIDE_CLAMPED, which, ntargets, stream, src, &s)) return -1;
    std::vector<DrawTarget> tab;
    if (ffgpu_frame_table(what, FRAME_DRAW, targets, ntargets, tab)) return -1;
    return ffgpu_launch_draw(std::is_same<Frame, ffgpu_nv12_frame>::value, src, tab, pal, npal, style->thickness, s);
}

extern "C" int ffgpu_exec_draw_bgr(ffgpu_exec *ex, int which, const ffgpu_bgr_frame *targets, int ntargets, const ffgpu_draw_style *style, void *stream)
{
    return exec_draw(ex, "draw_bgr", which, targets, ntargets, style, stream);
}

extern "C" int ffgpu_exec_draw_nv12(ffgpu_exec *ex, int which, const ffgpu_nv12_frame *targets, int ntargets, const ffgpu_draw_style *style, void *stream)
{
    return exec_draw(ex, "draw_nv12", which, targets, ntargets, style, stream);
}

// -------------------------------------------------------------------------- the detections redacted in the frames (include/ffcnn_hip.h; kernel: ffgpu_redact.inc)
// A post-pass like the draw, on the stream of the forward or merge it follows: reads the records and full lists (per entry, or the merged ones),
// reads and writes the caller's frames and nothing of the executor's.
template <class Frame>
static int exec_redact(ffgpu_exec *ex, const char *what, int which, const Frame *targets, int ntargets, const ffgpu_redact_spec *spec, void *stream)
{
    const bool nv12 = std::is_same<Frame, ffgpu_nv12_frame>::value;
    if (!exec_ok(ex, what)) return -1;
    if (!targets) { ffgpu_set_error("%s: NULL targets", what); return -1; }
    RedactPlan pl;
    if (ffgpu_redact_spec_check(what, spec, nv12, pl)) return -1;
    DetSource src;
    hipStream_t s;
    if (exec_source(ex, what, "REDACT", "redaction", STRIDE_CLAMPED, which, ntargets, stream, src, &s)) return -1;
    std::vector<DrawTarget> tab;
    if (ffgpu_frame_table(what, FRAME_DRAW, targets, ntargets, tab)) return -1;
    return ffgpu_launch_redact(what, nv12, src, tab, pl, s);
}

extern "C" int ffgpu_exec_redact_bgr(ffgpu_exec *ex, int which, const ffgpu_bgr_frame *targets, int ntargets, const ffgpu_redact_spec *spec, void *stream)
{
    return exec_redact(ex, "redact_bgr", which, targets, ntargets, spec, stream);
}

extern "C" int ffgpu_exec_redact_nv12(ffgpu_exec *ex, int which, const ffgpu_nv12_frame *targets, int ntargets, const ffgpu_redact_spec *spec, void *stream)
{
    return exec_redact(ex, "redact_nv12", which, targets, ntargets, spec, stream);
}

// -------------------------------------------------------------------------- the detections blurred in the frames (include/ffcnn_hip.h; kernel: ffgpu_blur.inc)
// A post-pass like the redaction, with a scratch surface per target: reads the records and full lists, reads and writes the caller's frames and
// scratch surfaces and nothing of the executor's.
template <class Frame>
static int exec_blur(ffgpu_exec *ex, const char *what, int which, const Frame *targets, const Frame *scratch, int ntargets, const ffgpu_blur_spec *spec, void *stream)
{
    const bool nv12 = std::is_same<Frame, ffgpu_nv12_frame>::value;
    if (!exec_ok(ex, what)) return -1;
    if (!targets) { ffgpu_set_error("%s: NULL targets", what); return -1; }
    if (!scratch) { ffgpu_set_error("%s: NULL scratch", what); return -1; }
    BlurPlan pl;
    if (ffgpu_blur_spec_check(what, spec, pl)) return -1;
    DetSource src;
    hipStream_t s;
    if (exec_source(ex, what, "BLUR", "blur", STRIDE_CLAMPED, which, ntargets, stream, src, &s)) return -1;
    std::vector<DrawTarget> tab, stab;
    if (ffgpu_frame_table(what, FRAME_DRAW, targets, ntargets, tab) || ffgpu_frame_table(what, FRAME_SCRATCH, scratch, ntargets, stab)) return -1;
    return ffgpu_launch_blur(what, nv12, src, tab, stab, pl, s);
}

extern "C" int ffgpu_exec_blur_bgr(ffgpu_exec *ex, int which, const ffgpu_bgr_frame *targets, const ffgpu_bgr_frame *scratch, int ntargets,
                                   const ffgpu_blur_spec *spec, void *stream)
{
    return exec_blur(ex, "blur_bgr", which, targets, scratch, ntargets, spec, stream);
}

extern "C" int ffgpu_exec_blur_nv12(ffgpu_exec *ex, int which, const ffgpu_nv12_frame *targets, const ffgpu_nv12_frame *scratch, int ntargets,
                                    const ffgpu_blur_spec *spec, void *stream)
{
    return exec_blur(ex, "blur_nv12", which, targets, scratch, ntargets, spec, stream);
}

// -------------------------------------------------------------------------- the detections cut out of the frames (include/ffcnn_hip.h; kernels: ffgpu_crop.inc)
// A post-pass like the draw, on the stream of the forward or merge it follows: reads the records and full lists (per entry, or the merged ones) and
// the caller's frames, writes the caller's batch buffer and table and nothing of the executor's.
template <class Frame>
static int exec_crop(ffgpu_exec *ex, const char *what, int which, const Frame *sources, int ntargets, const ffgpu_crop_spec *spec,
                     void *d_out, void *d_table, int capacity, void *stream)
{
    if (!exec_ok(ex, what)) return -1;
    if (!sources) { ffgpu_set_error("%s: NULL targets", what); return -1; }
    CropPlan pl;
    if (ffgpu_crop_spec_check(what, spec, pl) || ffgpu_crop_buffers_check(what, d_out, d_table, capacity)) return -1;
    DetSource src;
    hipStream_t s;
    if (exec_source(ex, what, "CROP", "crop", STRIDE_CLAMPED, which, ntargets, stream, src, &s)) return -1;
    std::vector<CropSrc> tab;
    if (ffgpu_frame_table(what, FRAME_DRAW, sources, ntargets, tab)) return -1;
    return ffgpu_launch_crop(std::is_same<Frame, ffgpu_nv12_frame>::value, src, tab, pl, d_out, d_table, capacity, s);
}

extern "C" int ffgpu_exec_crop_bgr(ffgpu_exec *ex, int which, const ffgpu_bgr_frame *sources, int ntargets, const ffgpu_crop_spec *spec,
                                   void *d_out, void *d_table, int capacity, void *stream)
{
    return exec_crop(ex, "crop_bgr", which, sources, ntargets, spec, d_out, d_table, capacity, stream);
}

extern "C" int ffgpu_exec_crop_nv12(ffgpu_exec *ex, int which, const ffgpu_nv12_frame *sources, int ntargets, const ffgpu_crop_spec *spec,
                                    void *d_out, void *d_table, int capacity, void *stream)
{
    return exec_crop(ex, "crop_nv12", which, sources, ntargets, spec, d_out, d_table, capacity, stream);
}

// -------------------------------------------------------------------------- the detections tracked across frames (include/ffcnn_hip.h; kernel: ffgpu_track.inc)
// A post-pass like the crop, on the stream of the forward or merge it follows: reads the records and full lists (per entry, or the merged ones),
// writes the caller's state, ids and tracked records and nothing of the executor's.
extern "C" int ffgpu_exec_track(ffgpu_exec *ex, int which, const int *streams, int ntargets, const ffgpu_track_spec *spec, void *d_state, int nstreams,
                                void *d_ids, void *d_out_records, void *d_out_lists, void *stream)
{
    const char *const what = "exec_track";
    if (!exec_ok(ex, what)) return -1;
    if (ffgpu_track_args_check(what, streams, ntargets, spec, d_state, nstreams, d_ids, d_out_records, d_out_lists)) return -1;
    DetSource src;
    hipStream_t s;
    if (exec_source(ex, what, "TRACK", "tracker", STRIDE_REFUSED, which, ntargets, stream, src, &s)) return -1;
    return ffgpu_launch_track(src, streams, ntargets, *spec, d_state, d_ids, d_out_records, d_out_lists, s);
}

// -------------------------------------------------------------------------- zones and lines (include/ffcnn_hip.h; kernel: ffgpu_zones.inc)
// A post-pass like the tracker, on the stream of the forward or merge it follows: reads the records and full lists (per entry, or the merged ones), the
// caller's scenes and ids, writes the caller's state, events and gated records and nothing of the executor's.
extern "C" int ffgpu_exec_zones(ffgpu_exec *ex, int which, const int *streams, int ntargets, const ffgpu_zones_spec *spec, const void *d_scenes, void *d_state,
                                int nstreams, const void *d_ids, void *d_events, void *d_out_records, void *d_out_lists, void *stream)
{
    const char *const what = "exec_zones";
    if (!exec_ok(ex, what)) return -1;
    if (ffgpu_zones_args_check(what, streams, ntargets, spec, d_scenes, d_state, nstreams, d_ids, d_events, d_out_records, d_out_lists)) return -1;
    DetSource src;
    hipStream_t s;
    if (exec_source(ex, what, "ZONES", "zones pass", STRIDE_REFUSED, which, ntargets, stream, src, &s)) return -1;
    return ffgpu_launch_zones(src, streams, ntargets, *spec, d_scenes, d_state, d_ids, d_events, d_out_records, d_out_lists, s);
}

// -------------------------------------------------------------------------- track trails (include/ffcnn_hip.h; kernel: ffgpu_trails.inc)
// A post-pass like the zones pass, on the stream of the forward or merge it follows: reads the records and full lists (per entry, or the merged ones)
// and the caller's ids, writes the caller's state, rows and items and nothing of the executor's.
extern "C" int ffgpu_exec_trails(ffgpu_exec *ex, int which, const int *streams, int ntargets, const ffgpu_trails_spec *spec, void *d_state, int nstreams,
                                 const void *d_ids, void *d_rows, void *d_items, int items_stride, int first_item, int nitems, void *stream)
{
    const char *const what = "exec_trails";
    if (!exec_ok(ex, what)) return -1;
    TrailsPlan pl;
    if (ffgpu_trails_args_check(what, streams, ntargets, spec, d_state, nstreams, d_ids, d_rows, d_items, items_stride, first_item, nitems, pl)) return -1;
    DetSource src;
    hipStream_t s;
    if (exec_source(ex, what, "TRAILS", "trails pass", STRIDE_REFUSED, which, ntargets, stream, src, &s)) return -1;
    return ffgpu_launch_trails(src, streams, ntargets, pl, d_state, d_ids, d_rows, d_items, items_stride, first_item, nitems, s);
}

// -------------------------------------------------------------------------- heat maps (include/ffcnn_hip.h; kernels: ffgpu_heat.inc)
// A post-pass like the zones pass, on the stream of the forward or merge it follows: reads the records and full lists (per entry, or the merged ones),
// writes the caller's state and rows and nothing of the executor's.  The blend has no executor form: it reads the state, not the records.
extern "C" int ffgpu_exec_heat(ffgpu_exec *ex, int which, const int *streams, int ntargets, const ffgpu_heat_spec *spec, void *d_state, int nstreams,
                               void *d_rows, void *stream)
{
    const char *const what = "exec_heat";
    if (!exec_ok(ex, what)) return -1;
    HeatPlan pl;
    if (ffgpu_heat_args_check(what, streams, ntargets, spec, d_state, nstreams, d_rows, pl)) return -1;
    DetSource src;
    hipStream_t s;
    if (exec_source(ex, what, "HEAT", "heat pass", STRIDE_CLAMPED, which, ntargets, stream, src, &s)) return -1;
    return ffgpu_launch_heat(src, streams, ntargets, pl, d_state, d_rows, s);
}

// -------------------------------------------------------------------------- motion maps (include/ffcnn_hip.h; kernels: ffgpu_motion.inc)
// A post-pass like the zones pass, on the stream of the forward or merge it follows: reads the records and full lists (per entry, or the merged ones)
// and the caller's motion state, writes the caller's words and gated records and nothing of the executor's.  The update has no executor form: it
// reads frames, not records.
extern "C" int ffgpu_exec_motion_gate(ffgpu_exec *ex, int which, const int *streams, int ntargets, const ffgpu_motion_spec *spec, const void *d_state, int nstreams,
                                      void *d_words, void *d_out_records, void *d_out_lists, void *stream)
{
    const char *const what = "exec_motion_gate";
    if (!exec_ok(ex, what)) return -1;
    MotionPlan pl;
    if (ffgpu_motion_gate_args_check(what, streams, ntargets, spec, d_state, nstreams, d_words, d_out_records, d_out_lists, pl)) return -1;
    DetSource src;
    hipStream_t s;
    if (exec_source(ex, what, "MOTION", "motion gate", STRIDE_REFUSED, which, ntargets, stream, src, &s)) return -1;
    return ffgpu_launch_motion_gate(src, streams, ntargets, pl, d_state, d_words, d_out_records, d_out_lists, s);
}

// -------------------------------------------------------------------------- captions (include/ffcnn_hip.h; kernels: ffgpu_text.inc)
// A post-pass like the draw, on the stream of the forward or merge it follows, in two launches: the items composed from the records and full lists (per
// entry, or the merged ones) into the caller's d_items, then rasterised into the caller's frames.  Nothing of the executor's is written.
template <class Frame>
static int exec_caption(ffgpu_exec *ex, const char *what, int which, const Frame *targets, int ntargets, const ffgpu_caption_spec *spec, const void *d_ids,
                        void *d_items, int items_stride, const void *d_font, void *stream)
{
    if (!exec_ok(ex, what)) return -1;
    if (!targets) { ffgpu_set_error("%s: NULL targets", what); return -1; }
    CaptionPlan pl;
    if (ffgpu_caption_boxes_args_check(what, spec, d_ids, d_items, items_stride, pl)) return -1;
    DetSource src;
    hipStream_t s;
    if (exec_source(ex, what, "CAPTION", "caption", d_ids ? STRIDE_REFUSED : STRIDE_CLAMPED, which, ntargets, stream, src, &s)) return -1;
    std::vector<DrawTarget> tab;
    if (ffgpu_frame_table(what, FRAME_DRAW, targets, ntargets, tab)) return -1;
    if (ffgpu_launch_caption_boxes(src, ntargets, pl, d_ids, d_items, items_stride, s)) return -1;
    return ffgpu_launch_draw_text(std::is_same<Frame, ffgpu_nv12_frame>::value, d_items, items_stride, d_font, tab, s);
}

extern "C" int ffgpu_exec_caption_bgr(ffgpu_exec *ex, int which, const ffgpu_bgr_frame *targets, int ntargets, const ffgpu_caption_spec *spec,
                                      const void *d_ids, void *d_items, int items_stride, const void *d_font, void *stream)
{
    return exec_caption(ex, "caption_bgr", which, targets, ntargets, spec, d_ids, d_items, items_stride, d_font, stream);
}

extern "C" int ffgpu_exec_caption_nv12(ffgpu_exec *ex, int which, const ffgpu_nv12_frame *targets, int ntargets, const ffgpu_caption_spec *spec,
                                       const void *d_ids, void *d_items, int items_stride, const void *d_font, void *stream)
{
    return exec_caption(ex, "caption_nv12", which, targets, ntargets, spec, d_ids, d_items, items_stride, d_font, stream);
}

// -------------------------------------------------------------------------- the crops classified (include/ffcnn_hip.h; kernels: ffgpu_feature.inc)
// The tensor a feature spec names on this plan: its id and the frame's c x h x w, or -1 with a message.  layer == -1 is the last layer's, aliases
// resolved by canon[] (a trailing dropout or one-source route holds its source's tensor id).  Nothing takes that tensor's floats after the forward: the
// first-fit allocator of plan() hands a range on only to a tensor whose first use lies BEHIND the range's last use, pass 3 extends a tensor's last use to
// every layer that reads it -- a trailing route's index included -- and behind a trailing dropout (which touches nothing) no tensor is born at all.
static int feature_tensor(const ffgpu_exec *ex, const char *what, const ffgpu_feature_spec *spec, int *c, int *h, int *w)
{
    if (!spec) { ffgpu_set_error("%s: NULL spec", what); return -1; }
    if (spec->reserved != 0) { ffgpu_set_error("%s: spec: reserved must be 0", what); return -1; }
    const ffgpu_exec *pl = ex->child[0] ? ex->child[0] : ex;        // (the parts of a split executor have one and the same plan)
    const int L = ex->net->layer_num;
    int layer = spec->layer;
    if (layer < -1 || layer >= L) { ffgpu_set_error("%s: layer %d is outside -1 .. %d", what, layer, L - 1); return -1; }
    if (layer >= 0 && !(ex->flags & FFGPU_KEEP_ALL)) { ffgpu_set_error("%s: layer %d needs an FFGPU_KEEP_ALL executor (layer -1, the last layer's tensor, is legal on every plan)", what, layer); return -1; }
    if (layer < 0) layer = L - 1;
    if (L < 1) { ffgpu_set_error("%s: the net has no layer", what); return -1; }
    if (ex->net->layer_list[layer].type == LAYER_TYPE_YOLO) {
        ffgpu_set_error("%s: layer %d is a [yolo] layer: it leaves no tensor (its product is the detection records)", what, layer);
        return -1;
    }
    const int t = pl->layout.canon[layer];
    if (t == -1) { ffgpu_set_error("%s: layer %d is an alias of the net input, which is frame-major: no CNHW tensor", what, layer); return -1; }
    if (t < 0 || !pl->layout.readable[layer]) { ffgpu_set_error("%s: layer %d is not materialised by this executor (fused away or no tensor)", what, layer); return -1; }
    const LAYER &o = ex->net->layer_list[layer + 1];
    *c = o.c; *h = o.h; *w = o.w;
    return t;
}

extern "C" int ffgpu_exec_feature_dim(const ffgpu_exec *ex, const ffgpu_feature_spec *spec)
{
    const char *const what = "exec_feature_dim";
    if (!alive(ex, what)) return -1;
    int c = 0, h = 0, w = 0;
    if (feature_tensor(ex, what, spec, &c, &h, &w) < 0) return -1;
    if (spec->pool < FFGPU_FEAT_FLAT || spec->pool > FFGPU_FEAT_MAX) { ffgpu_set_error("%s: pool %d is none of FFGPU_FEAT_FLAT, _MEAN, _MAX", what, spec->pool); return -1; }
    const int d = ffgpu_feature_dim(c, h, w, spec->pool);
    if (d < 1) { ffgpu_set_error("%s: %d x %d x %d gives a plane or a row of more than 2^24 values", what, c, h, w); return -1; }
    return d;
}

// A post-pass like the crop, on the stream of the forward it follows: reads the tensor the forward left (each part's, on a split executor), writes the
// caller's rows and nothing of the executor's.
extern "C" int ffgpu_exec_features(ffgpu_exec *ex, const ffgpu_feature_spec *spec, float *d_out, long out_stride, void *stream)
{
    const char *const what = "exec_features";
    if (!exec_ok(ex, what)) return -1;
    int c = 0, h = 0, w = 0;
    const int t = feature_tensor(ex, what, spec, &c, &h, &w);
    if (t < 0) return -1;
    if (ffgpu_feature_args_check(what, ex->N, c, h, w, spec->pool, spec->post, d_out, out_stride)) return -1;
    const hipStream_t s = stream ? (hipStream_t)stream : ex->own_stream;
    if (s != ex->last_stream) { ffgpu_set_error("%s: the features must be enqueued on the stream of the forward they follow", what); return -1; }
    const float *parts[ffgpu_exec::MAXPART] = {};
    const int nparts = ex->child[0] ? ex->nchild : 1;
    for (int k = 0; k < nparts; k++) parts[k] = tensor_ptr(ex->child[0] ? ex->child[k] : ex, t);
    return ffgpu_launch_features(parts, nparts, ex->N / nparts, c, h, w, spec->pool, spec->post, d_out, out_stride, s);
}

// On the first stage's executor: reads its records and full lists (per entry, or the merged ones), the caller's table and labels; writes the caller's
// relabelled records and lists and nothing of the executor's.
extern "C" int ffgpu_exec_relabel(ffgpu_exec *ex, int which, const void *d_table, int capacity, const void *d_labels, int k, int ntargets,
                                  const ffgpu_relabel_spec *spec, void *d_out_records, void *d_out_lists, void *stream)
{
    const char *const what = "exec_relabel";
    if (!exec_ok(ex, what)) return -1;
    if (ffgpu_relabel_args_check(what, d_table, capacity, d_labels, k, ntargets, spec, d_out_records)) return -1;
    DetSource src;
    hipStream_t s;
    if (exec_source(ex, what, "RELABEL", "relabelling", STRIDE_REFUSED, which, ntargets, stream, src, &s)) return -1;
    return ffgpu_launch_relabel(d_table, capacity, d_labels, k, src, ntargets, *spec, d_out_records, d_out_lists, s);
}

// FFGPU_KEEP_ALL executors: one 64-bit hash per materialised layer over the layer's WHOLE batch tensor (every bit of every frame), computed on the
// device behind the last forward; 0 for layers this executor does not materialise.  What the concurrency soak compares round after round
// (tests/test_gpu_round5.py): 8 bytes per layer cross the bus instead of the activations.
extern "C" int ffgpu_exec_hash_layers(ffgpu_exec *ex, unsigned long long *host_out, int cap)
{
    if (!alive(ex, "hash_layers")) return -1;
    if (ex->child[0]) { ffgpu_set_error("hash_layers: not for FFGPU_SPLIT2 executors"); return -1; }
    if (!(ex->flags & FFGPU_KEEP_ALL)) { ffgpu_set_error("hash_layers needs an FFGPU_KEEP_ALL executor"); return -1; }
    const int L = ex->net->layer_num;
    if (!host_out || cap < L) { ffgpu_set_error("hash_layers: room for %d values needed", L); return -1; }
    unsigned long long *d = nullptr;
    FFGPU_CHECK(hipMalloc(&d, sizeof(unsigned long long) * L));
    hipStream_t s = ex->last_stream;
    int rc = 0, nh = 0;
    if (hipMemsetAsync(d, 0, sizeof(unsigned long long) * L, s) != hipSuccess) rc = -1;
    for (int i = 0; i < L && !rc; i++) {
        if (ex->layout.canon[i] < 0 || !ex->layout.readable[i]) continue;
        const LAYER &o = ex->net->layer_list[i + 1];
        if (ffgpu_launch_hash64(tensor_ptr(ex, ex->layout.canon[i]), (long)o.c * ex->N * o.w * o.h, d + i, s)) rc = -1;
        nh++;
    }
    if (!rc && hipStreamSynchronize(s) != hipSuccess) rc = -1;
    if (!rc && copy_d2h(host_out, d, sizeof(unsigned long long) * L)) rc = -1;
    (void)hipFree(d);
    if (rc) { ffgpu_set_error("hash_layers: a device call failed"); return -1; }
    return nh;
}

extern "C" int ffgpu_exec_read_layer(ffgpu_exec *ex, int layer, int frame, float *host_out, size_t cap_floats)
{
    if (!alive(ex, "read_layer")) return -1;
    if (!host_out || frame < 0 || frame >= ex->N) { ffgpu_set_error("read_layer: bad arguments"); return -1; }
    if (ex->child[0]) return ffgpu_exec_read_layer(ex->child[frame / ex->child[0]->N], layer, frame % ex->child[0]->N, host_out, cap_floats);
    FFGPU_CHECK(hipStreamSynchronize(ex->last_stream));
    if (layer == -2) {                                            // candidates in reference emission order
        int cnt = 0;
        if (copy_d2h(&cnt, &ex->d_dets[frame].ncand, sizeof(int))) return -1;    // (k_nms has reset d_ncand)
        cnt = std::min(cnt, ex->cand_cap);
        if ((size_t)cnt * 6 > cap_floats) { ffgpu_set_error("read_layer: buffer too small"); return -1; }
        std::vector<BBOX> b(cnt);
        std::vector<int> k(cnt), idx(cnt);
        if (cnt) {
            if (copy_d2h(b.data(), ex->d_cand + (size_t)frame * ex->cand_cap, sizeof(BBOX) * cnt)) return -1;
            if (copy_d2h(k.data(), ex->d_cand_key + (size_t)frame * ex->cand_cap, sizeof(int) * cnt)) return -1;
        }
        for (int i = 0; i < cnt; i++) idx[i] = i;
        std::sort(idx.begin(), idx.end(), [&](int a, int c) { return k[a] < k[c]; });
        for (int i = 0; i < cnt; i++) memcpy(host_out + 6 * i, &b[idx[i]], sizeof(BBOX));
        return cnt;
    }
    if (layer == -1) {                                            // the network input as the first layer saw it (frame-major)
        const size_t fl = (size_t)ex->in_c * ex->in_h * ex->in_w;
        if (ex->last.form != IN_F32) { ffgpu_set_error("read_layer: the last forward's frames were u8 images converted by the first kernel -- no fp32 input tensor exists"); return -1; }
        if (!ex->last.frames) { ffgpu_set_error("read_layer: no forward has run yet"); return -1; }
        if (fl > cap_floats) { ffgpu_set_error("read_layer: buffer too small"); return -1; }
        if (copy_d2h(host_out, ex->last.frames + (size_t)frame * fl, fl * sizeof(float))) return -1;
        return (int)fl;
    }
    // (a layer with a tensor of its own that a launch leaves unwritten or partly written -- the front kernel's inside, a sparse head's input -- says so on every plan)
    if (layer >= 0 && layer < ex->net->layer_num && ex->layout.canon[layer] == layer && !ex->layout.readable[layer]) {
        ffgpu_set_error("read_layer: layer %d is not materialised by this executor (fused away or no tensor)", layer);
        return -1;
    }
    if (!(ex->flags & FFGPU_KEEP_ALL)) { ffgpu_set_error("read_layer needs an FFGPU_KEEP_ALL executor"); return -1; }
    if (layer < 0 || layer >= ex->net->layer_num || ex->layout.canon[layer] < 0 || !ex->layout.readable[layer]) {
        ffgpu_set_error("read_layer: layer %d is not materialised by this executor (fused away or no tensor)", layer);
        return -1;
    }
    const LAYER &o = ex->net->layer_list[layer + 1];
    const size_t plane = (size_t)o.w * o.h;
    if (plane * o.c > cap_floats) { ffgpu_set_error("read_layer: buffer too small"); return -1; }
    const float *src = tensor_ptr(ex, ex->layout.canon[layer]) + (size_t)frame * plane;
    {   // the frame's planes (one per channel, N planes apart in CNHW) gathered into the bounce buffer, then into caller memory
        const size_t row = plane * sizeof(float), per = std::max<size_t>(1, BOUNCE_BYTES / row);
        if (row > BOUNCE_BYTES) {                                  // a plane larger than the staging buffer (> 2048 x 2048 floats): contiguous, chunked plane by plane
            for (size_t c = 0; c < (size_t)o.c; c++)
                if (copy_d2h(host_out + c * plane, src + c * plane * ex->N, row)) return -1;
            return (int)(plane * o.c);
        }
        Bounce &bn = bounce_cur();
        std::lock_guard<std::mutex> lk(bn.mu);
        if (bounce_ready(bn)) return -1;
        char *const g_bounce = bn.p;
        for (size_t c0 = 0; c0 < (size_t)o.c; c0 += per) {
            const size_t nc = std::min(per, (size_t)o.c - c0);
            FFGPU_CHECK(hipMemcpy2D(g_bounce, row, src + c0 * plane * ex->N, row * ex->N, row, nc, hipMemcpyDeviceToHost));
            memcpy(host_out + c0 * plane, g_bounce, nc * row);
        }
    }
    return (int)(plane * o.c);
}

// The steps of one forward timed one by one on the executor's own stream: a warm-up pass, then `reps` passes with an event behind every step;
// us[i] = mean time of step i.  The events are destroyed on every path.
static int timed_issue(ffgpu_exec *ex, const float *d_frames, int reps, std::vector<float> &us)
{
    hipStream_t s = ex->own_stream;
    const InputSrc in = fp32_src(d_frames);
    if (push_params(ex, in, s)) return -1;
    const size_t n = ex->steps.size();
    std::vector<hipEvent_t> ev(n + 1, nullptr);
    us.assign(n, 0.f);
    auto run = [&]() -> int {
        for (auto &e : ev) FFGPU_CHECK(hipEventCreate(&e));
        if (issue_all(ex, in, s)) return -1;                    // warm
        for (int r = 0; r < reps; r++) {
            FFGPU_CHECK(hipEventRecord(ev[0], s));
            for (size_t i = 0; i < n; i++) {
                if (issue_step(ex, ex->steps[i], in, s)) return -1;
                FFGPU_CHECK(hipEventRecord(ev[i + 1], s));
            }
            FFGPU_CHECK(hipStreamSynchronize(s));
            for (size_t i = 0; i < n; i++) {
                float ms = 0.f;
                FFGPU_CHECK(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
                us[i] += ms * 1000.f / reps;
            }
        }
        return 0;
    };
    const int rc = run();
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    if (!rc) ex->last_stream = s;
    return rc;
}

extern "C" int ffgpu_exec_profile(ffgpu_exec *ex, const float *d_frames, float us_by_kind[LAYER_TYPE_TOTOAL])
{
    if (!alive(ex, "profile")) return -1;
    if (!d_frames || !us_by_kind) { ffgpu_set_error("profile: NULL argument"); return -1; }
    if (ex->child[0]) { ffgpu_set_error("profile: not available on a split executor"); return -1; }
    std::vector<float> us;
    if (timed_issue(ex, d_frames, 1, us)) return -1;
    for (int k = 0; k < LAYER_TYPE_TOTOAL; k++) us_by_kind[k] = 0.f;
    for (size_t i = 0; i < us.size(); i++) {
        const int k = ex->steps[i].ltype;
        if (k >= 0 && k < LAYER_TYPE_TOTOAL) us_by_kind[k] += us[i];
    }
    return 0;
}

extern "C" int ffgpu_exec_profile_steps(ffgpu_exec *ex, const float *d_frames, int *layer_of, float *us, int cap)
{
    if (!alive(ex, "profile_steps")) return -1;
    if (!d_frames || !layer_of || !us) { ffgpu_set_error("profile_steps: NULL argument"); return -1; }
    if (ex->child[0]) { ffgpu_set_error("profile_steps: not available on a split executor"); return -1; }
    std::vector<float> acc;
    if (timed_issue(ex, d_frames, 5, acc)) return -1;
    const int n = (int)std::min<size_t>(acc.size(), (size_t)cap);
    for (int i = 0; i < n; i++) { layer_of[i] = ex->steps[i].layer; us[i] = acc[i]; }
    return n;
}

// -------------------------------------------------------------------------- C-ABI: net device state
// device copy of the net's folded filter rows on `device` (-1: the calling thread's current device); upload == false leaves
// it zeroed -- the other GPUs of a node receive the weights over RCCL (ffgpu_node.inc)
static ffgpu_netdev *netdev_create_on(NET *net, int device, bool upload)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        (void)hipGetLastError();
        ffgpu_set_error("no HIP device visible: libffcnn_hip has no CPU fallback");
        return nullptr;
    }
    ffgpu_netdev *dev = new ffgpu_netdev();
    dev->net = net;
    if (device >= 0) { dev->device = device; if (hipSetDevice(device) != hipSuccess) { ffgpu_set_error("hipSetDevice(%d) failed", device); delete dev; return nullptr; } }
    else if (hipGetDevice(&dev->device) != hipSuccess) dev->device = 0;
    dev->weight_bytes = sizeof(float) * (size_t)std::max(net->weight_size, 1);
    if (hipMalloc(&dev->d_weights, dev->weight_bytes) != hipSuccess ||
        (upload ? (copy_h2d(dev->d_weights, net->weight_buf, sizeof(float) * (size_t)net->weight_size) ? hipErrorUnknown : hipSuccess)
                : hipMemset(dev->d_weights, 0, dev->weight_bytes)) != hipSuccess ||
        hipStreamSynchronize(nullptr) != hipSuccess) {                // (the memset is asynchronous on the NULL stream: a broadcast on
                                                                      //  another stream must not be overtaken by it)
        ffgpu_set_error("weight upload failed: %s", hipGetErrorString(hipGetLastError()));
        (void)hipFree(dev->d_weights);
        delete dev;
        return nullptr;
    }
    return dev;
}

extern "C" void *ffgpu_netdev_create(NET *net) { return netdev_create_on(net, -1, true); }

extern "C" float *ffgpu_host_alloc(size_t bytes)
{
    void *p = nullptr;
    if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    memset(p, 0, bytes);
    { std::lock_guard<std::mutex> lk(g_pin_mu); g_pinned.push_back({ (const char *)p, bytes }); }
    return (float *)p;
}

extern "C" void ffgpu_host_free(float *p)
{
    if (!p) return;
    {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        for (size_t i = 0; i < g_pinned.size(); i++) if (g_pinned[i].p == (const char *)p) { g_pinned.erase(g_pinned.begin() + i); break; }
    }
    (void)hipHostFree(p);
}

extern "C" void ffgpu_netdev_destroy(void *p)
{
    ffgpu_netdev *dev = (ffgpu_netdev *)p;
    if (!dev) return;
    if (dev->exec1) { ffgpu_exec_destroy(dev->exec1); dev->exec1 = nullptr; }
    // executors the caller still holds outlive the net as orphans: their steps point into d_weights and the layer table,
    // so they wait for their streams here and from now on refuse to run (alive()); ffgpu_exec_destroy still frees them
    std::vector<ffgpu_exec *> left;
    { std::lock_guard<std::mutex> lk(dev->mu); left.swap(dev->execs); }
    for (ffgpu_exec *ex : left) {
        if (ex->last_stream) (void)hipStreamSynchronize(ex->last_stream);
        ex->dev = nullptr; ex->net = nullptr;
    }
    (void)hipFree(dev->d_weights);
    delete dev;
}

// net_forward (ffcnn.c:476-520) for the one frame in layer_list[0].data: H2D, the batch-1 executor, boxes back into
// net->bbox_list -- ALL of them, up to net->bbox_max like the reference (the fixed-size record holds the first
// FFGPU_MAX_DET; the rest comes from the executor's full list).  profile != 0 (FFCNN_PROFILE=1, the counterpart of
// ENABLE_NET_PROFILE, ffcnn.c:33,494-510): the forward runs launch by launch between HIP events and the device time of
// every layer kind is added to net->timeused[] (whole milliseconds of the accumulated time, as the reference keeps them).
extern "C" int ffgpu_netdev_forward1(NET *net, void *p, int profile)
{
    ffgpu_netdev *dev = (ffgpu_netdev *)p;
    if (!dev->exec1) {
        // one frame at a time is latency: the records come back through the pinned host mirror (no device-to-host copy), and the
        // input tensor the application fills is page-locked memory of the runtime since net_load (ffgpu_host_alloc): one DMA up
        dev->exec1 = ffgpu_exec_create(net, 1, FFGPU_HOST_DETS);
        if (!dev->exec1) return -1;
    }
    ffgpu_exec *ex = dev->exec1;
    ex->s1 = net->s1 ? net->s1 : 1;
    ex->s2 = net->s2 ? net->s2 : 1;
    ex->bbox_max = std::max(net->bbox_max, 1);
    if (profile) {
        if (ensure_input(ex)) return -1;
        if (copy_h2d(ex->d_input, net->layer_list[0].data, sizeof(float) * (size_t)ex->in_c * ex->in_h * ex->in_w)) return -1;
        float us[LAYER_TYPE_TOTOAL];
        if (ffgpu_exec_profile(ex, ex->d_input, us)) return -1;
        for (int k = 0; k < LAYER_TYPE_TOTOAL; k++) { dev->us_acc[k] += us[k]; net->timeused[k] = (int)(dev->us_acc[k] / 1000.0 + 0.5); }
    } else if (ffgpu_exec_forward_host(ex, net->layer_list[0].data)) return -1;
    static thread_local ffgpu_frame_dets rec;
    if (ffgpu_exec_read_dets(ex, &rec, 1) != 1) return -1;
    const ffcnn_ext *ext = ffcnn_ext_of(net);
    const int nb = std::max(0, std::min(rec.nfull, std::min(net->bbox_max, ext ? ext->box_cap : FFGPU_MAX_DET)));
    if (nb <= FFGPU_MAX_DET) memcpy(net->bbox_list, rec.box, sizeof(BBOX) * (size_t)nb);
    else if (ffgpu_exec_read_boxes(ex, 0, net->bbox_list, nb) < 0) return -1;
    net->bbox_num = nb;
    return 0;
}

extern "C" int ffgpu_netdev_profile_us(void *p, double us_by_kind[LAYER_TYPE_TOTOAL])
{
    ffgpu_netdev *dev = (ffgpu_netdev *)p;
    if (!dev) return -1;
    for (int k = 0; k < LAYER_TYPE_TOTOAL; k++) us_by_kind[k] = dev->us_acc[k];
    return 0;
}

extern "C" int ffgpu_net_weights_dev(NET *net, void **dev_ptr, size_t *bytes)
{
    ffgpu_netdev *dev = netdev_of(net);
    if (!dev) return -1;
    if (dev_ptr) *dev_ptr = dev->d_weights;
    if (bytes) *bytes = sizeof(float) * (size_t)net->weight_size;
    return 0;
}

extern "C" int ffgpu_net_weights_commit(NET *net, void *stream)
{
    ffgpu_netdev *dev = netdev_of(net);
    if (!dev) return -1;
    std::lock_guard<std::mutex> lk(dev->mu);
    for (ffgpu_exec *ex : dev->execs)           // fused blocks keep their constants in a packed LDS image
        if (repack(ex, stream ? (hipStream_t)stream : ex->own_stream)) return -1;
    if (!stream) for (ffgpu_exec *ex : dev->execs) FFGPU_CHECK(hipStreamSynchronize(ex->own_stream));
    return 0;
}

#include "ffgpu_node.inc"

// -------------------------------------------------------------------------- C-ABI: single conv on device tensors
static void fill_desc(ConvDesc &d, const float *in, const float *filt, float *out, int batch,
                      int iw, int ih, int ic, int groups, int pad, int stride, int fs, int ow, int oh, int oc, int act, int flags)
{
    memset(&d, 0, sizeof d);
    d.in = in; d.filt = filt; d.out = out; d.N = batch;
    d.iw = iw; d.ih = ih; d.ic = ic; d.ow = ow; d.oh = oh; d.oc = oc;
    d.fs = fs; d.stride = stride; d.pad = pad; d.groups = groups; d.act = act; d.flags = flags & (FFGPU_COMPAT_V6 | FFGPU_BF16_PW);
    d.in_cs = (long)batch * iw * ih; d.in_ns = (long)iw * ih;
    d.out_cs = (long)batch * ow * oh; d.out_ns = (long)ow * oh;
}

extern "C" int ffgpu_groupconv_dev(const float *d_in, const float *d_filt, float *d_out, int batch,
                                   int iw, int ih, int ic, int groups, int pad, int stride,
                                   int fs, int fn, int ow, int oh, int oc, int act,
                                   int flags, int variant, void *stream)
{
    if (!d_in || !d_filt || !d_out || batch < 1 || fn != oc) { ffgpu_set_error("groupconv_dev: bad arguments"); return -1; }
    ConvDesc d;
    fill_desc(d, d_in, d_filt, d_out, batch, iw, ih, ic, groups, pad, stride, fs, ow, oh, oc, act, flags);
    return ffgpu_launch_conv(d, variant, (hipStream_t)stream);
}

// The sparse form of a yolo head's input layer on caller-owned tensors (tests): the pointwise layer ic -> 3 (5 + classes) on batch x ih x iw pixels as the box
// pass and the class pass of k_conv_x3, whatever AUTO would pick for the shape.  d_list (batch ih iw / 4 ints) and d_count (one int) are the caller's: the
// count is NOT reset here -- a caller zeroes it (or leaves it as the case under test wants it) and reads list and count back after the call.
extern "C" int ffgpu_sparse_head_dev(const float *d_in, const float *d_filt, float *d_out, int batch, int iw, int ih, int ic, int classes, int act,
                                     float thresh, int *d_list, int *d_count, void *stream)
{
    if (!d_in || !d_filt || !d_out || !d_list || !d_count || batch < 1 || iw < 1 || ih < 1 || classes < 1 || classes > 4096) { ffgpu_set_error("sparse_head_dev: bad arguments"); return -1; }
    ConvDesc d;
    fill_desc(d, d_in, d_filt, d_out, batch, iw, ih, ic, 1, 0, 1, 1, iw, ih, 3 * (5 + classes), act, 0);
    d.sp_classes = classes; d.sp_thresh = thresh; d.sp_list = d_list; d.sp_ctr = d_count;
    return ffgpu_launch_conv(d, FFGPU_K_CONV_X3, (hipStream_t)stream);
}

// pure host code: what an executor made with `flags` launches for the pointwise layer ic -> 3 (5 + classes) in front of a yolo head
extern "C" int ffgpu_sparse_head_launch_text(int batch, int iw, int ih, int ic, int classes, int flags, char *buf, int cap)
{
    if (!buf || cap < 1 || batch < 1 || iw < 1 || ih < 1 || ic < 1 || classes < 1) { ffgpu_set_error("sparse_head_launch_text: bad arguments"); return -1; }
    ConvDesc d;
    fill_desc(d, nullptr, nullptr, nullptr, batch, iw, ih, ic, 1, 0, 1, 1, iw, ih, 3 * (5 + classes), 0, 0);
    return ffgpu_conv_sparse_head_line(d, classes, sparse_head_wanted(flags | (knob(K_NO_FUSE) ? FFGPU_NO_FUSE : 0)), buf, (size_t)cap);
}

extern "C" const char *ffgpu_groupconv_kernel_name(int batch, int iw, int ih, int ic, int groups, int pad,
                                                   int stride, int fs, int fn, int variant)
{
    ConvDesc d;
    const int ow = (iw + 2 * pad - fs) / stride + 1, oh = (ih + 2 * pad - fs) / stride + 1;
    fill_desc(d, nullptr, nullptr, nullptr, batch, iw, ih, ic, groups, pad, stride, fs, ow, oh, fn, 0, 0);
    return ffgpu_conv_kernel_name(d, variant);
}

extern "C" float ffgpu_groupconv_time_dev(const float *d_in, const float *d_filt, float *d_out, int batch,
                                          int iw, int ih, int ic, int groups, int pad, int stride,
                                          int fs, int fn, int ow, int oh, int oc, int act,
                                          int flags, int variant, int warmup, int iters, void *stream)
{
    if (iters < 1 || fn != oc) { ffgpu_set_error("groupconv_time_dev: bad arguments"); return -1.f; }
    hipStream_t s = (hipStream_t)stream;
    ConvDesc d;
    fill_desc(d, d_in, d_filt, d_out, batch, iw, ih, ic, groups, pad, stride, fs, ow, oh, oc, act, flags);
    // like the executor, hand pointwise kernels their plan-time weight image (packed once, outside the timed loop)
    float *pk = nullptr;
    if (variant == FFGPU_K_AUTO && ffgpu_pw_pack_floats(d) > 0) {
        if (hipMalloc(&pk, ffgpu_pw_pack_floats(d) * sizeof(float)) != hipSuccess || ffgpu_pw_pack(d, pk, s)) { ffgpu_set_error("pack failed"); return -1.f; }
        d.wpack = pk;
    }
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { ffgpu_set_error("hipEventCreate failed"); return -1.f; }
    for (int i = 0; i < warmup; i++) if (ffgpu_launch_conv(d, variant, s)) return -1.f;
    (void)hipEventRecord(e0, s);
    for (int i = 0; i < iters; i++) if (ffgpu_launch_conv(d, variant, s)) return -1.f;
    (void)hipEventRecord(e1, s);
    if (hipEventSynchronize(e1) != hipSuccess) { ffgpu_set_error("hipEventSynchronize: %s", hipGetErrorString(hipGetLastError())); return -1.f; }
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return ms * 1000.f / iters;
}

static void irb_fill(IrbDesc &d, int batch, int iw, int ih, int ic, int ec, int oc, int stride, int act1, int actd, int act2, int res_act)
{
    d.N = batch; d.H = ih; d.W = iw; d.OH = (ih + 2 - 3) / stride + 1; d.OW = (iw + 2 - 3) / stride + 1;
    d.ic = ic; d.ec = ec; d.oc = oc; d.stride = stride;
    d.act1 = act1; d.actd = actd; d.act2 = act2; d.res_act = res_act;
}

// pure host code: what ffgpu_irb_plan decides for the block, as one line of text
extern "C" int ffgpu_irb_plan_text(int batch, int iw, int ih, int ic, int ec, int oc, int stride, int act1, int actd, int act2, int res_act, int flags, char *buf, int cap)
{
    if (!buf || cap < 1 || batch < 1 || iw < 1 || ih < 1 || stride < 1) { ffgpu_set_error("irb_plan_text: bad arguments"); return -1; }
    IrbDesc d{};
    irb_fill(d, batch, iw, ih, ic, ec, oc, stride, act1, actd, act2, res_act);
    d.flags = flags & FFGPU_CONCURRENT;
    (void)ffgpu_irb_plan(d);
    return ffgpu_irb_plan_line(d, buf, (size_t)cap);
}

// pure host code: which instantiation of k_front a batch of `batch` frames on a plane of pw x ph takes (the net input is 2 pw x 2 ph) when it arrives in
// `form` (0 fp32, 1 u8 frames of the net's size, 2 u8 BGR frames of any size, 3 NV12 frames), and the launch shape: the block's plan, then the launch's own arithmetic
extern "C" int ffgpu_front_plan_text(int batch, int pw, int ph, int form, char *buf, int cap)
{
    if (!buf || cap < 1 || batch < 1 || pw < 1 || ph < 1 || form < 0 || form >= IN_FORMS) { ffgpu_set_error("front_plan_text: bad arguments"); return -1; }
    IrbDesc d{};
    irb_fill(d, batch, pw, ph, 8, 8, 4, 1, 0, 0, 0, 0);
    if (!ffgpu_irb_plan(d) || d.plan.family != IRB_THIN) return snprintf(buf, (size_t)cap, "unsupported");
    return ffgpu_front_plan_line(d, (InputForm)form, buf, (size_t)cap);
}

// pure host code: what an executor of `batch` frames made with `flags` does with a run of `blocks` blocks 48 -> 224 -> 48 on an iw x ih plane
extern "C" int ffgpu_irb_stage_plan_text(int batch, int iw, int ih, int blocks, int act1, int actd, int flags, char *buf, int cap)
{
    if (!buf || cap < 1 || batch < 1 || iw < 1 || ih < 1 || blocks < 1 || blocks > 64) { ffgpu_set_error("irb_stage_plan_text: bad arguments"); return -1; }
    std::vector<IrbDesc> run((size_t)blocks, IrbDesc{});
    for (IrbDesc &d : run) {
        irb_fill(d, batch, iw, ih, 48, 224, 48, 1, act1, actd, 0, 0);
        d.flags = flags & FFGPU_CONCURRENT;
        if (!ffgpu_irb_plan(d)) return snprintf(buf, (size_t)cap, "unsupported");
    }
    return ffgpu_irb_stage_line(run.data(), blocks, stage_wanted(batch, flags), buf, (size_t)cap);
}

// pure host code: the key of every fused-block instantiation, one per line, from the tables the planner dispatches through
extern "C" int ffgpu_irb_instantiations(char *buf, int cap)
{
    if (!buf || cap < 1) { ffgpu_set_error("irb_instantiations: bad arguments"); return -1; }
    return ffgpu_irb_keys(buf, (size_t)cap);
}

// pure host code: the table of ffgpu_knobs.hpp, one line per environment variable, with the value a read would return now
extern "C" int ffgpu_knobs_text(char *buf, int cap)
{
    if (!buf || cap < 1) { ffgpu_set_error("knobs_text: bad arguments"); return -1; }
    return ffgpu_knobs_lines(buf, (size_t)cap);
}

// pure host code: what the launch of a planned thin block does -- the single or the paired form of k_irb_thin, its band, tasks and grid
extern "C" int ffgpu_irb_thin_launch_text(int batch, int iw, int ih, int ic, int ec, int oc, int stride, int act1, int actd, int act2, int res_act, int flags, char *buf, int cap)
{
    if (!buf || cap < 1 || batch < 1 || iw < 1 || ih < 1 || stride < 1) { ffgpu_set_error("irb_thin_launch_text: bad arguments"); return -1; }
    IrbDesc d{};
    irb_fill(d, batch, iw, ih, ic, ec, oc, stride, act1, actd, act2, res_act);
    d.flags = flags & FFGPU_CONCURRENT;
    (void)ffgpu_irb_plan(d);
    return ffgpu_irb_thin_launch_line(d, buf, (size_t)cap);
}

// pure host code: what the launch of a planned block does where the streaming stride-2 form may take it -- thin_s2<4,24,8,3> or the planned key, frames
// per wave, band, tasks and grid
extern "C" int ffgpu_irb_s2_launch_text(int batch, int iw, int ih, int ic, int ec, int oc, int stride, int act1, int actd, int act2, int res_act, int flags, char *buf, int cap)
{
    if (!buf || cap < 1 || batch < 1 || iw < 1 || ih < 1 || stride < 1) { ffgpu_set_error("irb_s2_launch_text: bad arguments"); return -1; }
    IrbDesc d{};
    irb_fill(d, batch, iw, ih, ic, ec, oc, stride, act1, actd, act2, res_act);
    d.flags = flags & FFGPU_CONCURRENT;
    (void)ffgpu_irb_plan(d);
    return ffgpu_irb_s2_launch_line(d, buf, (size_t)cap);
}

extern "C" float ffgpu_irb_dev(const float *d_in, const float *d_w1, const float *d_wd, const float *d_w2,
                               const float *d_res, float *d_out, int batch, int iw, int ih, int ic, int ec, int oc,
                               int stride, int act1, int actd, int act2, int res_act, int warmup, int iters, void *stream)
{
    return ffgpu_irb_flags_dev(d_in, d_w1, d_wd, d_w2, d_res, d_out, batch, iw, ih, ic, ec, oc, stride, act1, actd, act2, res_act, 0, warmup, iters, stream);
}

// the same block as an executor created with `flags` (FFGPU_CONCURRENT or 0) plans and launches it
extern "C" float ffgpu_irb_flags_dev(const float *d_in, const float *d_w1, const float *d_wd, const float *d_w2,
                                     const float *d_res, float *d_out, int batch, int iw, int ih, int ic, int ec, int oc,
                                     int stride, int act1, int actd, int act2, int res_act, int flags, int warmup, int iters, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    IrbDesc d{};
    d.in = d_in; d.out = d_out; d.residual = d_res; d.w1 = d_w1; d.wd = d_wd; d.w2 = d_w2;
    irb_fill(d, batch, iw, ih, ic, ec, oc, stride, act1, actd, act2, res_act);
    d.flags = flags & FFGPU_CONCURRENT;
    if (!d_in || !d_out || !d_w1 || !d_wd || !d_w2 || !ffgpu_irb_plan(d)) { ffgpu_set_error("irb_dev: unsupported block shape"); return -1.f; }     // planned once per call
    float *pk = nullptr;
    if (hipMalloc(&pk, ffgpu_irb_pack_floats(d) * sizeof(float)) != hipSuccess) { ffgpu_set_error("irb_dev: hipMalloc failed"); return -1.f; }
    d.pk = pk;
    float us = 0.f;
    int rc = ffgpu_irb_pack(d, pk, s);
    if (!rc && iters <= 0) rc = ffgpu_launch_irb(d, s);
    if (!rc && iters > 0) {
        hipEvent_t e0, e1;
        (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
        for (int i = 0; i < warmup && !rc; i++) rc = ffgpu_launch_irb(d, s);
        (void)hipEventRecord(e0, s);
        for (int i = 0; i < iters && !rc; i++) rc = ffgpu_launch_irb(d, s);
        (void)hipEventRecord(e1, s);
        (void)hipEventSynchronize(e1);
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        us = ms * 1000.f / iters;
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    }
    (void)hipStreamSynchronize(s);
    (void)hipFree(pk);
    return rc ? -1.f : us;
}

// depthwise K x K (stride 1, same padding) + pointwise 1x1 in one launch: two consecutive groupconv calls of the reference;
// d_wd / d_wp are the two layers' filter rows (conv.h layout).  iters > 0: mean microseconds per launch instead of 0.
extern "C" float ffgpu_dwpw_dev(const float *d_in, const float *d_wd, const float *d_wp, float *d_out, int batch, int iw, int ih,
                                int c, int oc, int fs, int actd, int actp, int warmup, int iters, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    ConvDesc dw, pw;
    fill_desc(dw, d_in, d_wd, nullptr, batch, iw, ih, c, c, fs / 2, 1, fs, iw, ih, c, actd, 0);
    fill_desc(pw, nullptr, d_wp, d_out, batch, iw, ih, c, 1, 0, 1, 1, iw, ih, oc, actp, 0);
    if (!d_in || !d_wd || !d_wp || !d_out || !ffgpu_dwpw_ok(dw, pw)) { ffgpu_set_error("dwpw_dev: unsupported layer pair"); return -1.f; }
    float *pk = nullptr;
    if (hipMalloc(&pk, ffgpu_dwpw_pack_floats(dw, pw) * sizeof(float)) != hipSuccess) { ffgpu_set_error("dwpw_dev: hipMalloc failed"); return -1.f; }
    float us = 0.f;
    int rc = ffgpu_dwpw_pack(dw, pw, pk, s);
    if (!rc && iters <= 0) rc = ffgpu_launch_dwpw(dw, pw, pk, s);
    if (!rc && iters > 0) {
        hipEvent_t e0, e1;
        (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
        for (int i = 0; i < warmup && !rc; i++) rc = ffgpu_launch_dwpw(dw, pw, pk, s);
        (void)hipEventRecord(e0, s);
        for (int i = 0; i < iters && !rc; i++) rc = ffgpu_launch_dwpw(dw, pw, pk, s);
        (void)hipEventRecord(e1, s);
        (void)hipEventSynchronize(e1);
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        us = ms * 1000.f / iters;
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    }
    (void)hipStreamSynchronize(s);
    (void)hipFree(pk);
    return rc ? -1.f : us;
}

// -------------------------------------------------------------------------- conv.h drop-in (host pointers)
// Literal replacement for a conv-vN.c object: stages through device scratch that
// grows on demand and is kept for the life of the process (one per thread).
struct HostConvScratch { float *in = nullptr, *filt = nullptr, *out = nullptr; size_t in_n = 0, filt_n = 0, out_n = 0; int dev = -1; };

static int grow(float **p, size_t *have, size_t need)
{
    if (*have >= need) return 0;
    (void)hipFree(*p);
    *p = nullptr; *have = 0;
    FFGPU_CHECK(hipMalloc(p, need * sizeof(float)));
    *have = need;
    return 0;
}

extern "C" void groupconv(float *in, float *filt, float *out,
                          int iw, int ih, int ic, int ig, int ipad, int istride,
                          int fs, int fn, int ow, int oh, int oc, int act,
                          float **scratch, int *scratch_floats)
{
    static thread_local HostConvScratch sc;
    (void)scratch; (void)scratch_floats;          // the reference's callee-grown host scratch is not needed
    if (!in || !filt || !out || ig < 1 || ic % ig) { fprintf(stderr, "ffcnn groupconv: bad arguments\n"); return; }
    const size_t n_in = (size_t)iw * ih * ic, n_out = (size_t)ow * oh * oc;
    const size_t n_f = (size_t)fn * ((((size_t)fs * fs * (ic / ig) + 3) & ~(size_t)3) + 4);
    const int flags = knob(K_COMPAT_V6) ? FFGPU_COMPAT_V6 : 0;
    int cur = 0;
    (void)hipGetDevice(&cur);
    if (sc.dev != cur) {                          // the thread moved to another GPU (ffgpu_set_device): the buffers stay behind
        (void)hipFree(sc.in); (void)hipFree(sc.filt); (void)hipFree(sc.out);
        sc = HostConvScratch();
        sc.dev = cur;
    }
    int rc = grow(&sc.in, &sc.in_n, n_in) || grow(&sc.filt, &sc.filt_n, n_f) || grow(&sc.out, &sc.out_n, n_out);
    if (!rc) rc = copy_h2d(sc.in, in, n_in * sizeof(float)) || copy_h2d(sc.filt, filt, n_f * sizeof(float));   // (staged: DESIGN.md section 10)
    if (!rc) rc = ffgpu_groupconv_dev(sc.in, sc.filt, sc.out, 1, iw, ih, ic, ig, ipad, istride, fs, fn, ow, oh, oc, act, flags, FFGPU_K_AUTO, nullptr);
    if (!rc) rc = hipStreamSynchronize(nullptr) != hipSuccess || copy_d2h(out, sc.out, n_out * sizeof(float));
    if (rc) fprintf(stderr, "ffcnn groupconv: device path failed: %s\n", g_err[0] ? g_err : hipGetErrorString(hipGetLastError()));
}
