// ffgpu_node.inc -- the forward path on ALL GPUs of one node from ONE C process (included by ffgpu_exec.hip).
//
// SURVEY.md section 8(e) / north_star: "A batch of independent frames shards across the 8 GPUs of one node with an RCCL
// broadcast of weights and a gather of detections over xGMI ... host code stays in C".  net_forward has no cross-frame
// state (ffcnn.c:476-520), so the batch is cut into contiguous shards, one per device; every device holds its own copy of
// the folded filter rows and runs the whole net on its shard.  Exactly two exchanges exist:
//   * once, at ffgpu_node_create: ncclBroadcast of NET.weight_buf's device copy (356 576 floats for yolo-fastest) from
//     rank 0 to every other device (their copies start zeroed: what they compute with really arrived over RCCL);
//   * per forward: the shards' detection records travel to rank 0 in their COMPACT form (ffgpu_pack_records: header, four
//     ints per frame, the boxes behind each other -- ~13 KB instead of 99 KB for a 32-frame shard) -- one grouped ncclSend /
//     ncclRecv per peer (a gather; RCCL has no ncclGather) --, from there in ONE copy to pinned host memory, and
//     ffgpu_node_wait unpacks them into the caller's buffer of fixed-size records in global frame order.  A shard whose
//     frames hold more boxes than its block has room for (FFGPU_NODE_PACK_BOXES per frame on average) is fetched again in
//     full by ffgpu_node_wait: nothing is ever lost, the rare case only costs a copy.
//     With ONE device there is no exchange: FFGPU_HOST_DETS executors mirror the records into pinned host memory themselves.
// One host thread drives all devices (launches are asynchronous; each device has its own streams and HIP graphs); one
// communicator per device from ncclCommInitAll.  Up to DEPTH steps are in flight (FFGPU_NODE_DEPTH(n) in node_flags): slot
// s = step % DEPTH has its own executor, compute stream and input buffer on every device and its own gather / host buffers,
// ffgpu_node_submit enqueues a step and returns, ffgpu_node_wait(ticket) hands over its records; the exchange of a step runs
// on a per-device communication stream behind an event, so the next steps' kernels are not held up by it.  RCCL is resolved at run time (dlopen): libffcnn_hip.so has no link-time
// dependency on it, a single-GPU user never loads it, and a process that already carries an RCCL (e.g. through PyTorch)
// uses that one instead of a second copy.
// FFGPU_NODE_LOOPBACK replaces the two RCCL calls by peer copies on the same streams: it lets the whole multi-rank path
// (shards, per-rank executors, gather offsets, frame order) run with several ranks on ONE device, which is how the GPU
// tests cover it on a single-GPU box.
#include <dlfcn.h>
#include <rccl/rccl.h>

#define FFGPU_NODE_PACK_BOXES 16        // room in a shard's packed block: this many boxes per frame on average

struct RcclApi {
    void *handle = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*Broadcast)(const void *, void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};

static const RcclApi *rccl_api()
{
    static RcclApi api;
    static bool tried = false;
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    if (tried) return api.CommInitAll ? &api : nullptr;
    tried = true;
    // an RCCL already in the process (PyTorch brings its own) wins: its symbols are resolved through the global scope
    // (RTLD_DEFAULT is a null handle on glibc, so "found in the process" is its own flag); else the ROCm one, kept private
    const bool in_process = dlsym(RTLD_DEFAULT, "ncclCommInitAll") != nullptr;
    void *h = nullptr;
    if (!in_process) {
        for (const char *name : { "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1" }) {
            h = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (h) { api.handle = h; break; }
        }
        if (!h) { ffgpu_set_error("RCCL not found (librccl.so.1): %s", dlerror()); return nullptr; }
    }
#define RCCL_SYM(field, name) api.field = reinterpret_cast<decltype(api.field)>(dlsym(in_process ? RTLD_DEFAULT : h, name))
    RCCL_SYM(CommInitAll, "ncclCommInitAll"); RCCL_SYM(CommDestroy, "ncclCommDestroy"); RCCL_SYM(Broadcast, "ncclBroadcast");
    RCCL_SYM(Send, "ncclSend"); RCCL_SYM(Recv, "ncclRecv"); RCCL_SYM(GroupStart, "ncclGroupStart"); RCCL_SYM(GroupEnd, "ncclGroupEnd");
    RCCL_SYM(GetErrorString, "ncclGetErrorString");
#undef RCCL_SYM
    if (!api.CommInitAll || !api.CommDestroy || !api.Broadcast || !api.Send || !api.Recv || !api.GroupStart || !api.GroupEnd) {
        api.CommInitAll = nullptr;
        ffgpu_set_error("RCCL library lacks a required entry point");
        return nullptr;
    }
    return &api;
}

#define RCCL_CHECK(api, expr)                                                                            \
    do {                                                                                                 \
        ncclResult_t r_ = (expr);                                                                        \
        if (r_ != ncclSuccess) {                                                                         \
            ffgpu_set_error("%s failed: %s", #expr, (api)->GetErrorString ? (api)->GetErrorString(r_) : "?"); \
            return -1;                                                                                   \
        }                                                                                                \
    } while (0)

// contiguous frames [lo, hi) of `rank`: sizes differ by at most one, earlier ranks take the extra
extern "C" void ffgpu_shard_range(int total, int rank, int world, int *lo, int *hi)
{
    if (world < 1) world = 1;
    const int base = total / world, extra = total % world;
    const int a = rank * base + std::min(rank, extra);
    if (lo) *lo = a;
    if (hi) *hi = a + base + (rank < extra ? 1 : 0);
}

struct ffgpu_node {
    NET *net = nullptr;
    int  ndev = 0, total = 0, node_flags = 0, depth = 1;
    size_t frame_floats = 0;
    const RcclApi *rccl = nullptr;
    struct Rank {
        int device = 0, lo = 0, hi = 0;
        ffgpu_netdev *nd = nullptr; bool own_nd = false;
        ncclComm_t comm = nullptr;
        hipStream_t comm_st = nullptr;              // the exchange of every step, in step order
        std::vector<ffgpu_exec *> ex;               // per slot
        std::vector<hipStream_t> st;                // per slot: compute
        std::vector<float *> d_in;                  // per slot: the shard's frames (frame-major), owned by the node
        std::vector<hipEvent_t> ev_done;            // per slot: "this rank's records of the step are final"
        std::vector<float *> h_in;                  // per slot: page-locked staging of the shard's frames (ffgpu_node_submit from caller memory)
        std::vector<unsigned char *> d_pack;        // per slot, ranks > 0: the shard's packed records (what travels)
        int pack_cap = 0; size_t pack_bytes = 0, pack_off = 0;     // boxes a block holds, its size, its offset in the gather block
    };
    std::vector<Rank> rk;
    std::vector<unsigned char *> d_gather;          // per slot, on rank 0's device: the ranks' packed blocks behind each other
    std::vector<unsigned char *> h_gather;          // per slot, pinned
    size_t gather_bytes = 0;
    std::vector<hipEvent_t> ev_host;                // per slot: the records are in h_gather
    std::vector<long> ticket;                       // per slot: step in flight / waiting to be collected (-1: free)
    long next_step = 0;
    std::vector<ffgpu_frame_dets> scratch_out;      // ffgpu_node_run: where the records of all but the last step go
    bool direct = false;                            // one device: the executors' NMS kernels write the records into pinned host memory themselves
};

extern "C" void ffgpu_node_destroy(ffgpu_node *nd)
{
    if (!nd) return;
    int cur = 0;
    (void)hipGetDevice(&cur);
    for (auto &r : nd->rk) {
        (void)hipSetDevice(r.device);
        for (hipStream_t st : r.st) if (st) (void)hipStreamSynchronize(st);
        if (r.comm_st) (void)hipStreamSynchronize(r.comm_st);
    }
    for (auto &r : nd->rk) {
        (void)hipSetDevice(r.device);
        for (ffgpu_exec *ex : r.ex) if (ex) ffgpu_exec_destroy(ex);
        if (r.comm && nd->rccl) (void)nd->rccl->CommDestroy(r.comm);
        (void)hipSetDevice(r.device);
        for (float *p : r.d_in) if (p) (void)hipFree(p);
        for (unsigned char *p : r.d_pack) if (p) (void)hipFree(p);
        for (float *p : r.h_in) if (p) (void)hipHostFree(p);
        for (hipEvent_t e : r.ev_done) if (e) (void)hipEventDestroy(e);
        for (hipStream_t st : r.st) if (st) (void)hipStreamDestroy(st);
        if (r.comm_st) (void)hipStreamDestroy(r.comm_st);
        if (r.own_nd && r.nd) ffgpu_netdev_destroy(r.nd);
    }
    if (!nd->rk.empty()) (void)hipSetDevice(nd->rk[0].device);
    for (auto p : nd->d_gather) if (p) (void)hipFree(p);
    for (auto p : nd->h_gather) if (p) (void)hipHostFree(p);
    for (auto e : nd->ev_host) if (e) (void)hipEventDestroy(e);
    (void)hipSetDevice(cur);
    delete nd;
}

static int node_broadcast_weights(ffgpu_node *nd)
{
    const size_t nfl = (size_t)nd->net->weight_size;
    if (nd->ndev == 1 || nfl == 0) return 0;
    if (nd->node_flags & FFGPU_NODE_LOOPBACK) {
        for (int r = 1; r < nd->ndev; r++) {
            FFGPU_CHECK(hipSetDevice(nd->rk[r].device));
            FFGPU_CHECK(hipMemcpyPeerAsync(nd->rk[r].nd->d_weights, nd->rk[r].device, nd->rk[0].nd->d_weights, nd->rk[0].device,
                                           nfl * sizeof(float), nd->rk[r].comm_st));
        }
    } else {
        RCCL_CHECK(nd->rccl, nd->rccl->GroupStart());
        for (int r = 0; r < nd->ndev; r++) {
            FFGPU_CHECK(hipSetDevice(nd->rk[r].device));
            RCCL_CHECK(nd->rccl, nd->rccl->Broadcast(nd->rk[r].nd->d_weights, nd->rk[r].nd->d_weights, nfl, ncclFloat, 0, nd->rk[r].comm, nd->rk[r].comm_st));
        }
        RCCL_CHECK(nd->rccl, nd->rccl->GroupEnd());
    }
    for (int r = 0; r < nd->ndev; r++) { FFGPU_CHECK(hipSetDevice(nd->rk[r].device)); FFGPU_CHECK(hipStreamSynchronize(nd->rk[r].comm_st)); }
    return 0;
}

extern "C" ffgpu_node *ffgpu_node_create(NET *net, int ndev, const int *devices, int global_batch, int exec_flags, int node_flags)
{
    ffgpu_netdev *dev0 = netdev_of(net);
    if (!dev0) return nullptr;
    int have = 0;
    (void)hipGetDeviceCount(&have);
    if (ndev < 1 || global_batch < ndev) { ffgpu_set_error("node_create: need ndev >= 1 and at least one frame per device"); return nullptr; }
    const bool loop = (node_flags & FFGPU_NODE_LOOPBACK) != 0;
    const int depth = std::max(1, std::min((node_flags >> 8) & 0xf, 8));
    int cur = 0;
    (void)hipGetDevice(&cur);
    ffgpu_node *nd = new ffgpu_node();
    nd->net = net; nd->ndev = ndev; nd->total = global_batch; nd->node_flags = node_flags; nd->depth = depth;
    nd->frame_floats = (size_t)net->layer_list[0].c * net->layer_list[0].h * net->layer_list[0].w;
    nd->rk.resize(ndev);
    nd->d_gather.assign(depth, nullptr); nd->h_gather.assign(depth, nullptr); nd->ev_host.assign(depth, nullptr); nd->ticket.assign(depth, -1);
    std::vector<int> devlist(ndev);
    for (int r = 0; r < ndev; r++) {
        // default placement: rank 0 on the device the net was loaded on, the others on the next devices (loopback: all on it)
        const int d = devices ? devices[r] : (loop ? dev0->device : (dev0->device + r) % std::max(have, 1));
        if (d < 0 || d >= have) { ffgpu_set_error("node_create: device %d does not exist (%d visible)", d, have); ffgpu_node_destroy(nd); return nullptr; }
        for (int q = 0; q < r && !loop; q++)
            if (devlist[q] == d) { ffgpu_set_error("node_create: device %d used twice (RCCL wants one rank per device; FFGPU_NODE_LOOPBACK allows it)", d); ffgpu_node_destroy(nd); return nullptr; }
        devlist[r] = d;
        ffgpu_node::Rank &k = nd->rk[r];
        k.device = d;
        k.ex.assign(depth, nullptr); k.st.assign(depth, nullptr); k.d_in.assign(depth, nullptr); k.ev_done.assign(depth, nullptr);
        k.d_pack.assign(depth, nullptr); k.h_in.assign(depth, nullptr);
        ffgpu_shard_range(global_batch, r, ndev, &k.lo, &k.hi);
        if (k.hi - k.lo > 1024) { ffgpu_set_error("node_create: a shard of %d frames (the packed records hold at most 1024)", k.hi - k.lo); ffgpu_node_destroy(nd); return nullptr; }
        const int pb = knob(K_NODE_PACK_BOXES);                    // (tests: force the "block too small" path)
        k.pack_cap = std::max(1, pb > 0 ? pb : FFGPU_NODE_PACK_BOXES) * (k.hi - k.lo);
        k.pack_bytes = ffgpu_packed_records_bytes(k.hi - k.lo, k.pack_cap);
        k.pack_off = nd->gather_bytes;
        nd->gather_bytes += k.pack_bytes;
    }
    if (!loop && ndev > 1 && devlist[0] != dev0->device) { ffgpu_set_error("node_create: rank 0 must be the device the net was loaded on (%d)", dev0->device); ffgpu_node_destroy(nd); return nullptr; }
    auto fail = [&](const char *what) -> ffgpu_node * {
        if (what) ffgpu_set_error("node_create: %s: %s", what, hipGetErrorString(hipGetLastError()));
        ffgpu_node_destroy(nd);
        (void)hipSetDevice(cur);
        return nullptr;
    };
    if (!loop && ndev > 1) {                                        // one device: no exchange exists, RCCL is never loaded
        nd->rccl = rccl_api();
        if (!nd->rccl) return fail(nullptr);
        std::vector<ncclComm_t> comms(ndev, nullptr);
        ncclResult_t r0 = nd->rccl->CommInitAll(comms.data(), ndev, devlist.data());
        if (r0 != ncclSuccess) { ffgpu_set_error("ncclCommInitAll(%d): %s", ndev, nd->rccl->GetErrorString ? nd->rccl->GetErrorString(r0) : "?"); return fail(nullptr); }
        for (int r = 0; r < ndev; r++) nd->rk[r].comm = comms[r];
    }
    for (int r = 0; r < ndev; r++) {
        ffgpu_node::Rank &k = nd->rk[r];
        if (hipSetDevice(k.device) != hipSuccess) return fail("hipSetDevice");
        if (hipStreamCreateWithFlags(&k.comm_st, hipStreamNonBlocking) != hipSuccess) return fail("stream");
        // The compute streams are PRIORITY streams: the runtime keeps one pool of (at most four) hardware queues per priority level,
        // so they get queues of their own, whatever other streams the process holds.  Created at the default priority they share
        // the application's pool, and which of them end up behind each other on one hardware queue depends on how many streams
        // were created before them -- measured on one device, four steps in flight: 136 k frames/s, 180 k when two more streams
        // (RCCL's, or any) happened to exist first, 180-183 k with priority streams in every such setting (DESIGN.md section 6).
        int prio_lo = 0, prio_hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
        for (int s = 0; s < depth; s++)
            if (hipStreamCreateWithPriority(&k.st[s], hipStreamNonBlocking, prio_hi) != hipSuccess || hipEventCreateWithFlags(&k.ev_done[s], hipEventDisableTiming) != hipSuccess ||
                hipMalloc(&k.d_in[s], sizeof(float) * nd->frame_floats * (size_t)(k.hi - k.lo)) != hipSuccess ||
                (r > 0 && hipMalloc(&k.d_pack[s], k.pack_bytes) != hipSuccess)) return fail("per-slot resources");
        // rank 0 computes with the copy net_load made; every other rank gets a zeroed copy that the broadcast fills
        if (r == 0 && k.device == dev0->device) k.nd = dev0;
        else { k.nd = netdev_create_on(net, k.device, false); k.own_nd = true; if (!k.nd) return fail(nullptr); }
        if (r == 0 && k.own_nd &&
            copy_h2d(k.nd->d_weights, net->weight_buf, sizeof(float) * (size_t)net->weight_size)) return fail(nullptr);
    }
    if (node_broadcast_weights(nd)) return fail(nullptr);
    for (int r = 0; r < ndev; r++) {                               // executors pack their constants from the broadcast weights
        ffgpu_node::Rank &k = nd->rk[r];
        if (hipSetDevice(k.device) != hipSuccess) return fail("hipSetDevice");
        for (int s = 0; s < depth; s++) {
            // one device: no exchange at all -- FFGPU_HOST_DETS executors (the NMS kernel mirrors the records into pinned host memory)
            k.ex[s] = exec_create_on(k.nd, net, k.hi - k.lo, (exec_flags & ~(FFGPU_HOST_DETS | FFGPU_KEEP_ALL)) | (ndev == 1 ? FFGPU_HOST_DETS : 0));
            if (!k.ex[s]) return fail(nullptr);
        }
    }
    if (hipSetDevice(nd->rk[0].device) != hipSuccess) return fail("hipSetDevice");
    for (int s = 0; s < depth; s++)
        if (hipMalloc(&nd->d_gather[s], nd->gather_bytes) != hipSuccess ||
            hipHostMalloc(&nd->h_gather[s], nd->gather_bytes, hipHostMallocDefault) != hipSuccess ||
            hipEventCreateWithFlags(&nd->ev_host[s], hipEventDisableTiming) != hipSuccess) return fail("gather buffers");
    nd->direct = ndev == 1;
    (void)hipSetDevice(cur);
    return nd;
}

extern "C" int ffgpu_node_ndev(const ffgpu_node *nd) { return nd ? nd->ndev : 0; }
extern "C" int ffgpu_node_depth(const ffgpu_node *nd) { return nd ? nd->depth : 0; }
// communicators ncclCommInitAll really created for this node (0: one device or FFGPU_NODE_LOOPBACK -- RCCL never loaded)
extern "C" int ffgpu_node_rccl_ranks(const ffgpu_node *nd)
{
    int n = 0;
    if (nd && nd->rccl) for (const auto &r : nd->rk) n += r.comm != nullptr;
    return n;
}

extern "C" int ffgpu_node_shard(const ffgpu_node *nd, int rank, int *lo, int *hi, int *device)
{
    if (!nd || rank < 0 || rank >= nd->ndev) { ffgpu_set_error("node_shard: bad rank"); return -1; }
    if (lo) *lo = nd->rk[rank].lo;
    if (hi) *hi = nd->rk[rank].hi;
    if (device) *device = nd->rk[rank].device;
    return 0;
}

extern "C" float *ffgpu_node_input_slot_dev(ffgpu_node *nd, int rank, int slot)
{
    if (!nd || rank < 0 || rank >= nd->ndev || slot < 0 || slot >= nd->depth) { ffgpu_set_error("node_input_dev: bad rank / slot"); return nullptr; }
    return nd->rk[rank].d_in[slot];
}
// the input buffer the NEXT submitted step will read on `rank`
extern "C" float *ffgpu_node_input_dev(ffgpu_node *nd, int rank) { return ffgpu_node_input_slot_dev(nd, rank, nd ? (int)(nd->next_step % nd->depth) : 0); }

extern "C" int ffgpu_node_set_scale(ffgpu_node *nd, int s1, int s2)
{
    if (!nd || s2 == 0) { ffgpu_set_error("node_set_scale: bad arguments"); return -1; }
    for (auto &r : nd->rk) for (ffgpu_exec *ex : r.ex) { ex->s1 = s1; ex->s2 = s2; }
    return 0;
}

// Enqueue the next step (number returned = its ticket; slot = ticket % depth): forward on every device from the slot's
// input buffers -- h_frames (global_batch x C x H x W fp32, may be NULL) is copied into them first --, then, on the
// communication streams, the gather of the records on rank 0 and their copy to the slot's pinned host buffer.  Returns
// without waiting; fails if the slot still holds a step that was not collected with ffgpu_node_wait.
// host side of ffgpu_pack_records: one block -> `batch` fixed-size records (unused box slots zero, like the NMS kernel leaves
// them).  Returns 1 if the block had dropped boxes (header `over`), 0 otherwise.
static int node_unpack_block(const unsigned char *blk, int batch, int cap, ffgpu_frame_dets *out)
{
    const int *hdr = reinterpret_cast<const int *>(blk);
    const int *fr = hdr + 4;
    const BBOX *box = reinterpret_cast<const BBOX *>(fr + 4 * (size_t)batch);
    if (hdr[1] || hdr[2] != batch || hdr[3] != cap) return 1;    // (a malformed block is fetched again in full as well)
    int first = 0;
    for (int n = 0; n < batch; n++) {
        const int kept = std::max(0, std::min(fr[4 * n], FFGPU_MAX_DET));
        out[n].count = kept; out[n].ncand = fr[4 * n + 1]; out[n].overflow = fr[4 * n + 2]; out[n].nfull = fr[4 * n + 3];
        if (first + kept > cap) return 1;
        memcpy(out[n].box, box + first, sizeof(BBOX) * (size_t)kept);
        memset(out[n].box + kept, 0, sizeof(BBOX) * (size_t)(FFGPU_MAX_DET - kept));
        first += kept;
    }
    return 0;
}

// the same for any caller that gathers packed blocks itself (e.g. one process per GPU): pure host code, no device needed
extern "C" int ffgpu_unpack_records(const void *block, int batch, int cap, ffgpu_frame_dets *out)
{
    if (!block || !out || batch < 1 || cap < 1) { ffgpu_set_error("unpack_records: bad arguments"); return -1; }
    return node_unpack_block(static_cast<const unsigned char *>(block), batch, cap, out);
}

// (the body: any early return leaves `*in_group` telling whether an RCCL group is still open)
static int node_submit_step(ffgpu_node *nd, const float *h_frames, int s, bool *in_group)
{
    const bool loop = (nd->node_flags & FFGPU_NODE_LOOPBACK) != 0;
    for (int r = 0; r < nd->ndev; r++) {                            // every device starts its shard; nothing waits yet
        ffgpu_node::Rank &k = nd->rk[r];
        FFGPU_CHECK(hipSetDevice(k.device));
        if (!alive(k.ex[s], "node_submit")) return -1;
        if (h_frames) {
            // caller memory goes through the slot's page-locked staging buffer (allocated on the first such call): the device never
            // maps the caller's pages, and the caller's buffer is free again when submit returns
            const size_t bytes = sizeof(float) * nd->frame_floats * (size_t)(k.hi - k.lo);
            const float *src = h_frames + (size_t)k.lo * nd->frame_floats;
            if (!pinned_ours(src, bytes)) {
                if (!k.h_in[s]) FFGPU_CHECK(hipHostMalloc((void **)&k.h_in[s], bytes, hipHostMallocDefault));
                memcpy(k.h_in[s], src, bytes);                      // (the slot is free: its previous upload has completed)
                src = k.h_in[s];
            }
            FFGPU_CHECK(hipMemcpyAsync(k.d_in[s], src, bytes, hipMemcpyHostToDevice, k.st[s]));
        }
        if (forward_on(k.ex[s], fp32_src(k.d_in[s]), k.st[s])) return -1;
        if (nd->direct) { FFGPU_CHECK(hipEventRecord(nd->ev_host[s], k.st[s])); return 0; }   // the records are on the host when the step ends
        FFGPU_CHECK(hipEventRecord(k.ev_done[s], k.st[s]));
        FFGPU_CHECK(hipStreamWaitEvent(k.comm_st, k.ev_done[s], 0));
    }
    // every rank packs its shard's records on its communication stream (rank 0 straight into the gather block)
    ffgpu_node::Rank &k0 = nd->rk[0];
    for (int r = 0; r < nd->ndev; r++) {
        ffgpu_node::Rank &k = nd->rk[r];
        FFGPU_CHECK(hipSetDevice(k.device));
        if (ffgpu_pack_records(k.ex[s]->d_dets, 1, k.hi - k.lo, k.hi - k.lo, k.pack_cap,
                               r == 0 ? nd->d_gather[s] + k.pack_off : k.d_pack[s], k.comm_st)) return -1;
    }
    if (loop) {
        FFGPU_CHECK(hipSetDevice(k0.device));
        for (int r = 1; r < nd->ndev; r++) {
            ffgpu_node::Rank &k = nd->rk[r];
            FFGPU_CHECK(hipEventRecord(k.ev_done[s], k.comm_st));   // (now: "this rank's block is packed")
            FFGPU_CHECK(hipStreamWaitEvent(k0.comm_st, k.ev_done[s], 0));
            FFGPU_CHECK(hipMemcpyPeerAsync(nd->d_gather[s] + k.pack_off, k0.device, k.d_pack[s], k.device, k.pack_bytes, k0.comm_st));
        }
    } else if (nd->ndev > 1) {
        // gather = one send per peer, the matching receives on rank 0, fused into one RCCL group (point-to-point over xGMI)
        RCCL_CHECK(nd->rccl, nd->rccl->GroupStart());
        *in_group = true;
        for (int r = 1; r < nd->ndev; r++) {
            ffgpu_node::Rank &k = nd->rk[r];
            FFGPU_CHECK(hipSetDevice(k.device));
            RCCL_CHECK(nd->rccl, nd->rccl->Send(k.d_pack[s], k.pack_bytes, ncclChar, 0, k.comm, k.comm_st));
            FFGPU_CHECK(hipSetDevice(k0.device));
            RCCL_CHECK(nd->rccl, nd->rccl->Recv(nd->d_gather[s] + k.pack_off, k.pack_bytes, ncclChar, r, k0.comm, k0.comm_st));
        }
        *in_group = false;
        RCCL_CHECK(nd->rccl, nd->rccl->GroupEnd());
    }
    FFGPU_CHECK(hipSetDevice(k0.device));
    FFGPU_CHECK(hipMemcpyAsync(nd->h_gather[s], nd->d_gather[s], nd->gather_bytes, hipMemcpyDeviceToHost, k0.comm_st));
    FFGPU_CHECK(hipEventRecord(nd->ev_host[s], k0.comm_st));
    return 0;
}

extern "C" long ffgpu_node_submit(ffgpu_node *nd, const float *h_frames)
{
    if (!nd) { ffgpu_set_error("node_submit: NULL node"); return -1; }
    const long step = nd->next_step;
    const int s = (int)(step % nd->depth);
    if (nd->ticket[s] >= 0) { ffgpu_set_error("node_submit: step %ld of slot %d has not been collected (ffgpu_node_wait)", nd->ticket[s], s); return -1; }
    int cur = 0;
    (void)hipGetDevice(&cur);
    bool in_group = false;
    const int rc = node_submit_step(nd, h_frames, s, &in_group);
    if (in_group) (void)nd->rccl->GroupEnd();                       // an error inside the group: close it (the error text of the first failure stays)
    (void)hipSetDevice(cur);                                        // on every path the caller's current device is what it was
    if (rc) return -1;
    nd->ticket[s] = step;
    nd->next_step = step + 1;
    return step;
}

// wait for step `ticket` and copy its global_batch records (frame order) to host_out; frees the slot
extern "C" int ffgpu_node_wait(ffgpu_node *nd, long ticket, ffgpu_frame_dets *host_out)
{
    if (!nd || !host_out || ticket < 0) { ffgpu_set_error("node_wait: bad arguments"); return -1; }
    const int s = (int)(ticket % nd->depth);
    if (nd->ticket[s] != ticket) { ffgpu_set_error("node_wait: step %ld is not in flight", ticket); return -1; }
    FFGPU_CHECK(hipEventSynchronize(nd->ev_host[s]));
    if (nd->ndev > 1 && !(nd->node_flags & FFGPU_NODE_LOOPBACK)) {   // the peers' sends of this step have completed with the receives;
        int cur = 0;                                                 // make that explicit before their executors run again
        (void)hipGetDevice(&cur);
        for (int r = 1; r < nd->ndev; r++) { FFGPU_CHECK(hipSetDevice(nd->rk[r].device)); FFGPU_CHECK(hipStreamSynchronize(nd->rk[r].comm_st)); }
        (void)hipSetDevice(cur);
    }
    if (nd->direct) memcpy(host_out, nd->rk[0].ex[s]->h_dets, sizeof(ffgpu_frame_dets) * (size_t)nd->total);
    else {
        int cur = 0;
        (void)hipGetDevice(&cur);
        for (int r = 0; r < nd->ndev; r++) {
            const ffgpu_node::Rank &k = nd->rk[r];
            if (node_unpack_block(nd->h_gather[s] + k.pack_off, k.hi - k.lo, k.pack_cap, host_out + k.lo) == 1) {
                // more boxes than the block holds: this shard's full-size records, straight from its device (its executor
                // cannot have run again: the slot is still taken)
                hipError_t e = hipSetDevice(k.device);
                const int rc = e == hipSuccess ? copy_d2h(host_out + k.lo, k.ex[s]->d_dets, sizeof(ffgpu_frame_dets) * (size_t)(k.hi - k.lo)) : -1;
                (void)hipSetDevice(cur);
                if (e != hipSuccess) ffgpu_set_error("node_wait: hipSetDevice(%d): %s", k.device, hipGetErrorString(e));
                if (rc) return -1;
            }
        }
    }
    nd->ticket[s] = -1;
    return 0;
}

// `steps` steps from the slots' input buffers with the node's full depth in flight -- the loop a C host runs (collect step i - depth,
// submit step i), as one call; host_out (may be NULL) receives the records of the LAST step.  No step may be outstanding on entry.
extern "C" int ffgpu_node_run(ffgpu_node *nd, long steps, ffgpu_frame_dets *host_out)
{
    if (!nd || steps < 0) { ffgpu_set_error("node_run: bad arguments"); return -1; }
    for (long t : nd->ticket) if (t >= 0) { ffgpu_set_error("node_run: step %ld is still outstanding (ffgpu_node_wait)", t); return -1; }
    if (nd->scratch_out.size() < (size_t)nd->total) nd->scratch_out.resize((size_t)nd->total);
    std::vector<long> tick((size_t)nd->depth, -1);
    int rc = 0;
    for (long i = 0; i < steps + nd->depth && !rc; i++) {
        if (i >= nd->depth && i - nd->depth < steps &&
            ffgpu_node_wait(nd, tick[i % nd->depth], (i - nd->depth == steps - 1 && host_out) ? host_out : nd->scratch_out.data())) { rc = -1; break; }
        if (i < steps && (tick[i % nd->depth] = ffgpu_node_submit(nd, nullptr)) < 0) rc = -1;
    }
    if (rc) {
        // a submit or wait failed mid-loop: the caller never saw the tickets still in flight, so collect them here (results
        // dropped, the first failure's text kept) -- the node stays usable instead of refusing every later run with
        // "step still outstanding"
        std::string first = ffgpu_last_error();
        int cur = 0;
        (void)hipGetDevice(&cur);
        for (auto &r : nd->rk) {
            (void)hipSetDevice(r.device);
            for (hipStream_t st : r.st) if (st) (void)hipStreamSynchronize(st);
            if (r.comm_st) (void)hipStreamSynchronize(r.comm_st);
        }
        (void)hipSetDevice(cur);
        for (long &t : nd->ticket) t = -1;
        ffgpu_set_error("%s", first.c_str());
    }
    return rc;
}

// one step, synchronously, from the slot's input buffers (ffgpu_node_input_dev) ...
extern "C" int ffgpu_node_forward(ffgpu_node *nd, ffgpu_frame_dets *host_out)
{
    const long t = ffgpu_node_submit(nd, nullptr);
    return t < 0 ? -1 : ffgpu_node_wait(nd, t, host_out);
}

// ... or from host memory: h_frames = global_batch x C x H x W fp32 (frame-major); shards are copied to their devices first
extern "C" int ffgpu_node_forward_host(ffgpu_node *nd, const float *h_frames, ffgpu_frame_dets *host_out)
{
    if (!h_frames) { ffgpu_set_error("node_forward_host: NULL argument"); return -1; }
    const long t = ffgpu_node_submit(nd, h_frames);
    return t < 0 ? -1 : ffgpu_node_wait(nd, t, host_out);
}
