// ffgpu_zones.inc -- zones and lines: identified boxes counted, flagged and gated on the device (ffgpu_zones_boxes_dev, ffgpu_exec_zones,
// ffgpu_zones_reset_dev, ffgpu_zones_state_bytes, ffgpu_scene_check).  The contract is in include/ffcnn_hip.h; the host side (checks, grouping by
// stream) is ffgpu_zones_host.hpp.
//
// One workgroup per video stream and launch, as k_track: it loads the stream's scene and state into LDS once, walks the stream's records of the launch
// serially and writes the state back once.  Per frame: the considered boxes are compacted into LDS by ballots (list order kept); lanes 0..127 own the
// boxes, lanes 128..255 the slots.  A box's inside mask is found by eight consecutive lanes, a zone each, and read off the wave's ballot.  A box lane
// computes its anchor, finds out whether an earlier box has its identity and which slot holds it, and, being the only owner that can name that slot,
// updates it in place.  Frees by the slot lanes, fresh owners by ranks (block_rank: the r-th fresh owner takes the r-th free slot), every count of the
// event row by ballots folded in wave order.  No atomic, no arrival order.
struct ZonesArgs {
    StreamEntries<ZONES_ARG_ENTRIES> en;              // the launch's records, grouped by video stream (ffgpu_streams_host.hpp)
    ffgpu_zones_spec spec;
    int   ngroups, pad_[3];
};
static_assert(sizeof(ZonesArgs) + 10 * 8 <= 4096 - 256, "the tables travel as a kernel argument (4 KB at most, the hidden arguments included)");
static_assert(FFGPU_ZONES_DETS == 128 && FFGPU_ZONES_DETS == 2 * WAVE && FFGPU_MAX_DET == FFGPU_ZONES_DETS, "k_zones: waves 0 and 1 own the boxes, waves 2 and 3 the slots");
static_assert(ZONES_STATE_HEADER == 9 * 16 && sizeof(ffgpu_zone_slot) == 4 * 16 && FFGPU_ZONES_ROW == 16 + 4 * FFGPU_SCENE_ZONES + 2 * FFGPU_SCENE_LINES, "k_zones: the layouts of include/ffcnn_hip.h");

struct ZonesLds {
    int4  st[9 + 4 * FFGPU_ZONES_DETS];               // the stream's state as it lies in memory: header, then the slots
    int   sc[sizeof(ffgpu_scene) / 4];                // the stream's scene
    BBOX  det[FFGPU_ZONES_DETS];                      // the considered boxes
    int   didx[FFGPU_ZONES_DETS];                     // box j's index in its list
    int   ident[FFGPU_ZONES_DETS];                    // box j's identity
    int   ins[FFGPU_ZONES_DETS];                      // box j's inside mask
    int   named[FFGPU_ZONES_DETS];                    // slot s: an owner of this frame has its id
    int   freeslot[FFGPU_ZONES_DETS];
    int   cnt[4][FFGPU_ZONES_ROW];                    // wave w's count for word i of the event row
    int   wsum[4], zok[FFGPU_SCENE_ZONES];
};

// a class mask admits a box: all zero admits everything; a box of unknown class is admitted by nothing else
__device__ __forceinline__ bool zones_admits(const unsigned *m, int cls, bool cls_known)
{
    if ((m[0] | m[1] | m[2] | m[3]) == 0) return true;
    return cls_known && cls >= 0 && cls < 128 && ((m[cls >> 5] >> (cls & 31)) & 1u);
}
// the even-odd rule, edge by edge in the contract's words
__device__ __forceinline__ bool zones_inside(const ffgpu_zone &z, float px, float py)
{
#pragma clang fp contract(off)
    const int nv = z.nverts;
    bool in = false;
    for (int i = 0; i < nv; i++) {
        const int j = i + 1 == nv ? 0 : i + 1;
        const float xi = z.x[i], yi = z.y[i], xj = z.x[j], yj = z.y[j];
        if ((yi > py) != (yj > py)) {
            float u = (xj - xi) * (py - yi);
            asm volatile("" : "+v"(u));               // (the two products stay scalar instructions: see box_area in ffgpu_block.inc)
            const float d = u - (px - xi) * (yj - yi);
            if (yj > yi ? d > 0.f : d < 0.f) in = !in;
        }
    }
    return in;
}
__device__ __forceinline__ bool zones_side(float ax, float ay, float bx, float by, float px, float py)
{
#pragma clang fp contract(off)
    float u = (bx - ax) * (py - ay);
    asm volatile("" : "+v"(u));
    return u - (by - ay) * (px - ax) > 0.f;
}
// 0: no crossing; 1: forward; 2: backward
__device__ __forceinline__ int zones_cross(const ffgpu_line &l, float p0x, float p0y, float p1x, float p1y)
{
    const bool s0 = zones_side(l.ax, l.ay, l.bx, l.by, p0x, p0y), s1 = zones_side(l.ax, l.ay, l.bx, l.by, p1x, p1y);
    if (s0 == s1) return 0;
    if (zones_side(p0x, p0y, p1x, p1y, l.ax, l.ay) == zones_side(p0x, p0y, p1x, p1y, l.bx, l.by)) return 0;
    return s1 ? 1 : 2;
}
// this wave's count of the flagged lanes for word i of the event row
__device__ __forceinline__ void zones_count(int (*cnt)[FFGPU_ZONES_ROW], int i, bool flag) { wave_count(cnt, i, flag); }

// grid = groups of the launch, 256 lanes.  Counts are clamped to [0, stride] as the draw kernel clamps them.
__global__ void __launch_bounds__(256) k_zones(ZonesArgs a, const ffgpu_frame_dets *recs, const BBOX *lists, int stride, const unsigned char *scenes,
                                               unsigned char *state, const int *ids, int *events, ffgpu_frame_dets *out_recs, BBOX *out_lists)
{
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) unsigned char s_zones[sizeof(ZonesLds)];
    ZonesLds &L = *reinterpret_cast<ZonesLds *>(s_zones);
    const int tid = threadIdx.x, g = blockIdx.x;
    const int e0 = a.en.goff[g], e1 = a.en.goff[g + 1], vs = a.en.gstream[g], C = a.spec.capacity;
    const long rowlen = FFGPU_ZONES_ROW + 2 * (long)stride, idlen = 8 + (long)stride;
    if (vs < 0) {                                                                     // the ignored entries: every output byte zero (uniform)
        for (int e = e0; e < e1; e++) {
            const long t = a.en.rec[e];
            for (long i = tid; i < rowlen; i += blockDim.x) events[t * rowlen + i] = 0;
            if (out_recs) for (int i = tid; i < (int)(sizeof(ffgpu_frame_dets) / sizeof(int)); i += blockDim.x) reinterpret_cast<int *>(out_recs + t)[i] = 0;
            if (out_lists) for (long i = tid; i < stride; i += blockDim.x) track_zero(out_lists + t * stride + i);
        }
        return;
    }
    const int nst = 9 + 4 * C;                                                        // the state's 16-byte words
    int4 *const gst = reinterpret_cast<int4 *>(state + (size_t)vs * 16u * (size_t)nst);
    const int *const gsc = reinterpret_cast<const int *>(scenes + (size_t)vs * sizeof(ffgpu_scene));
    for (int i = tid; i < nst; i += blockDim.x) L.st[i] = gst[i];
    for (int i = tid; i < (int)(sizeof(ffgpu_scene) / 4); i += blockDim.x) L.sc[i] = gsc[i];
    __syncthreads();
    const ffgpu_scene &S = *reinterpret_cast<const ffgpu_scene *>(L.sc);
    ffgpu_zone_slot *const slot = reinterpret_cast<ffgpu_zone_slot *>(L.st + 9);
    unsigned *const hdr = reinterpret_cast<unsigned *>(L.st);                         // frames, live, reserved x 2, then the four totals
    const int nz = max(0, min(S.nzones, FFGPU_SCENE_ZONES)), nl = max(0, min(S.nlines, FFGPU_SCENE_LINES));
    const bool bottom = S.anchor != 0;
    if (tid < FFGPU_SCENE_ZONES) {                                                    // a zone that can contain something
        const ffgpu_zone &z = S.zone[tid];
        bool ok = z.nverts >= 3 && z.nverts <= FFGPU_ZONE_VERTS;
        for (int i = 0; ok && i < z.nverts; i++) ok = z.x[i] == z.x[i] && z.y[i] == z.y[i];
        L.zok[tid] = ok;
    }
    int frames = (int)hdr[0];                                                         // (uniform; written back at the end)
    const float min_score = a.spec.min_score;
    const int mode = a.spec.identity;
    const bool invert = (a.spec.flags & FFGPU_ZONES_GATE_INVERT) != 0;
    const int sidx = tid - FFGPU_ZONES_DETS;                                          // the slot of lanes 128..255
    const bool slane = sidx >= 0 && sidx < C;

    for (int e = e0; e < e1; e++) {
        const long t = a.en.rec[e];
        const ffgpu_frame_dets *rec = recs + t;
        const int n = max(0, min(lists ? rec->nfull : rec->count, stride)), ncand = rec->ncand, ovf = rec->overflow;
        const BBOX *list = lists ? lists + a.en.first[e] : rec->box;
        int *const row = events + t * rowlen;
        for (long i = tid; i < 2 * (long)stride; i += blockDim.x) row[FFGPU_ZONES_ROW + i] = 0;
        if (tid < FFGPU_ZONES_DETS) L.named[tid] = 0;

        // 1. the considered boxes, in list order
        const long nq = block_consider(n, FFGPU_ZONES_DETS, L.wsum, [&](int k) { return list[k].score >= min_score; },      // the qualifying boxes (uniform)
                                       [&](int ord, int k) { track_put(&L.det[ord], list[k].type, list[k]); L.didx[ord] = k; });
        const int nd = (int)min(nq, (long)FFGPU_ZONES_DETS), dropped = (int)min(nq - nd, 0x7fffffffL);

        // 2. geometry.  A lane owns its box: anchor, identity, the lines that admit it.  The inside mask is found by eight consecutive lanes per box,
        // a zone each (the same anchor arithmetic in each of them): the box's byte of the wave's ballot is its mask
        const bool box = tid < nd;
        const bool cls_known = mode != FFGPU_ZONES_TYPE;
        float px = 0.f, py = 0.f;
        int ident = 0;
        unsigned ladm = 0;
        if (box) {
            const BBOX b = L.det[tid];
            px = (b.x1 + b.x2) * 0.5f;
            py = bottom ? b.y2 : (b.y1 + b.y2) * 0.5f;
            ident = mode == FFGPU_ZONES_NONE ? 0 : mode == FFGPU_ZONES_TYPE ? b.type : ids[t * idlen + 8 + L.didx[tid]];
            for (int l = 0; l < nl; l++)
                if (zones_admits(S.line[l].classes, b.type, cls_known)) ladm |= 1u << l;
            L.ident[tid] = ident;
        }
        for (int p0 = 0; p0 < nd * FFGPU_SCENE_ZONES; p0 += 256) {                    // (uniform)
            const int j = (p0 + tid) >> 3, z = tid & 7;
            bool in = false;
            if (j < nd && z < nz && L.zok[z]) {
                const BBOX &b = L.det[j];
                const float qx = (b.x1 + b.x2) * 0.5f, qy = bottom ? b.y2 : (b.y1 + b.y2) * 0.5f;
                in = zones_admits(S.zone[z].classes, b.type, cls_known) && zones_inside(S.zone[z], qx, qy);
            }
            const unsigned long long m = __ballot(in);
            if (j < nd && z == 0) L.ins[j] = (int)((m >> (tid & 56)) & 0xffull);
        }
        __syncthreads();
        const int ins = box ? L.ins[tid] : 0;

        // 3. owners; 4. known owners: the lowest slot with the identity -- no other owner has it, so the lane updates the slot in place (no lane writes
        // an id before the next barrier)
        const bool anon = box && ident <= 0;
        const bool dup = box && !anon && ident_duplicate(L.ident, tid, ident);
        const bool owner = box && !anon && !dup;
        const int sl = owner ? slot_lowest(C, ident, [&](int s) { return slot[s].id; }) : -1;
        const bool known = sl >= 0;
        int entered = 0, left = 0, loit = 0, fwd = 0, back = 0;
        if (known) {
            ffgpu_zone_slot &q = slot[sl];
            const int was = q.inside & 0xff;
            entered = ins & ~was;
            left = was & ~ins;
            for (int z = 0; z < FFGPU_SCENE_ZONES; z++) if ((entered >> z) & 1) q.since[z] = frames;
            for (int l = 0; l < nl; l++)
                if ((ladm >> l) & 1u) {
                    const int c = zones_cross(S.line[l], q.px, q.py, px, py);
                    fwd |= (c == 1) << l;
                    back |= (c == 2) << l;
                }
            for (int z = 0; z < nz; z++) {
                const int dwell = S.zone[z].dwell_frames;
                if (((ins >> z) & 1) && dwell > 0 && (int)((unsigned)frames - (unsigned)q.since[z]) >= dwell) loit |= 1 << z;
            }
            q.px = px; q.py = py; q.inside = ins; q.last = frames;
            L.named[sl] = 1;
        }
        __syncthreads();

        // 5. frees (a lane owns its slot)
        bool freed = false;
        if (slane) {
            const ffgpu_zone_slot &q = slot[sidx];
            if (q.id != 0 && !L.named[sidx] && (int)((unsigned)frames - (unsigned)q.last) > a.spec.max_missed) {
                freed = true;
                left = q.inside & 0xff;                                               // (a slot lane has no box: its `left` is the freed object's)
                L.st[9 + 4 * sidx] = L.st[10 + 4 * sidx] = L.st[11 + 4 * sidx] = L.st[12 + 4 * sidx] = make_int4(0, 0, 0, 0);
            }
        }

        // 6. fresh owners: the r-th takes the r-th free slot (ranks within a wave pair: waves 0-1 the boxes, waves 2-3 the slots)
        const bool flag = tid < FFGPU_ZONES_DETS ? owner && !known : slane && slot[sidx].id == 0;
        bool fresh = false, refused = false;
        {
            const int fs = block_take_free(flag, tid < FFGPU_ZONES_DETS, sidx, L.wsum, L.freeslot);
            if (fs > -2) {
                if (fs >= 0) {
                    ffgpu_zone_slot &q = slot[fs];
                    q.id = ident; q.px = px; q.py = py; q.inside = ins; q.last = frames; q.reserved[0] = q.reserved[1] = q.reserved[2] = 0;
                    for (int z = 0; z < FFGPU_SCENE_ZONES; z++) q.since[z] = ((ins >> z) & 1) ? frames : 0;
                    fresh = true;
                    entered = ins;
                } else refused = true;
            }
            __syncthreads();
        }

        // 7. the boxes' words, the counts, the gated record
        unsigned w0 = 0, w1 = 0;
        if (box) {
            w0 = (unsigned)ins | (unsigned)entered << 8 | (unsigned)left << 16 | (unsigned)loit << 24;
            w1 = (unsigned)fwd | (unsigned)back << 8 | (unsigned)known << 16 | (unsigned)fresh << 17 | (unsigned)refused << 18 | (unsigned)dup << 19 | (unsigned)anon << 20;
            row[FFGPU_ZONES_ROW + 2 * L.didx[tid]] = (int)w0;                         // (zeroed above, barriers in between)
            row[FFGPU_ZONES_ROW + 2 * L.didx[tid] + 1] = (int)w1;
        }
        zones_count(L.cnt, 1, known); zones_count(L.cnt, 2, fresh); zones_count(L.cnt, 3, refused); zones_count(L.cnt, 4, dup); zones_count(L.cnt, 5, anon);
        zones_count(L.cnt, 7, freed);
        zones_count(L.cnt, 8, slane && slot[sidx].id != 0);
        for (int z = 0; z < FFGPU_SCENE_ZONES; z++) {
            zones_count(L.cnt, 16 + 4 * z, (ins >> z) & 1);
            zones_count(L.cnt, 17 + 4 * z, (entered >> z) & 1);
            zones_count(L.cnt, 18 + 4 * z, (left >> z) & 1);
            zones_count(L.cnt, 19 + 4 * z, (loit >> z) & 1);
        }
        for (int l = 0; l < FFGPU_SCENE_LINES; l++) { zones_count(L.cnt, 48 + 2 * l, (fwd >> l) & 1); zones_count(L.cnt, 49 + 2 * l, (back >> l) & 1); }
        const bool sel = box && ((((w0 & a.spec.gate_zone) | (w1 & a.spec.gate_line)) != 0) != invert);
        const int ord = block_rank(sel, L.wsum, 2), nt = L.wsum[0] + L.wsum[1];        // (nt <= nd <= n <= stride; the barrier inside publishes the counts)
        if (tid < FFGPU_ZONES_ROW) {
            const bool counted = tid >= 16 || (tid >= 1 && tid <= 8 && tid != 6);
            int v = counted ? L.cnt[0][tid] + L.cnt[1][tid] + L.cnt[2][tid] + L.cnt[3][tid] : tid == 0 ? nd : tid == 6 ? dropped : tid == 9 ? frames : 0;
            row[tid] = v;
            if (tid == 8) hdr[1] = (unsigned)v;
            if (tid >= 16 && tid < 48) {
                const int z = (tid - 16) >> 2, f = (tid - 16) & 3;
                if (f == 1) hdr[4 + z] += (unsigned)v;
                if (f == 2) hdr[12 + z] += (unsigned)v;
            }
            if (tid >= 48) hdr[((tid & 1) ? 28 : 20) + ((tid - 48) >> 1)] += (unsigned)v;
        }
        if (out_recs) {
            ffgpu_frame_dets *o = out_recs + t;
            if (sel) track_put(&o->box[ord], L.det[tid].type, L.det[tid]);
            if (tid >= nt && tid < FFGPU_MAX_DET) track_zero(&o->box[tid]);
            if (tid == 0) { o->count = min(nt, FFGPU_MAX_DET); o->ncand = ncand; o->overflow = (ovf & 1) | (nt > FFGPU_MAX_DET ? 4 : 0); o->nfull = nt; }
        }
        if (out_lists) {
            BBOX *ol = out_lists + t * stride;
            if (sel) track_put(&ol[ord], L.det[tid].type, L.det[tid]);
            for (long i = nt + tid; i < stride; i += blockDim.x) track_zero(&ol[i]);
        }
        frames = (int)((unsigned)frames + 1u);
        __syncthreads();                                                              // (the next frame rewrites the boxes and the counts)
    }
    if (tid == 0) hdr[0] = (unsigned)frames;
    __syncthreads();
    for (int i = tid; i < nst; i += blockDim.x) gst[i] = L.st[i];
}

// ---- host side
extern "C" size_t ffgpu_zones_state_bytes(int nstreams, int capacity) { return ffgpu_zones_state_bytes_host(nstreams, capacity); }
extern "C" int ffgpu_scene_check(const ffgpu_scene *host_scenes, int n) { return ffgpu_scene_check_host(host_scenes, n); }

// everything has been checked
int ffgpu_launch_zones(const DetSource &src, const int *streams, int ntargets, const ffgpu_zones_spec &spec, const void *d_scenes, void *d_state, const void *d_ids,
                       void *d_events, void *d_out_records, void *d_out_lists, hipStream_t s)
{
    for (int t0 = 0; t0 < ntargets; t0 += ZONES_ARG_ENTRIES) {
        const int nt = std::min(ZONES_ARG_ENTRIES, ntargets - t0);
        ZonesArgs a;
        memset(&a, 0, sizeof a);
        a.spec = spec;
        a.ngroups = ffgpu_stream_entries(src.first, streams, t0, nt, a.en);
        hipLaunchKernelGGL(k_zones, dim3((unsigned)a.ngroups), dim3(256), 0, s, a, src.recs, src.lists, src.stride, (const unsigned char *)d_scenes,
                           (unsigned char *)d_state, (const int *)d_ids, (int *)d_events, (ffgpu_frame_dets *)d_out_records, (BBOX *)d_out_lists);
        LAUNCH_OK("zones_boxes");
    }
    return 0;
}

extern "C" int ffgpu_zones_reset_dev(void *d_state, int nstreams, int capacity, int which_stream, void *stream)
{
    const char *const what = "zones_reset_dev";
    if (ffgpu_no_device(what)) return -1;
    const size_t all = ffgpu_zones_state_bytes(nstreams, capacity);
    if (!all) ffgpu_set_error("%s: %d streams of %d slots (nstreams 1..65536, capacity 1..%d)", what, nstreams, capacity, FFGPU_ZONES_DETS);   // (stands unless the state is NULL)
    return ffgpu_state_reset(what, d_state, all, nstreams, which_stream, stream);
}

extern "C" int ffgpu_zones_boxes_dev(const void *d_records, const void *d_lists, int list_stride, const int *list_first, const int *streams, int ntargets,
                                     const ffgpu_zones_spec *spec, const void *d_scenes, void *d_state, int nstreams, const void *d_ids, void *d_events,
                                     void *d_out_records, void *d_out_lists, void *stream)
{
    const char *const what = "zones_boxes_dev";
    if (ffgpu_no_device(what)) return -1;
    if (ffgpu_zones_args_check(what, streams, ntargets, spec, d_scenes, d_state, nstreams, d_ids, d_events, d_out_records, d_out_lists)) return -1;
    DetSource src;
    if (ffgpu_source_dev(what, d_records, d_lists, list_stride, list_first, ntargets, src)) return -1;
    return ffgpu_launch_zones(src, streams, ntargets, *spec, d_scenes, d_state, d_ids, d_events, d_out_records, d_out_lists, (hipStream_t)stream);
}
