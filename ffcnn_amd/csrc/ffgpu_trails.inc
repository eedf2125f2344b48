// ffgpu_trails.inc -- track trails: a history of anchors per identity and stream kept on the device, composed into segment items and motion rows
// (ffgpu_trails_boxes_dev, ffgpu_exec_trails, ffgpu_trails_reset_dev, ffgpu_trails_state_bytes, ffgpu_trails_spec_check).  The contract is in
// include/ffcnn_hip.h; the host side (spec and argument checks) is ffgpu_trails_host.hpp.
//
// One workgroup per video stream and launch, as k_zones, with its primitives (ffgpu_block.inc): the considered boxes compacted in list order, lanes
// 0..127 the boxes, lanes 128..255 the slots, a known owner the only lane that can name its slot, frees by the slot lanes, fresh owners by ranks.  The
// slots' 32-byte heads go through LDS (8 KB at capacity 128); the rings stay in global memory (48 KB per stream at capacity 128, which beside the
// boxes would sit against the 64 KB of static LDS): a slot has one owner lane per frame, which reads the newest point and writes one.  Whole rings
// are written only where a slot is freed or taken (zeroed, a fresh owner's first point with them), by all lanes together.  The items of a record are
// written by all lanes too, a (region, item) pair each: the two ring points a lane reads may have been written by another lane of the workgroup in
// this frame, in front of a barrier -- workgroup scope is all it takes; no device-scope fence, no atomic.  Integer arithmetic but the anchor.
struct TrailsArgs {
    StreamEntries<TRAILS_ARG_ENTRIES> en;             // the launch's records, grouped by video stream (ffgpu_streams_host.hpp)
    unsigned pal[256];
    int   capacity, max_missed, identity, flags, anchor, points, min_move, thickness, coast_dash, npal;
    float min_score;
    int   items_stride, first_item, nitems, ngroups;
};
static_assert(sizeof(TrailsArgs) + 8 * 8 <= 4096 - 256, "the tables travel as a kernel argument (4 KB at most, the hidden arguments included)");
static_assert(FFGPU_TRAILS_DETS == 128 && FFGPU_TRAILS_DETS == 2 * WAVE && FFGPU_MAX_DET == FFGPU_TRAILS_DETS, "k_trails: waves 0 and 1 own the boxes, waves 2 and 3 the slots");
static_assert(TRAILS_STATE_HEADER == 16 && sizeof(ffgpu_trail_slot) == 26 * 16 && offsetof(ffgpu_trail_slot, ring) == 32 && FFGPU_TRAIL_POINTS == 32 &&
              sizeof(ffgpu_trail_point) == 12 && FFGPU_TRAILS_ROW == 16, "k_trails: the layouts of include/ffcnn_hip.h");

struct TrailHead { int id, last, n, head, cx, cy, reserved[2]; };                     // the first 32 bytes of an ffgpu_trail_slot
struct TrailsLds {
    int4  hdr;                                        // the stream's header as it lies in memory
    TrailHead hd[FFGPU_TRAILS_DETS];                  // the slots' heads
    BBOX  det[FFGPU_TRAILS_DETS];                     // the considered boxes
    int   didx[FFGPU_TRAILS_DETS];                    // box j's index in its list
    int   ident[FFGPU_TRAILS_DETS];                   // box j's identity
    int   named[FFGPU_TRAILS_DETS];                   // slot s: an owner of this frame has its id
    int   refill[FFGPU_TRAILS_DETS];                  // slot s: its ring is rewritten in this frame (freed or taken)
    int4  first_pt[FFGPU_TRAILS_DETS];                //         and starts with these 16 bytes
    int   freeslot[FFGPU_TRAILS_DETS];
    int   region[FFGPU_TRAILS_DETS];                  // the k-th drawn slot
    int   cnt[4][FFGPU_TRAILS_ROW];                   // wave w's count for word i of the row's header
    int   wsum[4];
};
typedef unsigned trails_u4 __attribute__((ext_vector_type(4), aligned(4)));           // 16 bytes of an item: the items are 4-byte aligned

// what is read of a slot's n and head: n clamped to 0..points, head modulo 32
__device__ __forceinline__ int trails_n(int n, int P) { return max(0, min(n, P)); }
__device__ __forceinline__ int trails_head(int head) { return head & (FFGPU_TRAIL_POINTS - 1); }
__device__ __forceinline__ long long trails_abs(long long v) { return v < 0 ? -v : v; }

// grid = groups of the launch, 256 lanes.  Counts are clamped to [0, stride] as the draw kernel clamps them.  Total over any state bytes.
__global__ void __launch_bounds__(256) k_trails(TrailsArgs a, const ffgpu_frame_dets *recs, const BBOX *lists, int stride, unsigned char *state, const int *ids,
                                                int *rows, unsigned *items)
{
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) unsigned char s_trails[sizeof(TrailsLds)];
    TrailsLds &L = *reinterpret_cast<TrailsLds *>(s_trails);
    const int tid = threadIdx.x, g = blockIdx.x;
    const int e0 = a.en.goff[g], e1 = a.en.goff[g + 1], vs = a.en.gstream[g], C = a.capacity, P = a.points;
    const long rowlen = FFGPU_TRAILS_ROW + 4 * (long)stride, idlen = 8 + (long)stride;
    const int nitems = items ? a.nitems : 0;
    if (vs < 0) {                                                                     // the ignored entries: every output byte zero (uniform)
        for (int e = e0; e < e1; e++) {
            const long t = a.en.rec[e];
            for (long i = tid; i < rowlen; i += blockDim.x) rows[t * rowlen + i] = 0;
            unsigned *dst = items + ((size_t)t * (size_t)a.items_stride + (size_t)a.first_item) * 8u;
            for (int i = tid; i < nitems * 8; i += blockDim.x) dst[i] = 0;
        }
        return;
    }
    unsigned char *const gbase = state + (size_t)vs * (TRAILS_STATE_HEADER + sizeof(ffgpu_trail_slot) * (size_t)C);
    ffgpu_trail_slot *const gslot = reinterpret_cast<ffgpu_trail_slot *>(gbase + TRAILS_STATE_HEADER);
    if (tid == 0) L.hdr = *reinterpret_cast<const int4 *>(gbase);
    for (int i = tid; i < 2 * C; i += blockDim.x) reinterpret_cast<int4 *>(L.hd)[i] = reinterpret_cast<const int4 *>(gslot + (i >> 1))[i & 1];
    __syncthreads();
    int frames = L.hdr.x;                                                             // (uniform; written back at the end)
    const float min_score = a.min_score;
    const bool bottom = a.anchor != 0, by_type = a.identity == FFGPU_ZONES_TYPE;
    const bool coast = (a.flags & FFGPU_TRAILS_COAST) != 0, taper = (a.flags & FFGPU_TRAILS_TAPER) != 0;
    const int sidx = tid - FFGPU_TRAILS_DETS;                                         // the slot of lanes 128..255
    const bool slane = sidx >= 0 && sidx < C;

    for (int e = e0; e < e1; e++) {
        const long t = a.en.rec[e];
        const ffgpu_frame_dets *rec = recs + t;
        const int n = max(0, min(lists ? rec->nfull : rec->count, stride));
        const BBOX *list = lists ? lists + a.en.first[e] : rec->box;
        int *const row = rows + t * rowlen;
        for (long i = tid; i < 4 * (long)stride; i += blockDim.x) row[FFGPU_TRAILS_ROW + i] = 0;
        if (tid < FFGPU_TRAILS_DETS) { L.named[tid] = 0; L.refill[tid] = 0; }

        // 1. the considered boxes, in list order
        const long nq = block_consider(n, FFGPU_TRAILS_DETS, L.wsum, [&](int k) { return list[k].score >= min_score; },
                                       [&](int ord, int k) { track_put(&L.det[ord], list[k].type, list[k]); L.didx[ord] = k; });
        const int nd = (int)min(nq, (long)FFGPU_TRAILS_DETS), dropped = (int)min(nq - nd, 0x7fffffffL);

        // 2. a lane owns its box: the anchor, converted, and the identity
        const bool box = tid < nd;
        int ax = 0, ay = 0, ident = 0;
        if (box) {
            const BBOX b = L.det[tid];
            ax = draw_f2i((b.x1 + b.x2) * 0.5f);
            ay = draw_f2i(bottom ? b.y2 : (b.y1 + b.y2) * 0.5f);
            ident = by_type ? b.type : ids[t * idlen + 8 + L.didx[tid]];
            L.ident[tid] = ident;
        }
        __syncthreads();

        // 3. owners; 4. known owners: the lowest slot with the identity -- no other owner has it, so the lane updates the head in place and is the one
        // lane that touches the slot's ring in this frame (no lane writes an id before the next barrier)
        const bool anon = box && ident <= 0;
        const bool dup = box && !anon && ident_duplicate(L.ident, tid, ident);
        const bool owner = box && !anon && !dup;
        const int sl = owner ? slot_lowest(C, ident, [&](int s) { return L.hd[s].id; }) : -1;
        const bool known = sl >= 0;
        bool appended = false;
        int mn = 0, mdx = 0, mdy = 0, mdf = 0;                                        // the motion row
        if (known) {
            TrailHead &q = L.hd[sl];
            ffgpu_trail_point *const ring = gslot[sl].ring;
            int qn = trails_n(q.n, P), qh = trails_head(q.head);
            appended = qn == 0;
            if (!appended) {
                const ffgpu_trail_point &N = ring[(qh + qn - 1) & 31];
                const int nx = N.x, ny = N.y;
                appended = max(trails_abs((long long)ax - nx), trails_abs((long long)ay - ny)) >= (long long)a.min_move;
            }
            if (appended) {
                if (qn == P) qh = (qh + 1) & 31; else qn++;
                ffgpu_trail_point &w = ring[(qh + qn - 1) & 31];
                w.x = ax; w.y = ay; w.frame = frames;
            }
            int ox = ax, oy = ay, of = frames;                                        // the oldest live point: the one just written when it is the only one
            if (!(appended && qn == 1)) { ox = ring[qh].x; oy = ring[qh].y; of = ring[qh].frame; }
            q.n = qn; q.head = qh; q.cx = ax; q.cy = ay; q.last = frames;
            mn = qn; mdx = seg_sat((long long)ax - ox); mdy = seg_sat((long long)ay - oy); mdf = (int)((unsigned)frames - (unsigned)of);
            L.named[sl] = 1;
        }
        __syncthreads();

        // 5. frees (a lane owns its slot): the head here, the ring below
        bool freed = false;
        if (slane) {
            TrailHead &q = L.hd[sidx];
            if (q.id != 0 && !L.named[sidx] && (int)((unsigned)frames - (unsigned)q.last) > a.max_missed) {
                freed = true;
                reinterpret_cast<int4 *>(&q)[0] = reinterpret_cast<int4 *>(&q)[1] = make_int4(0, 0, 0, 0);
                L.refill[sidx] = 1; L.first_pt[sidx] = make_int4(0, 0, 0, 0);
            }
        }

        // 6. fresh owners: the r-th takes the r-th free slot
        const bool flag = tid < FFGPU_TRAILS_DETS ? owner && !known : slane && L.hd[sidx].id == 0;
        const int fs = block_take_free(flag, tid < FFGPU_TRAILS_DETS, sidx, L.wsum, L.freeslot);
        const bool fresh = fs >= 0, refused = fs == -1;
        if (fresh) {
            TrailHead &q = L.hd[fs];
            q.id = ident; q.last = frames; q.n = 1; q.head = 0; q.cx = ax; q.cy = ay; q.reserved[0] = q.reserved[1] = 0;
            L.refill[fs] = 1; L.first_pt[fs] = make_int4(ax, ay, frames, 0);
            mn = 1;
        }
        __syncthreads();
        for (int i = tid; i < C * 24; i += blockDim.x) {                              // the rings of the freed and the taken slots: 24 x 16 bytes each
            const int s = i / 24, w = i - s * 24;
            if (L.refill[s]) reinterpret_cast<int4 *>(gslot[s].ring)[w] = w ? make_int4(0, 0, 0, 0) : L.first_pt[s];
        }

        // 7. the motion rows, the drawn slots' regions, the counts
        if (known || fresh) {
            int *w = row + FFGPU_TRAILS_ROW + 4 * (long)L.didx[tid];                  // (zeroed above, barriers in between)
            w[0] = mn; w[1] = mdx; w[2] = mdy; w[3] = mdf;
        }
        bool drawn = false;
        if (slane) {
            const TrailHead &q = L.hd[sidx];
            drawn = q.id != 0 && trails_n(q.n, P) >= 1 && (q.last == frames || coast);
        }
        const int k = block_rank(drawn, L.wsum, 2);                                   // (the box lanes flag nothing; the barrier inside publishes the rings)
        const bool placed = drawn && ((long)k + 1) * P <= nitems;
        if (placed) L.region[k] = sidx;
        wave_count(L.cnt, 1, known); wave_count(L.cnt, 2, fresh); wave_count(L.cnt, 3, refused); wave_count(L.cnt, 4, dup); wave_count(L.cnt, 5, anon);
        wave_count(L.cnt, 7, freed);
        wave_count(L.cnt, 8, slane && L.hd[sidx].id != 0);
        wave_count(L.cnt, 10, appended); wave_count(L.cnt, 11, placed); wave_count(L.cnt, 12, drawn && !placed);
        __syncthreads();
        if (tid < FFGPU_TRAILS_ROW) {
            const bool counted = (tid >= 1 && tid <= 5) || tid == 7 || tid == 8 || (tid >= 10 && tid <= 12);
            const int v = counted ? L.cnt[0][tid] + L.cnt[1][tid] + L.cnt[2][tid] + L.cnt[3][tid] : tid == 0 ? nd : tid == 6 ? dropped : tid == 9 ? frames : 0;
            row[tid] = v;
            if (tid == 8) L.hdr.y = v;
        }
        const int nreg = L.cnt[2][11] + L.cnt[3][11];
        unsigned *const dst = items + ((size_t)t * (size_t)a.items_stride + (size_t)a.first_item) * 8u;
        for (int i = tid; i < nitems; i += blockDim.x) {                              // item i: item j of region r
            const int r = i / P, j = i - r * P;
            trails_u4 lo = { 0u, 0u, 0u, 0u }, hi = { 0u, 0u, 0u, 0u };
            if (r < nreg) {
                const int s = L.region[r];
                const TrailHead &q = L.hd[s];
                const ffgpu_trail_point *ring = gslot[s].ring;
                const int qn = trails_n(q.n, P), qh = trails_head(q.head);
                const bool tip = j == P - 1;
                if (tip || j + 1 < qn) {                                              // (the words of seg_put; ints need no saturation)
                    const ffgpu_trail_point &p0 = ring[(qh + (tip ? qn - 1 : j)) & 31], &p1 = ring[(qh + j + 1) & 31];
                    const int x0 = p0.x, y0 = p0.y, x1 = tip ? q.cx : p1.x, y1 = tip ? q.cy : p1.y;
                    const int T = tip || !taper ? a.thickness : 1 + ((a.thickness - 1) * (j + 1)) / qn;
                    const int d = q.last != frames ? a.coast_dash : 0;
                    lo = (trails_u4){ (unsigned)x0, (unsigned)y0, (unsigned)x1, (unsigned)y1 };
                    hi = (trails_u4){ a.pal[draw_colour_index(q.id, a.npal)], (unsigned)T | (unsigned)d << 8, 0u, 0u };
                }
            }
            *reinterpret_cast<trails_u4 *>(dst + (size_t)i * 8u) = lo;
            *reinterpret_cast<trails_u4 *>(dst + (size_t)i * 8u + 4u) = hi;
        }
        frames = (int)((unsigned)frames + 1u);
        __syncthreads();                                                              // (the next frame rewrites the boxes, the heads and the counts)
    }
    if (tid == 0) { L.hdr.x = frames; *reinterpret_cast<int4 *>(gbase) = L.hdr; }
    for (int i = tid; i < 2 * C; i += blockDim.x) reinterpret_cast<int4 *>(gslot + (i >> 1))[i & 1] = reinterpret_cast<const int4 *>(L.hd)[i];
}

// ---- host side
extern "C" size_t ffgpu_trails_state_bytes(int nstreams, int capacity) { return ffgpu_trails_state_bytes_host(nstreams, capacity); }
extern "C" int ffgpu_trails_spec_check(const ffgpu_trails_spec *spec)
{
    TrailsPlan pl;
    return ffgpu_trails_spec_plan("trails_spec_check", spec, pl);
}

// everything has been checked
int ffgpu_launch_trails(const DetSource &src, const int *streams, int ntargets, const TrailsPlan &pl, void *d_state, const void *d_ids, void *d_rows, void *d_items,
                        int items_stride, int first_item, int nitems, hipStream_t s)
{
    for (int t0 = 0; t0 < ntargets; t0 += TRAILS_ARG_ENTRIES) {
        const int nt = std::min(TRAILS_ARG_ENTRIES, ntargets - t0);
        TrailsArgs a;
        memset(&a, 0, sizeof a);
        memcpy(a.pal, pl.pal, sizeof a.pal);
        a.capacity = pl.capacity; a.max_missed = pl.max_missed; a.identity = pl.identity; a.flags = pl.flags; a.anchor = pl.anchor; a.points = pl.points;
        a.min_move = pl.min_move; a.thickness = pl.thickness; a.coast_dash = pl.coast_dash; a.npal = pl.npal; a.min_score = pl.min_score;
        a.items_stride = items_stride; a.first_item = first_item; a.nitems = nitems;
        a.ngroups = ffgpu_stream_entries(src.first, streams, t0, nt, a.en);
        hipLaunchKernelGGL(k_trails, dim3((unsigned)a.ngroups), dim3(256), 0, s, a, src.recs, src.lists, src.stride, (unsigned char *)d_state, (const int *)d_ids,
                           (int *)d_rows, (unsigned *)d_items);
        LAUNCH_OK("trails_boxes");
    }
    return 0;
}

extern "C" int ffgpu_trails_reset_dev(void *d_state, int nstreams, int capacity, int which_stream, void *stream)
{
    const char *const what = "trails_reset_dev";
    if (ffgpu_no_device(what)) return -1;
    const size_t all = ffgpu_trails_state_bytes(nstreams, capacity);
    if (!all) ffgpu_set_error("%s: %d streams of %d slots (nstreams 1..65536, capacity 1..%d)", what, nstreams, capacity, FFGPU_TRAILS_DETS);   // (stands unless the state is NULL)
    return ffgpu_state_reset(what, d_state, all, nstreams, which_stream, stream);
}

extern "C" int ffgpu_trails_boxes_dev(const void *d_records, const void *d_lists, int list_stride, const int *list_first, const int *streams, int ntargets,
                                      const ffgpu_trails_spec *spec, void *d_state, int nstreams, const void *d_ids, void *d_rows, void *d_items,
                                      int items_stride, int first_item, int nitems, void *stream)
{
    const char *const what = "trails_boxes_dev";
    if (ffgpu_no_device(what)) return -1;
    TrailsPlan pl;
    if (ffgpu_trails_args_check(what, streams, ntargets, spec, d_state, nstreams, d_ids, d_rows, d_items, items_stride, first_item, nitems, pl)) return -1;
    DetSource src;
    if (ffgpu_source_dev(what, d_records, d_lists, list_stride, list_first, ntargets, src)) return -1;
    return ffgpu_launch_trails(src, streams, ntargets, pl, d_state, d_ids, d_rows, d_items, items_stride, first_item, nitems, (hipStream_t)stream);
}
