// ffgpu_track.inc -- the detections tracked across a stream's frames on the device (ffgpu_track_boxes_dev, ffgpu_exec_track, ffgpu_track_reset_dev,
// ffgpu_track_state_bytes): a greedy, class-aware IoU tracker with "last box, no motion model", specified so that its result is a pure function of
// its inputs.  The contract is in include/ffcnn_hip.h; the host side (spec and argument checks) is ffgpu_track_host.hpp.
//
// One workgroup per video stream and launch: it loads the stream's state into LDS once, walks the stream's records of the launch serially and writes
// the state back once.  Per frame: the considered detections are compacted into LDS by ballots (list order kept), the IoU of every (slot, detection)
// pair goes into an LDS matrix (box_overlap and box_iou of ffgpu_block.inc; -1: not eligible), and the greedy matching in the contract's total order is found without sorting: a pair that
// is the first of its row (iou desc, detection asc) AND the first of its column (iou desc, slot asc) among the unmatched precedes every other
// remaining pair that shares its track or its detection, so the serial walk takes it; all such pairs are taken per round, and the first remaining
// pair of the whole matrix is always one of them.  Rounds: a handful on real frames, at most min(tracks, detections).  Frees, births (ranks from
// ballots, block_rank: the r-th birth takes the r-th free slot) and the counters use no atomic.
//
// The entries of a launch (TRACK_ARG_ENTRIES records, sorted by video stream on the host, record order kept inside a stream) and the spec travel as
// ONE by-value kernel argument; more records: more launches, in order on the one stream, the state carrying a stream from one to the next.
#define TRACK_ARG_ENTRIES 128
#define TRACK_PITCH       (FFGPU_TRACK_DETS + 1)      // floats per matrix row: row a starts in bank a
struct TrackArgs {
    StreamEntries<TRACK_ARG_ENTRIES> en;              // the launch's records, grouped by video stream (ffgpu_streams_host.hpp)
    ffgpu_track_spec spec;
    int   ngroups, pad_[3];
};
static_assert(sizeof(TrackArgs) + 7 * 8 <= 4096 - 256, "the tables travel as a kernel argument (4 KB at most, the hidden arguments included)");
static_assert(FFGPU_TRACK_DETS == 128 && FFGPU_TRACK_DETS == 2 * WAVE, "k_track: waves 0 and 1 own the detections, waves 2 and 3 the slots");

// the workgroup's LDS, all of it dynamic (above 64 KB: allowed per kernel and per device like k_spp's)
struct TrackLds {
    float iou[FFGPU_TRACK_DETS * TRACK_PITCH];        // [slot][detection]; -1: not eligible
    int4  st[1 + 3 * FFGPU_TRACK_DETS];               // the stream's state as it lies in memory: header, then the slots
    BBOX  det[FFGPU_TRACK_DETS];                      // the considered detections
    int   didx[FFGPU_TRACK_DETS];                     // detection j's index in its list
    int   dmatch[FFGPU_TRACK_DETS];                   // detection j's slot (matched or born), -1: none
    int   tmatch[FFGPU_TRACK_DETS];                   // slot a's detection, -1: none
    int   rowj[FFGPU_TRACK_DETS], cola[FFGPU_TRACK_DETS], freeslot[FFGPU_TRACK_DETS];
    int   wsum[4], any, pad_[3];
};

// a box written field by field (no BBOX temporaries: they would live in scratch)
__device__ __forceinline__ void track_put(BBOX *p, int type, const BBOX &b) { p->type = type; p->score = b.score; p->x1 = b.x1; p->y1 = b.y1; p->x2 = b.x2; p->y2 = b.y2; }
__device__ __forceinline__ void track_zero(BBOX *p) { p->type = 0; p->score = 0.f; p->x1 = 0.f; p->y1 = 0.f; p->x2 = 0.f; p->y2 = 0.f; }

// grid = groups of the launch, 256 lanes.  Counts are clamped to [0, stride] as the draw kernel clamps them.
__global__ void __launch_bounds__(256) k_track(TrackArgs a, const ffgpu_frame_dets *recs, const BBOX *lists, int stride, unsigned char *state,
                                               int *ids, ffgpu_frame_dets *out_recs, BBOX *out_lists)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char s_track[];
    TrackLds &L = *reinterpret_cast<TrackLds *>(s_track);
    const int tid = threadIdx.x, g = blockIdx.x;
    const int e0 = a.en.goff[g], e1 = a.en.goff[g + 1], vs = a.en.gstream[g], C = a.spec.capacity;
    const long rowlen = 8 + (long)stride;
    if (vs < 0) {                                                                     // the ignored entries: every output byte zero (uniform)
        for (int e = e0; e < e1; e++) {
            const long t = a.en.rec[e];
            for (long i = tid; i < rowlen; i += blockDim.x) ids[t * rowlen + i] = 0;
            if (out_recs) for (int i = tid; i < (int)(sizeof(ffgpu_frame_dets) / sizeof(int)); i += blockDim.x) reinterpret_cast<int *>(out_recs + t)[i] = 0;
            if (out_lists) for (long i = tid; i < stride; i += blockDim.x) track_zero(out_lists + t * stride + i);
        }
        return;
    }
    const int nst = 1 + 3 * C;                                                        // the state's 16-byte words
    int4 *const gst = reinterpret_cast<int4 *>(state + (size_t)vs * 16u * (size_t)nst);
    for (int i = tid; i < nst; i += blockDim.x) L.st[i] = gst[i];
    __syncthreads();
    ffgpu_track *const trk = reinterpret_cast<ffgpu_track *>(L.st + 1);
    int issued = L.st[0].x, frames = L.st[0].y, live = L.st[0].z;                     // (uniform; written back at the end)
    const float min_score = a.spec.min_score, birth_score = a.spec.birth_score, thr = a.spec.iou_thresh;

    for (int e = e0; e < e1; e++) {
        const long t = a.en.rec[e];
        const ffgpu_frame_dets *rec = recs + t;
        const int n = max(0, min(lists ? rec->nfull : rec->count, stride)), ncand = rec->ncand, ovf = rec->overflow;
        const BBOX *list = lists ? lists + a.en.first[e] : rec->box;
        int *const row = ids + t * rowlen;
        for (long i = tid; i < stride; i += blockDim.x) row[8 + i] = 0;
        if (tid < FFGPU_TRACK_DETS) { L.dmatch[tid] = -1; L.tmatch[tid] = -1; }

        // 1. the considered detections, in list order
        long nq = 0;                                                                  // qualifying boxes so far (uniform)
        for (int k0 = 0; k0 < n; k0 += 256) {
            const int k = k0 + tid;
            const bool q = k < n && list[k].score >= min_score;
            int tot;
            const long ord = nq + block_rank(q, L.wsum, 4, tot);
            if (q && ord < FFGPU_TRACK_DETS) { track_put(&L.det[ord], list[k].type, list[k]); L.didx[ord] = k; }
            nq += tot;
            __syncthreads();
        }
        const int nd = (int)min(nq, (long)FFGPU_TRACK_DETS), dropped = (int)min(nq - nd, 0x7fffffffL);

        // 2. the matrix
        for (int p = tid; p < C * nd; p += blockDim.x) {
            const int s = p / nd, j = p - s * nd;
            const ffgpu_track ba = trk[s];
            float v = -1.f;
            if (ba.id != 0) {
                const BBOX bj = L.det[j];
                const float area_a = box_area(ba.x1, ba.y1, ba.x2, ba.y2);
                float inter, area_j;
                box_overlap(ba, bj, inter, area_j);
                const float iou = box_iou(inter, area_a, area_j);
                if (iou >= thr && (!a.spec.class_aware || ba.type == bj.type)) v = iou;   // (thr >= 0: an eligible value is never below -0.0)
            }
            L.iou[s * TRACK_PITCH + j] = v;
        }
        __syncthreads();

        // 3. the matching: lanes 0..127 own the slots (rows), lanes 128..255 the detections (columns)
        const bool occupied = tid < C && trk[tid < C ? tid : 0].id != 0;              // slot tid at the frame's start (lanes >= 128: false)
        for (;;) {
            if (tid == 0) L.any = 0;
            __syncthreads();
            if (tid < FFGPU_TRACK_DETS) {
                int bj = -1;
                float best = -1.f;
                if (occupied && L.tmatch[tid] < 0)
                    for (int j = 0; j < nd; j++) {
                        if (L.dmatch[j] >= 0) continue;
                        const float v = L.iou[tid * TRACK_PITCH + j];
                        if (v >= 0.f && (bj < 0 || v > best)) { best = v; bj = j; }
                    }
                L.rowj[tid] = bj;
                if (bj >= 0) L.any = 1;
            } else {
                const int j = tid - FFGPU_TRACK_DETS;
                int bs = -1;
                float best = -1.f;
                if (j < nd && L.dmatch[j] < 0)
                    for (int s = 0; s < C; s++) {
                        if (L.tmatch[s] >= 0) continue;
                        const float v = L.iou[s * TRACK_PITCH + j];
                        if (v >= 0.f && (bs < 0 || v > best)) { best = v; bs = s; }
                    }
                L.cola[j] = bs;
            }
            __syncthreads();
            if (!L.any) break;                                                        // (uniform: read behind a barrier, rewritten behind the next)
            if (tid < FFGPU_TRACK_DETS) {
                const int bj = L.rowj[tid];
                if (bj >= 0 && L.cola[bj] == tid) { L.tmatch[tid] = bj; L.dmatch[bj] = tid; }
            }
            __syncthreads();
        }

        // 4. 5. matched and unmatched tracks (a lane owns its slot)
        bool matched = false, gone = false;
        if (occupied) {
            ffgpu_track &tr = trk[tid];
            const int j = L.tmatch[tid];
            if (j >= 0) {
                const BBOX b = L.det[j];
                tr.type = b.type; tr.score = b.score; tr.x1 = b.x1; tr.y1 = b.y1; tr.x2 = b.x2; tr.y2 = b.y2;
                tr.hits += 1; tr.missed = 0; tr.det = L.didx[j];
                matched = true;
            } else {
                tr.missed += 1; tr.det = -1;
                gone = tr.missed > a.spec.max_missed;
                if (gone) L.st[1 + 3 * tid] = L.st[2 + 3 * tid] = L.st[3 + 3 * tid] = make_int4(0, 0, 0, 0);
            }
        }
        const int nmatched = __syncthreads_count(matched), nfreed = __syncthreads_count(gone);

        // 6. births: the r-th unmatched detection that may start a track takes the r-th free slot (ranks within a wave pair: waves 0-1 the
        // detections, waves 2-3 the slots)
        bool flag;
        if (tid < FFGPU_TRACK_DETS) flag = tid < nd && L.dmatch[tid] < 0 && L.det[tid].score >= birth_score;
        else                        flag = tid - FFGPU_TRACK_DETS < C && trk[tid - FFGPU_TRACK_DETS].id == 0;
        {
            const int r = block_rank(flag, L.wsum, 2);
            const int nwant = L.wsum[0] + L.wsum[1], nfree = L.wsum[2] + L.wsum[3];
            if (flag && tid >= FFGPU_TRACK_DETS) L.freeslot[r] = tid - FFGPU_TRACK_DETS;
            __syncthreads();
            if (flag && tid < FFGPU_TRACK_DETS && r < nfree) {
                const int s = L.freeslot[r];
                const BBOX b = L.det[tid];
                ffgpu_track &tr = trk[s];
                tr.id = (int)((unsigned)issued + (unsigned)r + 1u); tr.type = b.type; tr.score = b.score; tr.x1 = b.x1; tr.y1 = b.y1; tr.x2 = b.x2; tr.y2 = b.y2;
                tr.hits = 1; tr.missed = 0; tr.born = frames; tr.det = L.didx[tid]; tr.reserved = 0;
                L.dmatch[tid] = s;
            }
            const int nborn = min(nwant, nfree), nrefused = nwant - nborn;
            issued = (int)((unsigned)issued + (unsigned)nborn);
            __syncthreads();

            // 7. and the outputs
            live = __syncthreads_count(tid < C && trk[tid < C ? tid : 0].id != 0);
            if (tid == 0) {
                row[0] = nd; row[1] = nmatched; row[2] = nborn; row[3] = nrefused; row[4] = dropped; row[5] = nfreed; row[6] = live; row[7] = frames;
            }
        }
        int id = 0;
        bool conf = false;
        if (tid < nd && L.dmatch[tid] >= 0) {
            const ffgpu_track tr = trk[L.dmatch[tid]];
            conf = tr.hits >= a.spec.min_hits;
            id = tr.id;
            row[8 + L.didx[tid]] = conf ? id : (int)(0u - (unsigned)id);               // (zeroed above, barriers in between)
        }
        {
            const int ord = block_rank(conf, L.wsum, 2), nt = L.wsum[0] + L.wsum[1];   // (nt <= nd <= n <= stride)
            if (out_recs) {
                ffgpu_frame_dets *o = out_recs + t;
                if (conf) track_put(&o->box[ord], id, L.det[tid]);
                if (tid >= nt && tid < FFGPU_MAX_DET) track_zero(&o->box[tid]);
                if (tid == 0) { o->count = min(nt, FFGPU_MAX_DET); o->ncand = ncand; o->overflow = (ovf & 1) | (nt > FFGPU_MAX_DET ? 4 : 0); o->nfull = nt; }
            }
            if (out_lists) {
                BBOX *ol = out_lists + t * stride;
                if (conf) track_put(&ol[ord], id, L.det[tid]);
                for (long i = nt + tid; i < stride; i += blockDim.x) track_zero(&ol[i]);
            }
        }
        frames = (int)((unsigned)frames + 1u);
        __syncthreads();                                                              // (the next frame rewrites the detections)
    }
    if (tid == 0) L.st[0] = make_int4(issued, frames, live, 0);
    __syncthreads();
    for (int i = tid; i < nst; i += blockDim.x) gst[i] = L.st[i];
}
static_assert(FFGPU_MAX_DET == FFGPU_TRACK_DETS, "k_track: a tracked record holds every considered box");

// ---- host side
extern "C" size_t ffgpu_track_state_bytes(int nstreams, int capacity) { return ffgpu_track_state_bytes_host(nstreams, capacity); }

// everything has been checked
int ffgpu_launch_track(const DetSource &src, const int *streams, int ntargets, const ffgpu_track_spec &spec, void *d_state, void *d_ids, void *d_out_records, void *d_out_lists, hipStream_t s)
{
    const size_t lds = sizeof(TrackLds);
    if (lds_allow((const void *)k_track, lds, "track_boxes")) return -1;
    for (int t0 = 0; t0 < ntargets; t0 += TRACK_ARG_ENTRIES) {
        const int nt = std::min(TRACK_ARG_ENTRIES, ntargets - t0);
        TrackArgs a;
        memset(&a, 0, sizeof a);
        a.spec = spec;
        a.ngroups = ffgpu_stream_entries(src.first, streams, t0, nt, a.en);
        hipLaunchKernelGGL(k_track, dim3((unsigned)a.ngroups), dim3(256), lds, s, a, src.recs, src.lists, src.stride, (unsigned char *)d_state, (int *)d_ids,
                           (ffgpu_frame_dets *)d_out_records, (BBOX *)d_out_lists);
        LAUNCH_OK("track_boxes");
    }
    return 0;
}

extern "C" int ffgpu_track_reset_dev(void *d_state, int nstreams, int capacity, int which_stream, void *stream)
{
    const char *const what = "track_reset_dev";
    if (ffgpu_no_device(what)) return -1;
    const size_t all = ffgpu_track_state_bytes(nstreams, capacity);
    if (!all) ffgpu_set_error("%s: %d streams of %d slots (nstreams 1..65536, capacity 1..%d)", what, nstreams, capacity, FFGPU_TRACK_DETS);   // (stands unless the state is NULL)
    return ffgpu_state_reset(what, d_state, all, nstreams, which_stream, stream);
}

extern "C" int ffgpu_track_boxes_dev(const void *d_records, const void *d_lists, int list_stride, const int *list_first, const int *streams, int ntargets,
                                     const ffgpu_track_spec *spec, void *d_state, int nstreams, void *d_ids, void *d_out_records, void *d_out_lists, void *stream)
{
    const char *const what = "track_boxes_dev";
    if (ffgpu_no_device(what)) return -1;
    if (ffgpu_track_args_check(what, streams, ntargets, spec, d_state, nstreams, d_ids, d_out_records, d_out_lists)) return -1;
    DetSource src;
    if (ffgpu_source_dev(what, d_records, d_lists, list_stride, list_first, ntargets, src)) return -1;
    return ffgpu_launch_track(src, streams, ntargets, *spec, d_state, d_ids, d_out_records, d_out_lists, (hipStream_t)stream);
}
