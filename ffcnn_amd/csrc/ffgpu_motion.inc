// ffgpu_motion.inc -- motion maps: a per-stream background model of the frames' luma kept on the device, the changed pixels counted per cell, and the
// boxes of any record gated by the cells that move (ffgpu_motion_update_bgr_dev / _nv12_dev, ffgpu_motion_gate_dev, ffgpu_exec_motion_gate,
// ffgpu_motion_reset_dev, ffgpu_motion_state_bytes, ffgpu_motion_spec_check).  The contract is in include/ffcnn_hip.h; the host side (layout, spec,
// argument checks and the rounds of an update call) is ffgpu_motion_host.hpp.
//
// k_motion_update<NV12>: the first kernel of the post-passes that reads whole frames: a streaming kernel, 3 + 2 + 2 bytes a pixel in BGR and
// 1 + 2 + 2 in NV12.  A workgroup owns a tile of 64 x 64 pixels of its target, which is whole cells at every legal cell size, and is the only one to
// touch the tile's shorts of the plane and the tile's cells.  A lane owns RUNS of 8 consecutive pixels, one in each half of the tile: the run's 16
// bytes of the plane are one aligned load and one aligned store (the plane's pitch is a multiple of 8 shorts), and its 24 (8) frame bytes, which
// start at any alignment, are the aligned dwords that cover them -- loaded whole where they lie inside the row's bytes, byte by byte at the row's
// two ends -- shifted into place by v_alignbyte; a whole run of a target whose rows are 8-byte aligned takes 8-byte loads instead.  Both runs' loads
// are issued before the first is used.  The changed pixels are counted per 4 pixels of a run into LDS, folded to the 16 x 16 cells of 4 pixels by
// one lane each and then level by level, 2 x 2 at a time, up to the spec's cell size; one lane stores a cell.  No atomics, no scratch.  The launch
// only READS the header's `frames`.
//
// k_motion_row: one workgroup per target, behind the update launch of its round: the stream's cells folded (block_fold) into the row, `frames`
// written.  k_motion_gate: one workgroup per record with k_heat_accumulate's list walk (block_consider); a wave takes a considered box and counts
// the active cells under it, lanes along the cells' rows; the gated record is written as k_zones writes its own.
struct MotionArgs {
    DrawTarget t[MOTION_ARG_TARGETS];                 // (first: the target's stream; p0 == NULL: skipped)
    int   tgt[MOTION_ARG_TARGETS];                    // the target's index in the call: its row
    int   w, h, k, gw, gh, pitch, thr, learn, learn_changed, min_pixels, warmup, pad_;
    unsigned long long cells_off, stream_bytes;
};
struct MotionGateArgs {
    long long first[MOTION_ARG_TARGETS];              // record e of the launch: its list's first box in `lists`
    int   stream[MOTION_ARG_TARGETS];                 //                         its video stream, or -1
    unsigned char classes[256];
    int   nclasses, w, h, k, gw, min_pixels, cover, warmup, invert;
    float min_score;
    unsigned long long cells_off, stream_bytes;
};
static_assert(sizeof(MotionArgs) + 2 * 8 <= 4096 - 256 && sizeof(MotionGateArgs) + 8 * 8 <= 4096 - 256,
              "the tables travel as a kernel argument (4 KB at most, the hidden arguments included)");
static_assert(FFGPU_MOTION_DETS == 128 && FFGPU_MOTION_ROW == 16 && FFGPU_MOTION_WORDS == 8 && MOTION_STATE_HEADER == 16 && MOTION_TILE == 64 && WAVE == 64,
              "k_motion_*: the layouts of include/ffcnn_hip.h");

// The bytes o .. o + nb - 1 of a row of nrow bytes as ND aligned dwords (the bytes behind the run: anything).  Dword j of the ND + 1 that cover the
// run lies at offset o - sh + 4 j of the row, sh = the run's misalignment: loaded whole where it lies inside the row, byte by byte where it sticks
// out of it, not at all behind the run.
template <int ND>
__device__ __forceinline__ void motion_load(const unsigned char *row, int nrow, int o, int nb, bool eight, int &sh, unsigned (&d)[ND + 1])
{
    if (eight && nb == 4 * ND) {                                                      // a whole run of a target whose rows are 8-byte aligned: 8-byte loads
#pragma unroll
        for (int j = 0; j < ND; j += 2) {
            const uint2 v = *reinterpret_cast<const uint2 *>(row + o + 4 * j);
            d[j] = v.x; d[j + 1] = v.y;
        }
        d[ND] = 0; sh = 0;
        return;
    }
    sh = (int)(reinterpret_cast<uintptr_t>(row + o) & 3);
#pragma unroll
    for (int j = 0; j <= ND; j++) {
        const int oj = o - sh + 4 * j;
        unsigned v = 0;
        if (oj < o + nb) {
            if (oj >= 0 && oj + 4 <= nrow) v = *reinterpret_cast<const unsigned *>(row + oj);
            else
                for (int b = 0; b < 4; b++) if (oj + b >= 0 && oj + b < nrow) v |= (unsigned)row[oj + b] << (8 * b);
        }
        d[j] = v;
    }
}
// the luma of pixel i of a run from its aligned dwords
template <bool NV12>
__device__ __forceinline__ int motion_luma(const unsigned *a, int i)
{
    auto byte = [&](int n) { return (int)((a[n >> 2] >> (8 * (n & 3))) & 0xffu); };
    if (NV12) return byte(i);
    return (29 * byte(3 * i) + 150 * byte(3 * i + 1) + 77 * byte(3 * i + 2) + 128) >> 8;
}

// grid (tiles of a frame, targets of this launch), 256 lanes.  Every load and store lies inside the target's w x h pixels, the tile's rows of the
// plane (their padding is read with the last run, never written) and the tile's cells.
template <bool NV12>
__global__ void __launch_bounds__(256) k_motion_update(MotionArgs a, unsigned char *state)
{
    constexpr int BPP = NV12 ? 1 : 3, ND = 2 * BPP;
    __shared__ __attribute__((aligned(16))) unsigned short s_run[MOTION_TILE * 8];    // row r, run u: the changed of pixels 0..3 (low byte) and 4..7
    __shared__ int s_g[2][256];
    const DrawTarget &t = a.t[blockIdx.y];
    if (!t.p0) return;                                                                // a skipped target (uniform)
    const int w = a.w, h = a.h, k = a.k, tid = threadIdx.x;
    const int ntx = (w + MOTION_TILE - 1) / MOTION_TILE;
    const int bx0 = (int)(blockIdx.x % ntx) * MOTION_TILE, by0 = (int)(blockIdx.x / ntx) * MOTION_TILE;
    unsigned char *const sbase = state + (size_t)t.first * a.stream_bytes;
    const bool first = *reinterpret_cast<const int *>(sbase) == 0;                    // (uniform; k_motion_row writes it behind this launch)
    unsigned short *const plane = reinterpret_cast<unsigned short *>(sbase + MOTION_STATE_HEADER);
    const int u = tid & 7, x = bx0 + 8 * u, np = max(0, min(w - x, 8)), r0 = tid >> 3;
    const int thr = a.thr, ls = a.learn, lsc = a.learn_changed;
    const bool eight = ((reinterpret_cast<uintptr_t>(t.p0) | (uintptr_t)t.pitch) & 7) == 0;       // (uniform: a run starts 8 BPP u + 64 BPP tiles into its row)

    unsigned d[2][ND + 1];
    uint4 old[2];
    int sh[2];
#pragma unroll
    for (int p = 0; p < 2; p++) {
        const int y = by0 + r0 + 32 * p;
        sh[p] = 0; old[p] = make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int j = 0; j <= ND; j++) d[p][j] = 0;
        if (y < h && np > 0) {
            motion_load<ND>(t.p0 + (size_t)y * (size_t)t.pitch, BPP * w, BPP * x, BPP * np, eight, sh[p], d[p]);
            old[p] = *reinterpret_cast<const uint4 *>(plane + (size_t)y * (size_t)a.pitch + x);
        }
    }
#pragma unroll
    for (int p = 0; p < 2; p++) {
        const int r = r0 + 32 * p, y = by0 + r;
        unsigned cnt = 0;
        if (y < h && np > 0) {
            unsigned al[ND];
#pragma unroll
            for (int j = 0; j < ND; j++) al[j] = __builtin_amdgcn_alignbyte(d[p][j + 1], d[p][j], (unsigned)sh[p]);
            const unsigned ow[4] = { old[p].x, old[p].y, old[p].z, old[p].w };
            unsigned nw[4];
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int cur = motion_luma<NV12>(al, i) << 8, bg = (int)((ow[i >> 1] >> (16 * (i & 1))) & 0xffffu);
                const int dd = cur - bg, ad = abs(dd);
                const bool changed = !first && ad > thr && i < np;
                const int ks = changed ? lsc : ls;
                const int step = ks >= 16 ? 0 : (ad + (1 << ks) - 1) >> ks;
                const int nb = first ? cur : bg + (dd < 0 ? -step : step);
                cnt += (unsigned)changed << (8 * (i >> 2));
                if (i & 1) nw[i >> 1] |= (unsigned)nb << 16; else nw[i >> 1] = (unsigned)nb;
            }
            unsigned short *bp = plane + (size_t)y * (size_t)a.pitch + x;
            if (np == 8) *reinterpret_cast<uint4 *>(bp) = make_uint4(nw[0], nw[1], nw[2], nw[3]);
            else
                for (int i = 0; i < np; i++) bp[i] = (unsigned short)(nw[i >> 1] >> (16 * (i & 1)));
        }
        s_run[r * 8 + u] = (unsigned short)cnt;
    }
    __syncthreads();

    // the tile's cells: 16 x 16 cells of 4 pixels first (a lane each: 4 rows of its column of bytes), then 2 x 2 at a time up to the cell size
    {
        const unsigned char *b4 = reinterpret_cast<const unsigned char *>(s_run);
        const int c4 = tid & 15, rg = tid >> 4;
        s_g[0][tid] = (int)b4[(4 * rg) * 16 + c4] + (int)b4[(4 * rg + 1) * 16 + c4] + (int)b4[(4 * rg + 2) * 16 + c4] + (int)b4[(4 * rg + 3) * 16 + c4];
    }
    __syncthreads();
    for (int l = 1; l <= k - 2; l++) {                                                // (uniform)
        const int n = 16 >> l;
        if (tid < n * n) {
            const int i = tid & (n - 1), j = tid >> (4 - l);
            const int *src = s_g[(l - 1) & 1] + (2 * j) * (2 * n) + 2 * i;
            s_g[l & 1][tid] = src[0] + src[1] + src[2 * n] + src[2 * n + 1];
        }
        __syncthreads();
    }
    const int n = MOTION_TILE >> k;
    if (tid < n * n) {
        const int ci = (bx0 >> k) + (tid & (n - 1)), cj = (by0 >> k) + tid / n;
        if (ci < a.gw && cj < a.gh)
            reinterpret_cast<unsigned *>(sbase + a.cells_off)[(size_t)cj * (size_t)a.gw + ci] = (unsigned)s_g[(k - 2) & 1][tid];
    }
}

// grid = targets of this launch, 256 lanes: the row of a target whose frame k_motion_update has just taken, and the stream's `frames`
__global__ void __launch_bounds__(256) k_motion_row(MotionArgs a, unsigned char *state, int *rows)
{
    __shared__ int s_red[4];
    const DrawTarget &t = a.t[blockIdx.x];
    const int tid = threadIdx.x;
    int *const row = rows + (size_t)a.tgt[blockIdx.x] * FFGPU_MOTION_ROW;
    if (!t.p0) {                                                                      // a skipped target: the row is zero (uniform)
        if (tid < FFGPU_MOTION_ROW) row[tid] = 0;
        return;
    }
    unsigned char *const sbase = state + (size_t)t.first * a.stream_bytes;
    const unsigned frames = *reinterpret_cast<const unsigned *>(sbase);               // (every lane, in front of the folds' barriers and lane 0's store)
    const unsigned *const cell = reinterpret_cast<const unsigned *>(sbase + a.cells_off);
    const int gw = a.gw, ncell = gw * a.gh, big = 0x7fffffff;
    int sum = 0, act = 0, i0 = big, j0 = big, i1 = -1, j1 = -1;
    // four cells a load (the cells start 16-byte aligned and are rounded up to 16 bytes: the last load may reach into the rounding, which is masked),
    // four loads in flight
    const int nq = (ncell + 3) >> 2;
    for (int q0 = tid; q0 < nq; q0 += 4 * (int)blockDim.x) {
        uint4 v4[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int q = q0 + u * (int)blockDim.x;
            v4[u] = q < nq ? reinterpret_cast<const uint4 *>(cell)[q] : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int c0 = 4 * (q0 + u * (int)blockDim.x);
            const unsigned vv[4] = { v4[u].x, v4[u].y, v4[u].z, v4[u].w };
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int c = c0 + e;
                if (c < ncell) {
                    const int j = c / gw, i = c - j * gw;
                    sum += (int)vv[e];
                    if (vv[e] >= (unsigned)a.min_pixels) { act++; i0 = min(i0, i); j0 = min(j0, j); i1 = max(i1, i); j1 = max(j1, j); }
                }
            }
        }
    }
    auto add = [](int x, int y) { return x + y; };
    auto lo = [](int x, int y) { return min(x, y); };
    auto hi = [](int x, int y) { return max(x, y); };
    sum = block_fold(sum, s_red, 4, add); act = block_fold(act, s_red, 4, add);
    i0 = block_fold(i0, s_red, 4, lo); j0 = block_fold(j0, s_red, 4, lo); i1 = block_fold(i1, s_red, 4, hi); j1 = block_fold(j1, s_red, 4, hi);
    if (tid < FFGPU_MOTION_ROW) {
        const int k = a.k;
        int v = 0;
        if (tid == 0) v = (int)frames;
        if (tid == 1) v = sum;
        if (tid == 2) v = act;
        if (tid == 3) v = act ? i0 << k : 0;
        if (tid == 4) v = act ? j0 << k : 0;
        if (tid == 5) v = act ? min((i1 + 1) << k, a.w) - 1 : -1;
        if (tid == 6) v = act ? min((j1 + 1) << k, a.h) - 1 : -1;
        if (tid == 7) v = frames + 1u > (unsigned)a.warmup;
        row[tid] = v;
    }
    if (tid == 0) *reinterpret_cast<unsigned *>(sbase) = frames + 1u;
}

struct MotionGateLds {
    BBOX det[FFGPU_MOTION_DETS];                      // the considered boxes, in list order
    int  didx[FFGPU_MOTION_DETS];                     // their places in the list
    int  touched[FFGPU_MOTION_DETS], active[FFGPU_MOTION_DETS];
    int  wsum[4];
};

// grid = records of this launch (record t0 + blockIdx.x of the call), 256 lanes.  Counts are clamped to [0, stride] as the draw kernel clamps them.
// Only reads the state; total over any state bytes.
__global__ void __launch_bounds__(256) k_motion_gate(MotionGateArgs a, const ffgpu_frame_dets *recs, const BBOX *lists, int stride, const unsigned char *state, int t0,
                                                     int *words, ffgpu_frame_dets *out_recs, BBOX *out_lists)
{
    __shared__ MotionGateLds L;
    const int tid = threadIdx.x, e = blockIdx.x, vs = a.stream[e];
    const long t = (long)t0 + e;
    const long rowlen = FFGPU_MOTION_WORDS + 2 * (long)stride;
    int *const row = words + t * rowlen;
    if (vs < 0) {                                                                     // an ignored entry: every output byte zero (uniform)
        for (long i = tid; i < rowlen; i += blockDim.x) row[i] = 0;
        if (out_recs) for (int i = tid; i < (int)(sizeof(ffgpu_frame_dets) / sizeof(int)); i += blockDim.x) reinterpret_cast<int *>(out_recs + t)[i] = 0;
        if (out_lists) for (long i = tid; i < stride; i += blockDim.x) track_zero(out_lists + t * stride + i);
        return;
    }
    const unsigned char *const sbase = state + (size_t)vs * a.stream_bytes;
    const unsigned frames = *reinterpret_cast<const unsigned *>(sbase);
    const unsigned *const cell = reinterpret_cast<const unsigned *>(sbase + a.cells_off);
    const bool warm = frames > (unsigned)a.warmup;
    const ffgpu_frame_dets *rec = recs + t;
    const int n = max(0, min(lists ? rec->nfull : rec->count, stride)), ncand = rec->ncand, ovf = rec->overflow;
    const BBOX *list = lists ? lists + a.first[e] : rec->box;
    const float min_score = a.min_score;
    for (long i = tid; i < 2 * (long)stride; i += blockDim.x) row[FFGPU_MOTION_WORDS + i] = 0;

    // the considered boxes, in list order
    const long nq = block_consider(n, FFGPU_MOTION_DETS, L.wsum,
        [&](int i) { const BBOX &b = list[i]; return b.score >= min_score && (!a.nclasses || ((unsigned)b.type < (unsigned)a.nclasses && a.classes[(unsigned)b.type & 255u])); },
        [&](int ord, int i) { track_put(&L.det[ord], list[i].type, list[i]); L.didx[ord] = i; });
    const int nd = (int)min(nq, (long)FFGPU_MOTION_DETS), dropped = (int)min(nq - nd, 0x7fffffffL);

    // a wave per box: the cells its clipped region touches, lanes along a row of cells
    const int k = a.k, gw = a.gw, lane = tid & (WAVE - 1);
    for (int j = tid / WAVE; j < nd; j += 4) {                                        // (uniform per wave)
        const BBOX b = L.det[j];
        const int A = draw_f2i(b.x1), B = draw_f2i(b.y1), C = draw_f2i(b.x2), D = draw_f2i(b.y2);
        const int X0 = max(A, 0), Y0 = max(B, 0), X1 = min(C, a.w - 1), Y1 = min(D, a.h - 1);
        int touched = 0, act = 0;
        if (A <= C && B <= D && X0 <= X1 && Y0 <= Y1) {
            const int cx0 = X0 >> k, cy0 = Y0 >> k, cx1 = X1 >> k, cy1 = Y1 >> k;
            touched = (cx1 - cx0 + 1) * (cy1 - cy0 + 1);
            for (int cy = cy0; cy <= cy1; cy++)
                for (int cx = cx0 + lane; cx <= cx1; cx += WAVE) act += cell[(size_t)cy * (size_t)gw + cx] >= (unsigned)a.min_pixels;
            act = wave_fold(act, [](int x, int y) { return x + y; });
        }
        if (lane == 0) { L.touched[j] = touched; L.active[j] = act; }
    }
    __syncthreads();
    const bool box = tid < nd;
    const int touched = box ? L.touched[tid] : 0, act = box ? L.active[tid] : 0;
    const bool moving = box && (!warm || (touched >= 1 && (long long)act * 256 >= (long long)a.cover * touched));
    if (box) {
        row[FFGPU_MOTION_WORDS + 2 * L.didx[tid]] = touched;                          // (zeroed above, barriers in between)
        row[FFGPU_MOTION_WORDS + 2 * L.didx[tid] + 1] = act;
    }
    const int outside = __syncthreads_count(box && touched == 0), nmoving = __syncthreads_count(moving);
    const bool sel = box && (moving != (a.invert != 0));
    int nt;
    const int ord = block_rank(sel, L.wsum, 4, nt);                                   // (nt <= nd <= n <= stride)
    if (tid < FFGPU_MOTION_WORDS)
        row[tid] = tid == 0 ? nd : tid == 1 ? dropped : tid == 2 ? outside : tid == 3 ? nmoving : tid == 4 ? (int)warm : tid == 5 ? (int)frames : 0;
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
}

// ---- host side
extern "C" size_t ffgpu_motion_state_bytes(int nstreams, int w, int h, int cell_log2) { return ffgpu_motion_state_bytes_host(nstreams, w, h, cell_log2); }
extern "C" int ffgpu_motion_spec_check(const ffgpu_motion_spec *spec)
{
    MotionPlan pl;
    return ffgpu_motion_spec_plan("motion_spec_check", spec, pl);
}

extern "C" int ffgpu_motion_reset_dev(void *d_state, int nstreams, int w, int h, int cell_log2, int which_stream, void *stream)
{
    const char *const what = "motion_reset_dev";
    if (ffgpu_no_device(what)) return -1;
    const size_t all = ffgpu_motion_state_bytes(nstreams, w, h, cell_log2);
    if (!all) ffgpu_set_error("%s: %d streams of %d x %d pixels, cell_log2 %d (nstreams 1..65536, w and h 1..%d, cell_log2 2..6)", what, nstreams, w, h, cell_log2, FFGPU_MOTION_MAX_SIDE);   // (stands unless the state is NULL)
    return ffgpu_state_reset(what, d_state, all, nstreams, which_stream, stream);
}

// Round r of a call -- the r-th frame of every stream in it -- behind round r - 1, MOTION_ARG_TARGETS targets per launch: the update, then the rows
// and `frames`.  The skipped targets ride in round 0, where their zero rows are written.
template <class Frame>
static int motion_update_dev(const char *what, const Frame *targets, int ntargets, const int *streams, const ffgpu_motion_spec *spec, void *d_state, int nstreams,
                             void *d_rows, void *stream)
{
    const bool nv12 = std::is_same<Frame, ffgpu_nv12_frame>::value;
    if (ffgpu_no_device(what)) return -1;
    MotionPlan pl;
    std::vector<DrawTarget> tab;
    std::vector<int> round;
    const int nrounds = ffgpu_motion_update_args_check(what, targets, ntargets, streams, spec, d_state, nstreams, d_rows, pl, tab, round);
    if (nrounds < 0) return -1;
    std::vector<std::vector<int>> by((size_t)nrounds);
    for (int t = 0; t < ntargets; t++) by[(size_t)round[t]].push_back(t);
    const MotionLayout &l = pl.lay;
    const unsigned tiles = (unsigned)(((l.w + MOTION_TILE - 1) / MOTION_TILE) * ((l.h + MOTION_TILE - 1) / MOTION_TILE));
    for (int r = 0; r < nrounds; r++)
        for (size_t i0 = 0; i0 < by[(size_t)r].size(); i0 += MOTION_ARG_TARGETS) {
            const int nt = (int)std::min((size_t)MOTION_ARG_TARGETS, by[(size_t)r].size() - i0);
            MotionArgs a;
            memset(&a, 0, sizeof a);
            bool any = false;
            for (int i = 0; i < nt; i++) {
                a.tgt[i] = by[(size_t)r][i0 + (size_t)i];
                a.t[i] = tab[(size_t)a.tgt[i]];
                any |= a.t[i].p0 != nullptr;
            }
            a.w = l.w; a.h = l.h; a.k = l.cell_log2; a.gw = l.gw; a.gh = l.gh; a.pitch = l.pitch; a.thr = pl.threshold << 8; a.learn = pl.learn_shift;
            a.learn_changed = pl.learn_shift_changed; a.min_pixels = pl.min_pixels; a.warmup = pl.warmup; a.cells_off = l.cells_off; a.stream_bytes = l.stream_bytes;
            if (any) {
                if (nv12) hipLaunchKernelGGL(k_motion_update<true>, dim3(tiles, (unsigned)nt), dim3(256), 0, (hipStream_t)stream, a, (unsigned char *)d_state);
                else      hipLaunchKernelGGL(k_motion_update<false>, dim3(tiles, (unsigned)nt), dim3(256), 0, (hipStream_t)stream, a, (unsigned char *)d_state);
                LAUNCH_OK("motion_update");
            }
            hipLaunchKernelGGL(k_motion_row, dim3((unsigned)nt), dim3(256), 0, (hipStream_t)stream, a, (unsigned char *)d_state, (int *)d_rows);
            LAUNCH_OK("motion_row");
        }
    return 0;
}

extern "C" int ffgpu_motion_update_bgr_dev(const ffgpu_bgr_frame *targets, int ntargets, const int *streams, const ffgpu_motion_spec *spec, void *d_state,
                                           int nstreams, void *d_rows, void *stream)
{
    return motion_update_dev("motion_update_bgr_dev", targets, ntargets, streams, spec, d_state, nstreams, d_rows, stream);
}

extern "C" int ffgpu_motion_update_nv12_dev(const ffgpu_nv12_frame *targets, int ntargets, const int *streams, const ffgpu_motion_spec *spec, void *d_state,
                                            int nstreams, void *d_rows, void *stream)
{
    return motion_update_dev("motion_update_nv12_dev", targets, ntargets, streams, spec, d_state, nstreams, d_rows, stream);
}

// everything but the overlap has been checked
int ffgpu_launch_motion_gate(const DetSource &src, const int *streams, int ntargets, const MotionPlan &pl, const void *d_state, void *d_words, void *d_out_records,
                             void *d_out_lists, hipStream_t s)
{
    if ((const void *)src.recs == d_out_records || (src.lists && (const void *)src.lists == d_out_lists)) { ffgpu_set_error("motion_gate: the outputs must not overlap the inputs"); return -1; }
    for (int t0 = 0; t0 < ntargets; t0 += MOTION_ARG_TARGETS) {
        const int nt = std::min(MOTION_ARG_TARGETS, ntargets - t0);
        MotionGateArgs a;
        memset(&a, 0, sizeof a);
        memcpy(a.classes, pl.classes, sizeof a.classes);
        a.nclasses = pl.nclasses; a.w = pl.lay.w; a.h = pl.lay.h; a.k = pl.lay.cell_log2; a.gw = pl.lay.gw; a.min_pixels = pl.min_pixels; a.cover = pl.cover;
        a.warmup = pl.warmup; a.invert = pl.invert; a.min_score = pl.min_score; a.cells_off = pl.lay.cells_off; a.stream_bytes = pl.lay.stream_bytes;
        for (int i = 0; i < nt; i++) { a.first[i] = src.first[(size_t)(t0 + i)]; a.stream[i] = streams[t0 + i]; }
        hipLaunchKernelGGL(k_motion_gate, dim3((unsigned)nt), dim3(256), 0, s, a, src.recs, src.lists, src.stride, (const unsigned char *)d_state, t0, (int *)d_words,
                           (ffgpu_frame_dets *)d_out_records, (BBOX *)d_out_lists);
        LAUNCH_OK("motion_gate");
    }
    return 0;
}

extern "C" int ffgpu_motion_gate_dev(const void *d_records, const void *d_lists, int list_stride, const int *list_first, const int *streams, int ntargets,
                                     const ffgpu_motion_spec *spec, const void *d_state, int nstreams, void *d_words, void *d_out_records, void *d_out_lists,
                                     void *stream)
{
    const char *const what = "motion_gate_dev";
    if (ffgpu_no_device(what)) return -1;
    MotionPlan pl;
    if (ffgpu_motion_gate_args_check(what, streams, ntargets, spec, d_state, nstreams, d_words, d_out_records, d_out_lists, pl)) return -1;
    DetSource src;
    if (ffgpu_source_dev(what, d_records, d_lists, list_stride, list_first, ntargets, src)) return -1;
    return ffgpu_launch_motion_gate(src, streams, ntargets, pl, d_state, d_words, d_out_records, d_out_lists, (hipStream_t)stream);
}
