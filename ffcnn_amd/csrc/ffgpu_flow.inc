// ffgpu_flow.inc -- flow maps: per video stream the luma of the last two frames kept on the device, per block the integer vector that carries the
// previous frame's content into it (an exhaustive search by the sum of absolute differences), the vector most blocks agree on, and the motion of any
// record's boxes relative to it (ffgpu_flow_update_bgr_dev / _nv12_dev, ffgpu_flow_boxes_dev, ffgpu_exec_flow_boxes, ffgpu_flow_reset_dev,
// ffgpu_flow_state_bytes, ffgpu_flow_spec_check).  The contract is in include/ffcnn_hip.h; the host side (layout, spec, argument checks and the
// rounds of an update call) is ffgpu_flow_host.hpp.
//
// k_flow_match<NV12, K>: the first post-pass that is bound by arithmetic and LDS, not by memory: (2 r + 1)^2 byte differences a pixel.  A workgroup
// owns a tile of 64 x 32 pixels of its target: 32 blocks of 8 x 8 (K = 3) or 8 of 16 x 16 (K = 4).
//   1. A lane takes a run of 8 pixels (k_motion_update's loads: the aligned dwords that cover the run's bytes, shifted into place), makes the luma
//      once and puts it into the LDS tile s_cur; pixels outside the frame are 0 there.  128 lanes then store the tile into the current plane, 16
//      bytes a store; the ragged end of a row goes byte by byte, so the plane's padding is never written.
//   2. The previous plane's window -- the tile with a halo of r rows above and below and 16 columns left and right -- goes into s_win as ALIGNED
//      dwords: LDS column c is frame column bx0 - 16 + c, so a dword of the window is a dword of the plane.  Outside the plane: 0, never used:
//      an illegal candidate is excluded by its index, not by what the window holds there.
//   3. LPB = 256 / blocks lanes serve one block (8, or 32) and share its WORK ITEMS (vy, four consecutive vx): a lane walks the block's rows; per
//      row the cur dwords and NDW + 2 aligned window dwords are read from LDS, the misaligned window is built by v_alignbyte -- the shift is
//      (-r) & 3 for every item of the launch --, and one v_qsad_pk_u16_u8 per cur dword adds the four candidates' differences into a packed
//      16-bit accumulator pair (65280 fits).  A dword of a partial block's ragged edge takes four masked v_sad_u8 instead.
//   4. Per legal candidate a key: cost, then vx^2 + vy^2, then vy, then vx -- the contract's total order in one integer, so one min gives the winner
//      and settles every tie; a max over the cost gives the spread.  A lane folds its items, a butterfly the block's lanes; one lane stores the record.
// No atomics, no scratch.  The launch only READS the header.
//
// k_flow_row: one workgroup per target, behind the match launch of its round: the reliable blocks' vectors voted into a histogram in LDS (integer LDS
// atomics: a count is the same in any order), the argmax by a key, the header and the row written.  k_flow_boxes: one workgroup per record with
// k_motion_gate's list walk (block_consider); a wave takes a considered box and sums the reliable blocks under it, lanes along the blocks' rows.
struct FlowArgs {
    DrawTarget t[FLOW_ARG_TARGETS];                   // (first: the target's stream; p0 == NULL: skipped)
    int   tgt[FLOW_ARG_TARGETS];                      // the target's index in the call: its row
    int   w, h, gw, gh, pitch, range, min_spread, pad_;
    unsigned long long plane_bytes, recs_off, stream_bytes;
};
struct FlowBoxArgs {
    long long first[FLOW_ARG_TARGETS];                // record e of the launch: its list's first box in `lists`
    int   stream[FLOW_ARG_TARGETS];                   //                         its video stream, or -1
    unsigned char classes[256];
    int   nclasses, w, h, k, gw, min_spread;
    float min_score;
    int   pad_;
    unsigned long long recs_off, stream_bytes;
};
static_assert(sizeof(FlowArgs) + 8 <= 4096 - 256 && sizeof(FlowBoxArgs) + 6 * 8 <= 4096 - 256,
              "the tables travel as a kernel argument (4 KB at most, the hidden arguments included)");
static_assert(FFGPU_FLOW_DETS == 128 && FFGPU_FLOW_ROW == 16 && FFGPU_FLOW_WORDS == 8 && FLOW_STATE_HEADER == 16 && FLOW_TILE_W == 64 && FLOW_TILE_H == 32 &&
              FLOW_MAX_RANGE == 16 && WAVE == 64, "k_flow_*: the layouts of include/ffcnn_hip.h");
#define FLOW_WIN_DW   26                              // dwords a window row: 16 + 64 + 16 bytes and the two dwords the last item's second half reaches into
#define FLOW_WIN_ROWS (FLOW_TILE_H + 2 * FLOW_MAX_RANGE)
#define FLOW_TIE_BITS 22                              // vx^2 + vy^2 (<= 512: 10 bits), vy + 16 and vx + 16 (6 bits each)

// a candidate's place in the order (vx^2 + vy^2, vy, vx)
__device__ __forceinline__ unsigned flow_tie(int vx, int vy) { return (unsigned)(vx * vx + vy * vy) << 12 | (unsigned)(vy + 16) << 6 | (unsigned)(vx + 16); }

// Four candidates' differences over one dword of the block's row: src = 8 window bytes, candidate k reads its bytes k .. k + 3.  nvalid: the dword's
// pixels inside the frame, from the left; the others count for nothing.
__device__ __forceinline__ unsigned long long flow_sad4(unsigned long long src, unsigned cur, unsigned long long acc, int nvalid)
{
    if (nvalid >= 4) return __builtin_amdgcn_qsad_pk_u16_u8(src, cur, acc);
    const unsigned m = nvalid <= 0 ? 0u : (1u << (8 * nvalid)) - 1u;
#pragma unroll
    for (int k = 0; k < 4; k++) acc += (unsigned long long)__builtin_amdgcn_sad_u8((unsigned)(src >> (8 * k)) & m, cur & m, 0u) << (16 * k);
    return acc;
}

// grid (tiles of a frame, targets of this launch), 256 lanes.  Every load lies inside the target's w x h pixels and the previous plane's rows (their
// padding may be read, never used); every store inside the current plane's w x h bytes and the tile's records.
template <bool NV12, int K>
__global__ void __launch_bounds__(256) k_flow_match(FlowArgs a, unsigned char *state)
{
    constexpr int BPP = NV12 ? 1 : 3, ND = 2 * BPP, B = 1 << K, NBX = FLOW_TILE_W / B, NB = NBX * (FLOW_TILE_H / B), LPB = 256 / NB, NDW = B / 4, CDW = FLOW_TILE_W / 4;
    __shared__ __attribute__((aligned(16))) unsigned s_cur[FLOW_TILE_H * CDW];
    __shared__ __attribute__((aligned(16))) unsigned s_win[FLOW_WIN_ROWS * FLOW_WIN_DW];
    const DrawTarget &t = a.t[blockIdx.y];
    if (!t.p0) return;                                                                // a skipped target (uniform)
    const int w = a.w, h = a.h, r = a.range, tid = threadIdx.x;
    const int ntx = (w + FLOW_TILE_W - 1) / FLOW_TILE_W;
    const int bx0 = (int)(blockIdx.x % ntx) * FLOW_TILE_W, by0 = (int)(blockIdx.x / ntx) * FLOW_TILE_H;
    unsigned char *const sbase = state + (size_t)t.first * a.stream_bytes;
    const unsigned f = *reinterpret_cast<const unsigned *>(sbase);                    // (uniform; k_flow_row writes it behind this launch)
    unsigned char *const cur_plane = sbase + FLOW_STATE_HEADER + (size_t)(f & 1u) * a.plane_bytes;
    const unsigned char *const prev_plane = sbase + FLOW_STATE_HEADER + (size_t)((f & 1u) ^ 1u) * a.plane_bytes;

    // 1. the tile's luma
    {
        const int u = tid & 7, row = tid >> 3, x = bx0 + 8 * u, y = by0 + row, np = max(0, min(w - x, 8));
        const bool eight = ((reinterpret_cast<uintptr_t>(t.p0) | (uintptr_t)t.pitch) & 7) == 0;
        unsigned lo = 0, hi = 0;
        if (y < h && np > 0) {
            unsigned d[ND + 1], al[ND];
            int sh;
            motion_load<ND>(t.p0 + (size_t)y * (size_t)t.pitch, BPP * w, BPP * x, BPP * np, eight, sh, d);
#pragma unroll
            for (int j = 0; j < ND; j++) al[j] = __builtin_amdgcn_alignbyte(d[j + 1], d[j], (unsigned)sh);
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const unsigned v = i < np ? (unsigned)motion_luma<NV12>(al, i) << (8 * (i & 3)) : 0u;
                if (i < 4) lo |= v; else hi |= v;
            }
        }
        s_cur[row * CDW + 2 * u] = lo;
        s_cur[row * CDW + 2 * u + 1] = hi;
    }
    // 2. the previous plane's window (the first frame of a stream has none)
    if (f != 0u) {
        const int n = (FLOW_TILE_H + 2 * r) * FLOW_WIN_DW;
        for (int i = tid; i < n; i += 256) {
            const int wr = i / FLOW_WIN_DW, y = by0 - r + wr, x = bx0 - 16 + 4 * (i - wr * FLOW_WIN_DW);
            unsigned v = 0;
            if (y >= 0 && y < h && x >= 0 && x < a.pitch) v = *reinterpret_cast<const unsigned *>(prev_plane + (size_t)y * (size_t)a.pitch + x);
            s_win[i] = v;
        }
    }
    __syncthreads();
    if (tid < 128) {                                                                  // the tile into the current plane: 4 stores of 16 bytes a row
        const int row = tid >> 2, c = tid & 3, x = bx0 + 16 * c, y = by0 + row, n = min(16, w - x);
        if (y < h && n > 0) {
            unsigned char *p = cur_plane + (size_t)y * (size_t)a.pitch + x;
            if (n == 16) *reinterpret_cast<uint4 *>(p) = *reinterpret_cast<const uint4 *>(s_cur + row * CDW + 4 * c);
            else {
                const unsigned char *s = reinterpret_cast<const unsigned char *>(s_cur + row * CDW + 4 * c);
                for (int i = 0; i < n; i++) p[i] = s[i];
            }
        }
    }

    // 3. the block's work items over its lanes
    const int blk = tid / LPB, sub = tid % LPB;
    const int lbx = (blk % NBX) * B, lby = (blk / NBX) * B, bx = bx0 + lbx, by = by0 + lby;
    const bool live = bx < w && by < h;
    const int bw = min(B, w - bx), bh = min(B, h - by);
    unsigned long long best = ~0ull;
    unsigned worst = 0;
    if (f != 0u && live) {
        // p - v inside the frame for every pixel p of the block
        const int vx_lo = max(-r, bx + bw - w), vx_hi = min(r, bx), vy_lo = max(-r, by + bh - h), vy_hi = min(r, by);
        const int G = (2 * r + 4) >> 2, nitems = (2 * r + 1) * G;                      // G groups of four vx cover -r .. r
        const unsigned sh = (unsigned)(-r) & 3u;
        for (int it = sub; it < nitems; it += LPB) {
            const int vyi = it / G, vy = vyi - r, vxh = r - 4 * (it - vyi * G);       // the item's candidates: vx = vxh - k, k = 0 .. 3
            if (vy < vy_lo || vy > vy_hi || vxh - 3 > vx_hi || vxh < vx_lo) continue;
            const unsigned *wrow = s_win + (lby - vy + r) * FLOW_WIN_DW + ((lbx - vxh + 16) >> 2);    // (the column's low bits are sh)
            const unsigned *crow = s_cur + lby * CDW + (lbx >> 2);
            unsigned long long acc = 0;
            for (int y = 0; y < bh; y++, wrow += FLOW_WIN_DW, crow += CDW) {
                unsigned d[NDW + 2], al[NDW + 1];
#pragma unroll
                for (int j = 0; j < NDW + 2; j++) d[j] = wrow[j];
#pragma unroll
                for (int j = 0; j <= NDW; j++) al[j] = __builtin_amdgcn_alignbyte(d[j + 1], d[j], sh);
#pragma unroll
                for (int j = 0; j < NDW; j++) acc = flow_sad4((unsigned long long)al[j + 1] << 32 | al[j], crow[j], acc, bw - 4 * j);
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int vx = vxh - k;
                const unsigned c = (unsigned)(acc >> (16 * k)) & 0xffffu;
                if (vx >= vx_lo && vx <= vx_hi) {
                    const unsigned long long key = (unsigned long long)c << FLOW_TIE_BITS | flow_tie(vx, vy);
                    best = key < best ? key : best;
                    worst = max(worst, c);
                }
            }
        }
    }
    // 4. the block's lanes folded (every lane of the wave takes part; a block's lanes are LPB consecutive ones)
#pragma unroll
    for (int o = LPB / 2; o > 0; o >>= 1) {
        const unsigned olo = __shfl_xor((unsigned)best, o), ohi = __shfl_xor((unsigned)(best >> 32), o), ow = __shfl_xor(worst, o);
        const unsigned long long ob = (unsigned long long)ohi << 32 | olo;
        best = ob < best ? ob : best;
        worst = max(worst, ow);
    }
    if (sub == 0 && live) {
        uint2 rec = make_uint2(0u, 0u);
        if (f != 0u) {                                                                // (the zero vector is a candidate: best is set)
            const unsigned cost = (unsigned)(best >> FLOW_TIE_BITS);
            const int dx = (int)((unsigned)best & 63u) - 16, dy = (int)(((unsigned)best >> 6) & 63u) - 16;
            rec.x = ((unsigned)dx & 0xffffu) | (unsigned)dy << 16;
            rec.y = cost | min(worst - cost, 65535u) << 16;
        }
        reinterpret_cast<uint2 *>(sbase + a.recs_off)[(size_t)(by >> K) * (size_t)a.gw + (bx >> K)] = rec;
    }
}

// grid = targets of this launch, 256 lanes: the global vector and the row of a target whose frame k_flow_match has just taken, and the stream's header
__global__ void __launch_bounds__(256) k_flow_row(FlowArgs a, unsigned char *state, int *rows)
{
    __shared__ int s_hist[(2 * FLOW_MAX_RANGE + 1) * (2 * FLOW_MAX_RANGE + 1)];
    __shared__ unsigned long long s_key[4];
    __shared__ int s_red[4];
    const DrawTarget &t = a.t[blockIdx.x];
    const int tid = threadIdx.x;
    int *const row = rows + (size_t)a.tgt[blockIdx.x] * FFGPU_FLOW_ROW;
    if (!t.p0) {                                                                      // a skipped target: the row is zero (uniform)
        if (tid < FFGPU_FLOW_ROW) row[tid] = 0;
        return;
    }
    unsigned char *const sbase = state + (size_t)t.first * a.stream_bytes;
    const unsigned frames = *reinterpret_cast<const unsigned *>(sbase);               // (every lane, in front of the barriers and lane 0's store)
    const uint2 *const rec = reinterpret_cast<const uint2 *>(sbase + a.recs_off);
    const int r = a.range, side = 2 * r + 1, nblk = a.gw * a.gh;
    const unsigned thr = (unsigned)max(a.min_spread, 1);
    for (int i = tid; i < side * side; i += 256) s_hist[i] = 0;
    __syncthreads();
    int nrel = 0;
    for (int i = tid; i < nblk; i += 256) {
        const uint2 v = rec[i];
        if ((v.y >> 16) < thr) continue;
        const int dx = (short)(v.x & 0xffffu), dy = (short)(v.x >> 16);
        nrel++;
        if (abs(dx) <= r && abs(dy) <= r) atomicAdd(&s_hist[(dy + r) * side + dx + r], 1);       // (what k_flow_match stores always is)
    }
    __syncthreads();
    // the most blocks, then the least under (vx^2 + vy^2, vy, vx): one max over a key
    unsigned long long key = 0;
    for (int i = tid; i < side * side; i += 256) {
        const int c = s_hist[i], vyi = i / side;
        if (c > 0) {
            const unsigned long long k = (unsigned long long)c << FLOW_TIE_BITS | (0x3fffffu - flow_tie(i - vyi * side - r, vyi - r));
            key = k > key ? k : key;
        }
    }
    key = block_fold(key, s_key, 4, [](unsigned long long x, unsigned long long y) { return x > y ? x : y; });
    nrel = block_fold(nrel, s_red, 4, [](int x, int y) { return x + y; });
    const int support = (int)(key >> FLOW_TIE_BITS);
    const unsigned tie = 0x3fffffu - ((unsigned)key & 0x3fffffu);
    const int gdx = support ? (int)(tie & 63u) - 16 : 0, gdy = support ? (int)((tie >> 6) & 63u) - 16 : 0;
    if (tid < FFGPU_FLOW_ROW) {
        int v = 0;
        if (tid == 0) v = (int)frames;
        if (tid == 1) v = nblk;
        if (tid == 2) v = nrel;
        if (tid == 3) v = nrel - support;
        if (tid == 4) v = gdx;
        if (tid == 5) v = gdy;
        if (tid == 6) v = support;
        row[tid] = v;
    }
    if (tid == 0) *reinterpret_cast<int4 *>(sbase) = make_int4((int)(frames + 1u), gdx, gdy, support);
}

struct FlowBoxLds {
    BBOX det[FFGPU_FLOW_DETS];                        // the considered boxes, in list order
    int  didx[FFGPU_FLOW_DETS];                       // their places in the list
    int  out[FFGPU_FLOW_DETS][4];                     // touched, reliable, sum_dx, sum_dy
    int  wsum[4];
};

// grid = records of this launch (record t0 + blockIdx.x of the call), 256 lanes.  Counts are clamped to [0, stride] as the draw kernel clamps them.
// Only reads the state; total over any state bytes: the sums wrap.
__global__ void __launch_bounds__(256) k_flow_boxes(FlowBoxArgs a, const ffgpu_frame_dets *recs, const BBOX *lists, int stride, const unsigned char *state, int t0, int *words)
{
    __shared__ FlowBoxLds L;
    const int tid = threadIdx.x, e = blockIdx.x, vs = a.stream[e];
    const long t = (long)t0 + e;
    const long rowlen = FFGPU_FLOW_WORDS + 4 * (long)stride;
    int *const row = words + t * rowlen;
    if (vs < 0) {                                                                     // an ignored entry: every output byte zero (uniform)
        for (long i = tid; i < rowlen; i += blockDim.x) row[i] = 0;
        return;
    }
    const unsigned char *const sbase = state + (size_t)vs * a.stream_bytes;
    const int4 hdr = *reinterpret_cast<const int4 *>(sbase);                          // frames, gdx, gdy, support
    const uint2 *const brec = reinterpret_cast<const uint2 *>(sbase + a.recs_off);
    const ffgpu_frame_dets *rec = recs + t;
    const int n = max(0, min(lists ? rec->nfull : rec->count, stride));
    const BBOX *list = lists ? lists + a.first[e] : rec->box;
    const float min_score = a.min_score;
    for (long i = tid; i < 4 * (long)stride; i += blockDim.x) row[FFGPU_FLOW_WORDS + i] = 0;

    // the considered boxes, in list order
    const long nq = block_consider(n, FFGPU_FLOW_DETS, L.wsum,
        [&](int i) { const BBOX &b = list[i]; return b.score >= min_score && (!a.nclasses || ((unsigned)b.type < (unsigned)a.nclasses && a.classes[(unsigned)b.type & 255u])); },
        [&](int ord, int i) { track_put(&L.det[ord], list[i].type, list[i]); L.didx[ord] = i; });
    const int nd = (int)min(nq, (long)FFGPU_FLOW_DETS), dropped = (int)min(nq - nd, 0x7fffffffL);

    // a wave per box: the blocks its clipped region touches, lanes along a row of blocks
    const int k = a.k, gw = a.gw, lane = tid & (WAVE - 1);
    const unsigned thr = (unsigned)max(a.min_spread, 1);
    auto add = [](unsigned x, unsigned y) { return x + y; };
    for (int j = tid / WAVE; j < nd; j += 4) {                                        // (uniform per wave)
        const BBOX b = L.det[j];
        const int A = draw_f2i(b.x1), B = draw_f2i(b.y1), C = draw_f2i(b.x2), D = draw_f2i(b.y2);
        const int X0 = max(A, 0), Y0 = max(B, 0), X1 = min(C, a.w - 1), Y1 = min(D, a.h - 1);
        int touched = 0;
        unsigned rel = 0, sx = 0, sy = 0;
        if (A <= C && B <= D && X0 <= X1 && Y0 <= Y1) {
            const int cx0 = X0 >> k, cy0 = Y0 >> k, cx1 = X1 >> k, cy1 = Y1 >> k;
            touched = (cx1 - cx0 + 1) * (cy1 - cy0 + 1);
            for (int cy = cy0; cy <= cy1; cy++)
                for (int cx = cx0 + lane; cx <= cx1; cx += WAVE) {
                    const uint2 v = brec[(size_t)cy * (size_t)gw + cx];
                    if ((v.y >> 16) < thr) continue;
                    rel++;
                    sx += (unsigned)(int)(short)(v.x & 0xffffu) - (unsigned)hdr.y;
                    sy += (unsigned)(int)(short)(v.x >> 16) - (unsigned)hdr.z;
                }
            rel = wave_fold(rel, add); sx = wave_fold(sx, add); sy = wave_fold(sy, add);
        }
        if (lane == 0) { L.out[j][0] = touched; L.out[j][1] = (int)rel; L.out[j][2] = (int)sx; L.out[j][3] = (int)sy; }
    }
    __syncthreads();
    const bool box = tid < nd;
    if (box)
        for (int i = 0; i < 4; i++) row[FFGPU_FLOW_WORDS + 4 * (long)L.didx[tid] + i] = L.out[tid][i];        // (zeroed above, barriers in between)
    const int outside = __syncthreads_count(box && L.out[tid & (FFGPU_FLOW_DETS - 1)][0] == 0);
    if (tid < FFGPU_FLOW_WORDS)
        row[tid] = tid == 0 ? nd : tid == 1 ? dropped : tid == 2 ? outside : tid == 3 ? hdr.x : tid == 4 ? hdr.y : tid == 5 ? hdr.z : tid == 6 ? hdr.w : 0;
}

// ---- host side
extern "C" size_t ffgpu_flow_state_bytes(int nstreams, int w, int h, int block_log2) { return ffgpu_flow_state_bytes_host(nstreams, w, h, block_log2); }
extern "C" int ffgpu_flow_spec_check(const ffgpu_flow_spec *spec)
{
    FlowPlan pl;
    return ffgpu_flow_spec_plan("flow_spec_check", spec, pl);
}

extern "C" int ffgpu_flow_reset_dev(void *d_state, int nstreams, int w, int h, int block_log2, int which_stream, void *stream)
{
    const char *const what = "flow_reset_dev";
    if (ffgpu_no_device(what)) return -1;
    const size_t all = ffgpu_flow_state_bytes(nstreams, w, h, block_log2);
    if (!all) ffgpu_set_error("%s: %d streams of %d x %d pixels, block_log2 %d (nstreams 1..65536, w and h 1..%d, block_log2 3..4)", what, nstreams, w, h, block_log2, FFGPU_FLOW_MAX_SIDE);   // (stands unless the state is NULL)
    return ffgpu_state_reset(what, d_state, all, nstreams, which_stream, stream);
}

template <bool NV12>
static void flow_match_launch(int k, dim3 grid, hipStream_t s, const FlowArgs &a, unsigned char *state)
{
    if (k == 3) hipLaunchKernelGGL((k_flow_match<NV12, 3>), grid, dim3(256), 0, s, a, state);
    else        hipLaunchKernelGGL((k_flow_match<NV12, 4>), grid, dim3(256), 0, s, a, state);
}

// Round r of a call -- the r-th frame of every stream in it -- behind round r - 1, FLOW_ARG_TARGETS targets per launch: the match, then the global
// vectors, the rows and the headers.  The skipped targets ride in round 0, where their zero rows are written.
template <class Frame>
static int flow_update_dev(const char *what, const Frame *targets, int ntargets, const int *streams, const ffgpu_flow_spec *spec, void *d_state, int nstreams,
                           void *d_rows, void *stream)
{
    const bool nv12 = std::is_same<Frame, ffgpu_nv12_frame>::value;
    if (ffgpu_no_device(what)) return -1;
    FlowPlan pl;
    std::vector<DrawTarget> tab;
    std::vector<int> round;
    const int nrounds = ffgpu_flow_update_args_check(what, targets, ntargets, streams, spec, d_state, nstreams, d_rows, pl, tab, round);
    if (nrounds < 0) return -1;
    std::vector<std::vector<int>> by((size_t)nrounds);
    for (int t = 0; t < ntargets; t++) by[(size_t)round[t]].push_back(t);
    const FlowLayout &l = pl.lay;
    const unsigned tiles = (unsigned)(((l.w + FLOW_TILE_W - 1) / FLOW_TILE_W) * ((l.h + FLOW_TILE_H - 1) / FLOW_TILE_H));
    for (int r = 0; r < nrounds; r++)
        for (size_t i0 = 0; i0 < by[(size_t)r].size(); i0 += FLOW_ARG_TARGETS) {
            const int nt = (int)std::min((size_t)FLOW_ARG_TARGETS, by[(size_t)r].size() - i0);
            FlowArgs a;
            memset(&a, 0, sizeof a);
            bool any = false;
            for (int i = 0; i < nt; i++) {
                a.tgt[i] = by[(size_t)r][i0 + (size_t)i];
                a.t[i] = tab[(size_t)a.tgt[i]];
                any |= a.t[i].p0 != nullptr;
            }
            a.w = l.w; a.h = l.h; a.gw = l.gw; a.gh = l.gh; a.pitch = l.pitch; a.range = pl.range; a.min_spread = pl.min_spread;
            a.plane_bytes = l.plane_bytes; a.recs_off = l.recs_off; a.stream_bytes = l.stream_bytes;
            if (any) {
                if (nv12) flow_match_launch<true>(l.block_log2, dim3(tiles, (unsigned)nt), (hipStream_t)stream, a, (unsigned char *)d_state);
                else      flow_match_launch<false>(l.block_log2, dim3(tiles, (unsigned)nt), (hipStream_t)stream, a, (unsigned char *)d_state);
                LAUNCH_OK("flow_match");
            }
            hipLaunchKernelGGL(k_flow_row, dim3((unsigned)nt), dim3(256), 0, (hipStream_t)stream, a, (unsigned char *)d_state, (int *)d_rows);
            LAUNCH_OK("flow_row");
        }
    return 0;
}

extern "C" int ffgpu_flow_update_bgr_dev(const ffgpu_bgr_frame *targets, int ntargets, const int *streams, const ffgpu_flow_spec *spec, void *d_state,
                                         int nstreams, void *d_rows, void *stream)
{
    return flow_update_dev("flow_update_bgr_dev", targets, ntargets, streams, spec, d_state, nstreams, d_rows, stream);
}

extern "C" int ffgpu_flow_update_nv12_dev(const ffgpu_nv12_frame *targets, int ntargets, const int *streams, const ffgpu_flow_spec *spec, void *d_state,
                                          int nstreams, void *d_rows, void *stream)
{
    return flow_update_dev("flow_update_nv12_dev", targets, ntargets, streams, spec, d_state, nstreams, d_rows, stream);
}

int ffgpu_launch_flow_boxes(const DetSource &src, const int *streams, int ntargets, const FlowPlan &pl, const void *d_state, void *d_words, hipStream_t s)
{
    for (int t0 = 0; t0 < ntargets; t0 += FLOW_ARG_TARGETS) {
        const int nt = std::min(FLOW_ARG_TARGETS, ntargets - t0);
        FlowBoxArgs a;
        memset(&a, 0, sizeof a);
        memcpy(a.classes, pl.classes, sizeof a.classes);
        a.nclasses = pl.nclasses; a.w = pl.lay.w; a.h = pl.lay.h; a.k = pl.lay.block_log2; a.gw = pl.lay.gw; a.min_spread = pl.min_spread; a.min_score = pl.min_score;
        a.recs_off = pl.lay.recs_off; a.stream_bytes = pl.lay.stream_bytes;
        for (int i = 0; i < nt; i++) { a.first[i] = src.first[(size_t)(t0 + i)]; a.stream[i] = streams[t0 + i]; }
        hipLaunchKernelGGL(k_flow_boxes, dim3((unsigned)nt), dim3(256), 0, s, a, src.recs, src.lists, src.stride, (const unsigned char *)d_state, t0, (int *)d_words);
        LAUNCH_OK("flow_boxes");
    }
    return 0;
}

extern "C" int ffgpu_flow_boxes_dev(const void *d_records, const void *d_lists, int list_stride, const int *list_first, const int *streams, int ntargets,
                                    const ffgpu_flow_spec *spec, const void *d_state, int nstreams, void *d_words, void *stream)
{
    const char *const what = "flow_boxes_dev";
    if (ffgpu_no_device(what)) return -1;
    FlowPlan pl;
    if (ffgpu_flow_boxes_args_check(what, streams, ntargets, spec, d_state, nstreams, d_words, pl)) return -1;
    DetSource src;
    if (ffgpu_source_dev(what, d_records, d_lists, list_stride, list_first, ntargets, src)) return -1;
    return ffgpu_launch_flow_boxes(src, streams, ntargets, pl, d_state, d_words, (hipStream_t)stream);
}
