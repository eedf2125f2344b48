// ffgpu_block.inc -- the workgroup primitives of the detection tail and the post-passes (k_nms, k_merge_tiles, k_track, k_feat_pool, k_feat_post,
// k_topk, k_match, k_match_merge, k_enroll_decide, k_zones, k_trails, k_heat_accumulate, k_motion_row, k_motion_gate).  Device code only.  Every one of those kernels is held byte for byte to a Python restatement, so
// the ordering rule of a sort, the tie rule of a selection and the rounding of an overlap are part of a contract: each is written HERE, once, and what
// differs between two kernels (array layouts, padding values, which slots start dead, how a record is written) stays at the call site.
//
// No state, no options: a caller passes its arrays or a lambda.  A primitive that folds the waves' results takes `nw`, the waves it folds, and an LDS
// array with one slot per wave.  The pragma is lexical and does not follow a call: every function with floating-point arithmetic carries its own.

// ---- boxes.  A box is anything with x1, y1, x2, y2 (BBOX, ffgpu_track).
// (width and height of a box are kept out of ONE register pair: hipcc otherwise forms v_pk_mul_f32 v[a:b], v[a:b], v[a:b] op_sel:[0,1] ..., the operand
//  pattern of the packed-math slip under concurrent bf16 MFMAs -- see pw_fma4_apart in ffgpu_pw_mfma.inc)
__device__ __forceinline__ float box_area(float x1, float y1, float x2, float y2)
{
#pragma clang fp contract(off)
    float w = x2 - x1;
    asm volatile("" : "+v"(w));
    return w * (y2 - y1);
}

// intersection of a and b and b's area; a's area comes from the caller (box_area), who may have it from outside a loop over b
template <class A, class B>
__device__ __forceinline__ void box_overlap(const A &a, const B &b, float &inter, float &area_b)
{
#pragma clang fp contract(off)
    const float xa = a.x1 > b.x1 ? a.x1 : b.x1, ya = a.y1 > b.y1 ? a.y1 : b.y1;
    const float xb = a.x2 < b.x2 ? a.x2 : b.x2, yb = a.y2 < b.y2 ? a.y2 : b.y2;
    inter = (xa < xb && ya < yb) ? box_area(xa, ya, xb, yb) : 0.f;
    area_b = box_area(b.x1, b.y1, b.x2, b.y2);
}
__device__ __forceinline__ float box_iou(float inter, float area_a, float area_b)
{
#pragma clang fp contract(off)
    const float uni = area_a + area_b - inter;
    return inter / uni;
}
// the suppression metric of ffcnn.c:298-322: inter / min(area), or IoU
__device__ __forceinline__ float box_metric(float inter, float area_a, float area_b, int use_min)
{
#pragma clang fp contract(off)
    return use_min ? inter / (area_a < area_b ? area_a : area_b) : box_iou(inter, area_a, area_b);
}

// ---- sort, suppress, compact (k_nms, k_merge_tiles)
// bitonic sort of slots 0 .. pow2 - 1 (a power of two; the caller pads): precedes(i, l) is the order, swap(i, l) exchanges the two slots in every array
template <class Precedes, class Swap>
__device__ __forceinline__ void block_bitonic(int pow2, Precedes precedes, Swap swap)
{
    for (int k = 2; k <= pow2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < pow2; i += blockDim.x) {
                const int l = i ^ j;
                if (l > i && precedes(i, l) != ((i & k) == 0)) swap(i, l);
            }
            __syncthreads();
        }
}

// greedy class-aware suppression (ffcnn.c:298-322) over the m sorted slots: box_of(i) is the i-th BBOX in sorted order; a serial, j > a parallel, one
// barrier per kept a.  The caller has set alive[0 .. m) and passed a barrier: which slots start dead is its own rule.
template <class Alive, class BoxOf>
__device__ __forceinline__ void block_suppress(int m, Alive *alive, BoxOf box_of, float thresh, int use_min)
{
#pragma clang fp contract(off)
    for (int a = 0; a < m; a++) {
        if (!alive[a]) continue;                         // uniform: read after a barrier
        const BBOX ba = box_of(a);
        const float area_a = box_area(ba.x1, ba.y1, ba.x2, ba.y2);
        for (int j = a + 1 + threadIdx.x; j < m; j += blockDim.x) {
            if (!alive[j]) continue;
            const BBOX bj = box_of(j);
            if (bj.type != ba.type) continue;
            float inter, area_j;
            box_overlap(ba, bj, inter, area_j);
            if (box_metric(inter, area_a, area_j, use_min) > thresh) alive[j] = 0;
        }
        __syncthreads();
    }
}

// survivors in sorted order: keep[0 .. n) = idx of the alive slots; n in every lane.  One thread walks the list -- the survivors' order is the contract.
template <class Alive>
__device__ __forceinline__ int block_compact(int m, const Alive *alive, const int *idx, int *keep)
{
    __shared__ int s_nkeep;
    if (threadIdx.x == 0) {
        int n = 0;
        for (int i = 0; i < m; i++) if (alive[i]) keep[n++] = idx[i];
        s_nkeep = n;
    }
    __syncthreads();
    return s_nkeep;
}

// ---- selection in rounds (k_topk, k_match, k_match_merge): pairs (value, index) in the order "value descending, then index ascending"; index < 0: no pair.
// Round r takes the first pair behind round r - 1's.
// (ov, oi) replaces (bv, bi) if it precedes it
__device__ __forceinline__ void pair_take(float &bv, int &bi, float ov, int oi)
{
    if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
}
// is (v, i) strictly behind the previous round's pair (pv, pi)?
__device__ __forceinline__ bool pair_behind(float v, int i, float pv, int pi, bool first_round)
{
    return first_round || v < pv || (v == pv && i > pi);
}
// the lanes' candidates -> the workgroup's first pair, in every lane: a wave butterfly, the waves' results in LDS, every lane folding them in wave order
__device__ __forceinline__ void block_first_pair(float &bv, int &bi, float *s_v, int *s_i, int nw)
{
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    for (int s = WAVE / 2; s > 0; s >>= 1) { const float ov = __shfl_xor(bv, s); const int oi = __shfl_xor(bi, s); pair_take(bv, bi, ov, oi); }
    if (lane == 0) { s_v[wave] = bv; s_i[wave] = bi; }
    __syncthreads();
    bv = s_v[0]; bi = s_i[0];
    for (int w = 1; w < nw; w++) pair_take(bv, bi, s_v[w], s_i[w]);
    __syncthreads();
}

// ---- ranks.  This lane's rank, in lane order, among the flagged lanes of its group of gw consecutive waves (gw == the workgroup's waves, up to 16: of
// the workgroup), and the group's total.  wsum[w] is left holding wave w's count; it is free again behind the caller's next barrier.
__device__ __forceinline__ int block_rank(bool flag, int *wsum, int gw, int &total)
{
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE, w0 = wave - wave % gw;
    const unsigned long long m = __ballot(flag);
    if (lane == 0) wsum[wave] = __popcll(m);
    __syncthreads();
    int before = 0;
    total = 0;
    for (int w = w0; w < w0 + gw; w++) { const int c = wsum[w]; before += w < wave ? c : 0; total += c; }
    return before + __popcll(m & ((1ull << lane) - 1ull));
}
__device__ __forceinline__ int block_rank(bool flag, int *wsum, int gw) { int total; return block_rank(flag, wsum, gw, total); }

// ---- identified boxes against a stream's slots (k_zones, k_trails): a workgroup of 256 lanes, lanes 0..127 the boxes, lanes 128..255 the slots.
// The qualifying entries of a list of n, compacted in list order: put(ord, k) for the ord-th qualifying entry k while ord < cap.  Returns how many
// qualify (uniform).  wsum: 4 slots; ends in a barrier.
template <class Qual, class Put>
__device__ __forceinline__ long block_consider(int n, int cap, int *wsum, Qual qual, Put put)
{
    long nq = 0;
    for (int k0 = 0; k0 < n; k0 += 256) {
        const int k = k0 + threadIdx.x;
        const bool q = k < n && qual(k);
        int tot;
        const long ord = nq + block_rank(q, wsum, 4, tot);
        if (q && ord < cap) put((int)ord, k);
        nq += tot;
        __syncthreads();
    }
    return nq;
}
// an earlier box of the frame has box j's identity (no early exit: the loads do not wait for each other)
__device__ __forceinline__ bool ident_duplicate(const int *ident, int j, int id)
{
    bool dup = false;
    for (int i = 0; i < j; i++) dup |= ident[i] == id;
    return dup;
}
// the lowest of C slots whose id is `id`, or -1; id_of(s) reads slot s (no early exit)
template <class IdOf>
__device__ __forceinline__ int slot_lowest(int C, int id, IdOf id_of)
{
    int sl = -1;
    for (int s = C - 1; s >= 0; s--) if (id_of(s) == id) sl = s;
    return sl;
}
// Fresh owners: the r-th flagged box lane takes the r-th flagged (= free) slot lane's slot sidx.  Ranks within a wave pair: waves 0-1 the boxes, waves
// 2-3 the slots.  Returns the slot of a flagged box lane, -1 when there is none left for it (refused), and -2 in every other lane.  wsum: 4 slots,
// freeslot: 128; one barrier inside, and the caller's next one frees both.
__device__ __forceinline__ int block_take_free(bool flag, bool box_lane, int sidx, int *wsum, int *freeslot)
{
    const int r = block_rank(flag, wsum, 2);
    const int nfree = wsum[2] + wsum[3];
    if (flag && !box_lane) freeslot[r] = sidx;
    __syncthreads();
    if (!(flag && box_lane)) return -2;
    return r < nfree ? freeslot[r] : -1;
}
// this wave's count of the flagged lanes for word i of a row of counts (cnt[w]: wave w's)
template <int ROW>
__device__ __forceinline__ void wave_count(int (*cnt)[ROW], int i, bool flag)
{
    const unsigned long long m = __ballot(flag);
    if ((threadIdx.x & (WAVE - 1)) == 0) cnt[threadIdx.x / WAVE][i] = __popcll(m);
}

// ---- reductions in one fixed order: a wave butterfly; the waves' values in LDS, then every lane combines them in wave order (red: one slot per wave;
// free again on return).  The order of the additions is written here and nowhere else; the one arithmetic operation, add_f32, carries the pragma.
template <class T, class Op>
__device__ __forceinline__ T wave_fold(T v, Op op)
{
    for (int o = WAVE / 2; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o));
    return v;
}
template <class T, class Op>
__device__ __forceinline__ T block_fold(T v, T *red, int nw, Op op)
{
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    v = wave_fold(v, op);
    if (lane == 0) red[wave] = v;
    __syncthreads();
    T t = red[0];
    for (int w = 1; w < nw; w++) t = op(t, red[w]);
    __syncthreads();
    return t;
}
__device__ __forceinline__ float add_f32(float a, float b)
{
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float wave_sum(float v) { return wave_fold(v, add_f32); }
__device__ __forceinline__ float wave_max(float v) { return wave_fold(v, fmaxf); }
__device__ __forceinline__ int   wave_max(int v)   { return wave_fold(v, [](int a, int b) { return max(a, b); }); }
__device__ __forceinline__ float block_sum(float v, float *red, int nw) { return block_fold(v, red, nw, add_f32); }
__device__ __forceinline__ float block_max(float v, float *red, int nw) { return block_fold(v, red, nw, fmaxf); }
