// ffgpu_match.inc -- re-identification on the device (ffgpu_match_workspace_bytes, ffgpu_match_dev, ffgpu_gallery_enroll_dev): query rows against a gallery
// of rows that lives in HBM, the k best gallery rows of every query as ffgpu_label, and the queries nobody recognised appended to the gallery.  The
// contract is in include/ffcnn_hip.h.
//
// No atomic anywhere, every sum and every selection in one fixed order: the same bytes on every run, and sim(q, g) is the same bits wherever the two
// rows stand (one accumulator per element, k ascending, the chunking a function of D alone).
//
// Match, launch 1 (k_match): grid = (query blocks of MT_Q, gallery tiles of MT_G), 4 waves.  The workgroup walks D in chunks of MT_KC; a chunk of both
// operands is staged in LDS with its rows K-contiguous (row pitch MT_LD floats: lane (r, k) of an operand read hits bank 36 r + k, 64 different ones),
// the next chunk's global loads in flight while the current one is multiplied.  A quad is one 16-byte load where the base, the stride and D allow it,
// four guarded 4-byte loads otherwise -- the same bits either way; everything behind D, behind nq and behind `count` is zero in LDS.  Wave w owns
// queries 16 w .. 16 w + 15 against all MT_G gallery rows: four accumulator tiles of v_mfma_f32_16x16x4_f32 (A = queries, B = gallery; C/D: gallery
// row = 16 t + (lane & 15), query = 4 (lane >> 4) + reg), so the 64 sims of one query lie in four registers of ONE 16-lane group and the selection
// needs no LDS: round r finds, by four cross-lane exchanges, the first pair (sim, g) in the contract's order behind round r - 1's (pair_behind, pair_take of ffgpu_block.inc, as k_topk).
// The k pairs of (query, tile) go to the workspace.  A tile behind `count` writes its NaNs into d_sim (if given) and ends.
// Launch 2 (k_match_merge): one workgroup per query merges the live tiles' lists in the same order (block_first_pair), k rounds, and applies d_ids.
//
// Enrol, launch 1 (k_enroll_decide): ONE workgroup.  A wave per query decides matched / all finite; then the queries are ranked in ascending r by
// ballots and prefix counts (block_rank), ids and labels written, the head updated.  Launch 2 (k_enroll_copy): one workgroup per query; an enrolled query's slot
// follows from its id and the new head, its row is copied as integers.
#define MT_Q   64                                // queries per workgroup (16 per wave)
#define MT_G   64                                // gallery rows per tile
#define MT_KC  32                                // floats of D per chunk
#define MT_LD  36                                // LDS row pitch in floats
#define MT_QNAN 0x7fc00000u
typedef float v4f_mt __attribute__((ext_vector_type(4)));

struct MatchP {
    const float *q; long q_stride; int nq;
    const float *rows; const int *ids; const int *head; long row_stride; int capacity, d;
    int k, ntiles;
    float *sim; long sim_stride;
    int *work;                                    // [nq][ntiles][k] pairs { g or -1, the bits of sim }
    int *out;                                     // [nq][k] ffgpu_label
};

__device__ __forceinline__ int mt_count(const int *head, int capacity) { return head ? max(0, min(head[0], capacity)) : capacity; }

// quad kq of a row: floats k0 .. k0 + 3 (zero behind D, all zero for a row that is not there)
__device__ __forceinline__ uint4 mt_quad(const unsigned *row, bool there, bool vec, int k0, int D)
{
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (!there || k0 >= D) return v;
    if (vec && k0 + 3 < D) return *reinterpret_cast<const uint4 *>(row + k0);
    v.x = row[k0];
    if (k0 + 1 < D) v.y = row[k0 + 1];
    if (k0 + 2 < D) v.z = row[k0 + 2];
    if (k0 + 3 < D) v.w = row[k0 + 3];
    return v;
}

__global__ void __launch_bounds__(256) k_match(MatchP p)
{
    __shared__ __attribute__((aligned(16))) float s_a[MT_Q * MT_LD];
    __shared__ __attribute__((aligned(16))) float s_b[MT_G * MT_LD];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const int q0 = blockIdx.x * MT_Q, tile = blockIdx.y, g0 = tile * MT_G;
    const int count = mt_count(p.head, p.capacity);
    const int lc = lane & 15, lg = lane >> 4;

    if (g0 >= count) {                                                             // (uniform) nothing there: the matrix's NaNs, no list
        if (p.sim)
            for (int i = tid; i < MT_Q * MT_G; i += 256) {
                const int q = q0 + (i >> 6), g = g0 + (i & 63);
                if (q < p.nq && g < p.capacity) reinterpret_cast<unsigned *>(p.sim)[(long)q * p.sim_stride + g] = MT_QNAN;
            }
        return;
    }

    // staging: thread -> rows (tid >> 3) and (tid >> 3) + 32 of each operand, quad tid & 7 of the chunk
    const int sr = tid >> 3, sk = (tid & 7) * 4;
    const unsigned *qrow[2], *grow[2];
    bool qin[2], gin[2];
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int q = q0 + sr + 32 * j, g = g0 + sr + 32 * j;
        qin[j] = q < p.nq;
        gin[j] = g < count;
        qrow[j] = reinterpret_cast<const unsigned *>(p.q) + (long)(qin[j] ? q : 0) * p.q_stride;
        grow[j] = reinterpret_cast<const unsigned *>(p.rows) + (long)(gin[j] ? g : 0) * p.row_stride;
    }
    const bool qvec = (reinterpret_cast<uintptr_t>(p.q) & 15) == 0 && (p.q_stride & 3) == 0;       // (uniform)
    const bool gvec = (reinterpret_cast<uintptr_t>(p.rows) & 15) == 0 && (p.row_stride & 3) == 0;
    uint4 ra[2], rb[2];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int j = 0; j < 2; j++) {
            ra[j] = mt_quad(qrow[j], qin[j], qvec, k0 + sk, p.d);
            rb[j] = mt_quad(grow[j], gin[j], gvec, k0 + sk, p.d);
        }
    };

    v4f_mt acc[4];
#pragma unroll
    for (int t = 0; t < 4; t++) acc[t] = (v4f_mt){ 0.f, 0.f, 0.f, 0.f };
    const float *A = s_a + (16 * wave + lc) * MT_LD + lg;                          // + 4 s: query 16 wave + lc, k = 4 s + lg
    const float *B = s_b + lc * MT_LD + lg;                                        // + 16 t MT_LD + 4 s: gallery row 16 t + lc
    fetch(0);
    for (int k0 = 0; k0 < p.d; k0 += MT_KC) {
        __syncthreads();                                                           // the previous chunk has been read
#pragma unroll
        for (int j = 0; j < 2; j++) {
            *reinterpret_cast<uint4 *>(s_a + (sr + 32 * j) * MT_LD + sk) = ra[j];
            *reinterpret_cast<uint4 *>(s_b + (sr + 32 * j) * MT_LD + sk) = rb[j];
        }
        __syncthreads();
        if (k0 + MT_KC < p.d) fetch(k0 + MT_KC);
#pragma unroll
        for (int s = 0; s < MT_KC / 4; s++) {
            const float a = A[4 * s];
#pragma unroll
            for (int t = 0; t < 4; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, B[16 * t * MT_LD + 4 * s], acc[t], 0, 0, 0);
        }
    }

    // rows that are not there or are disabled: the quiet NaN
    int gi[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
        gi[t] = g0 + 16 * t + lc;
        const bool off = gi[t] >= count || (p.ids && p.ids[gi[t]] < 0);
        if (off)
#pragma unroll
            for (int e = 0; e < 4; e++) acc[t][e] = __uint_as_float(MT_QNAN);
    }
    const int qb = q0 + 16 * wave + 4 * lg;                                        // this lane's queries: qb + e
    if (p.sim)
#pragma unroll
        for (int e = 0; e < 4; e++)
#pragma unroll
            for (int t = 0; t < 4; t++)
                if (qb + e < p.nq && gi[t] < p.capacity) p.sim[(long)(qb + e) * p.sim_stride + gi[t]] = acc[t][e];

    // the k best pairs of each query, in order; the four queries of a lane group run side by side
    float pv[4] = { 0.f, 0.f, 0.f, 0.f };
    int pg[4] = { -1, -1, -1, -1 };
    for (int r = 0; r < p.k; r++) {
#pragma unroll
        for (int e = 0; e < 4; e++) {
            float bv = 0.f;
            int bg = -1;
#pragma unroll
            for (int t = 0; t < 4; t++) {                                           // (ascending g: of equal values a lane keeps the first)
                const float v = acc[t][e];
                const bool ok = v == v && pair_behind(v, gi[t], pv[e], pg[e], r == 0);
                if (ok && (bg < 0 || v > bv)) { bv = v; bg = gi[t]; }
            }
            if (r > 0 && pg[e] < 0) bg = -1;                                       // the list ended in an earlier round
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) { const float ov = __shfl_xor(bv, o); const int og = __shfl_xor(bg, o); pair_take(bv, bg, ov, og); }
            pv[e] = bv; pg[e] = bg;
            if (lc == 0 && qb + e < p.nq) {
                int *w = p.work + (((long)(qb + e) * p.ntiles + tile) * p.k + r) * 2;
                w[0] = bg;
                w[1] = bg < 0 ? 0 : __float_as_int(bv);
            }
        }
    }
}

// grid = queries, 256 lanes: k rounds over the live tiles' pairs
__global__ void __launch_bounds__(256) k_match_merge(MatchP p)
{
    __shared__ float s_v[256 / WAVE];
    __shared__ int s_g[256 / WAVE];
    const int tid = threadIdx.x;
    const int q = blockIdx.x;
    const int count = mt_count(p.head, p.capacity);
    const int n = ((count + MT_G - 1) / MT_G) * p.k;                                // pairs of the tiles that wrote a list
    const int *w = p.work + (long)q * p.ntiles * p.k * 2;
    int *o = p.out + (long)q * p.k * 2;
    float pv = 0.f;
    int pg = -1;
    int r = 0;
    for (; r < p.k; r++) {
        float bv = 0.f;
        int bg = -1;
        for (int i = tid; i < n; i += 256) {
            const int g = w[2 * i];
            const float v = __int_as_float(w[2 * i + 1]);
            if (g < 0) continue;
            if (!pair_behind(v, g, pv, pg, r == 0)) continue;
            pair_take(bv, bg, v, g);
        }
        block_first_pair(bv, bg, s_v, s_g, 256 / WAVE);
        if (bg < 0) break;                                                         // (uniform) no further pair
        if (tid == 0) { o[2 * r] = p.ids ? p.ids[bg] : bg; o[2 * r + 1] = __float_as_int(bv); }
        pv = bv; pg = bg;
    }
    for (int j = r + tid; j < p.k; j += 256) { o[2 * j] = -1; o[2 * j + 1] = 0; }
}

// ---- enrol
#define EN_MATCHED 0
#define EN_NEW     1
#define EN_DROP    2
struct EnrollP {
    const float *q; long q_stride; int nq;
    float *rows; int *ids; int *head; long row_stride; int capacity, d;
    const int *labels; int k; float min_value;
    int *out;
};

// one workgroup of 1024 lanes
__global__ void __launch_bounds__(1024) k_enroll_decide(EnrollP p)
{
    __shared__ unsigned char s_state[4096];
    __shared__ int s_cnt[1024 / WAVE];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int count = max(0, min(p.head[0], p.capacity)), issued = p.head[1], dropped = p.head[2];
    for (int r = wave; r < p.nq; r += 1024 / WAVE) {                                // a wave per query
        const int idx = p.labels[2 * (long)r * p.k];
        const float val = __int_as_float(p.labels[2 * (long)r * p.k + 1]);
        int st = EN_MATCHED;
        if (!(idx >= 0 && val >= p.min_value)) {
            const unsigned *row = reinterpret_cast<const unsigned *>(p.q) + (long)r * p.q_stride;
            bool bad = false;
            for (int i = lane; i < p.d; i += WAVE) bad = bad || (row[i] & 0x7f800000u) == 0x7f800000u;
            st = __ballot(bad) != 0ull ? EN_DROP : EN_NEW;
        }
        if (lane == 0) s_state[r] = (unsigned char)st;
    }
    __syncthreads();
    int seen = 0, ndrop = 0;                                                       // (uniform) new rows / dropped rows in front of this pass
    for (int r0 = 0; r0 < p.nq; r0 += 1024) {
        const int r = r0 + tid;
        const int st = r < p.nq ? s_state[r] : EN_MATCHED;
        int total;
        const int e = seen + block_rank(st == EN_NEW, s_cnt, 1024 / WAVE, total);   // this query's rank among the new ones
        const bool room = e < p.capacity - count;
        if (r < p.nq) {
            int2 o = make_int2(-1, 0);
            if (st == EN_MATCHED) o = make_int2(p.labels[2 * (long)r * p.k], p.labels[2 * (long)r * p.k + 1]);
            else if (st == EN_NEW && room) {
                o = make_int2(issued + e + 1, __float_as_int(p.min_value));
                p.ids[count + e] = o.x;
            }
            p.out[2 * r] = o.x;
            p.out[2 * r + 1] = o.y;
        }
        ndrop += __syncthreads_count(r < p.nq && (st == EN_DROP || (st == EN_NEW && !room)));
        seen += total;
    }
    if (tid == 0) {
        const int enrolled = min(seen, p.capacity - count);
        p.head[0] = count + enrolled;
        p.head[1] = issued + enrolled;
        p.head[2] = dropped + ndrop;
    }
}

// grid = queries, 256 lanes.  Query r was enrolled iff it was not matched and its label is no { -1, 0 }; its id is issued' - (enrolled - 1 - e) and
// its slot count' - (enrolled - e), so slot = count' - 1 - (issued' - id) with the head as launch 1 left it.
__global__ void __launch_bounds__(256) k_enroll_copy(EnrollP p)
{
    const int r = blockIdx.x;
    const int idx = p.labels[2 * (long)r * p.k];
    const float val = __int_as_float(p.labels[2 * (long)r * p.k + 1]);
    if (idx >= 0 && val >= p.min_value) return;
    const int id = p.out[2 * r];
    if (id < 0) return;
    const int slot = p.head[0] - 1 - (p.head[1] - id);
    if (slot < 0 || slot >= p.capacity) return;                                    // (cannot happen; a store is never made on trust)
    const unsigned *src = reinterpret_cast<const unsigned *>(p.q) + (long)r * p.q_stride;
    unsigned *dst = reinterpret_cast<unsigned *>(p.rows) + (long)slot * p.row_stride;
    for (int i = threadIdx.x; i < p.d; i += 256) dst[i] = src[i];
}

// ---- host side
#define MT_MAX_NQ  4096
#define MT_MAX_CAP (1 << 20)
#define MT_MAX_D   4096

extern "C" size_t ffgpu_match_workspace_bytes(int nq, int capacity, int k)
{
    if (nq < 1 || nq > MT_MAX_NQ || capacity < 1 || capacity > MT_MAX_CAP || k < 1 || k > FFGPU_TOPK_MAX) return 0;
    return (size_t)nq * (size_t)((capacity + MT_G - 1) / MT_G) * (size_t)k * 8;
}

// what match and enrol check alike
static int ffgpu_gallery_check(const char *what, const ffgpu_gallery *g, bool need_ids_head)
{
    if (!g) { ffgpu_set_error("%s: NULL gallery", what); return -1; }
    if (!g->d_rows) { ffgpu_set_error("%s: NULL gallery rows (d_rows)", what); return -1; }
    if (need_ids_head && !g->d_ids) { ffgpu_set_error("%s: NULL d_ids (enrolment issues ids)", what); return -1; }
    if (need_ids_head && !g->d_head) { ffgpu_set_error("%s: NULL d_head (enrolment counts on the device)", what); return -1; }
    if (g->capacity < 1 || g->capacity > MT_MAX_CAP) { ffgpu_set_error("%s: capacity %d is outside 1..2^20", what, g->capacity); return -1; }
    if (g->d < 1 || g->d > MT_MAX_D) { ffgpu_set_error("%s: rows of %d values (1..%d)", what, g->d, MT_MAX_D); return -1; }
    if (g->row_stride < g->d) { ffgpu_set_error("%s: row_stride %ld is below the row's %d values", what, g->row_stride, g->d); return -1; }
    if ((reinterpret_cast<uintptr_t>(g->d_rows) & 3) || (reinterpret_cast<uintptr_t>(g->d_ids) & 3)) { ffgpu_set_error("%s: d_rows and d_ids must be 4-byte aligned", what); return -1; }
    if (reinterpret_cast<uintptr_t>(g->d_head) & 15) { ffgpu_set_error("%s: d_head must be 16-byte aligned", what); return -1; }
    return 0;
}

extern "C" int ffgpu_match_dev(const float *d_q, int nq, long q_stride, const ffgpu_gallery *g, int k, void *d_out_labels, float *d_sim, long sim_stride,
                               void *d_work, size_t work_bytes, void *stream)
{
    const char *const what = "match_dev";
    if (ffgpu_no_device(what)) return -1;
    if (!d_q) { ffgpu_set_error("%s: NULL queries", what); return -1; }
    if (ffgpu_gallery_check(what, g, false)) return -1;
    if (!d_out_labels) { ffgpu_set_error("%s: NULL labels", what); return -1; }
    if (!d_work) { ffgpu_set_error("%s: NULL workspace", what); return -1; }
    if (nq < 1 || nq > MT_MAX_NQ) { ffgpu_set_error("%s: %d queries (1..%d)", what, nq, MT_MAX_NQ); return -1; }
    if (k < 1 || k > FFGPU_TOPK_MAX) { ffgpu_set_error("%s: k %d is outside 1..%d", what, k, FFGPU_TOPK_MAX); return -1; }
    if (q_stride < g->d) { ffgpu_set_error("%s: q_stride %ld is below the row's %d values", what, q_stride, g->d); return -1; }
    if (d_sim && sim_stride < g->capacity) { ffgpu_set_error("%s: sim_stride %ld is below the capacity %d", what, sim_stride, g->capacity); return -1; }
    const size_t need = ffgpu_match_workspace_bytes(nq, g->capacity, k);
    if (work_bytes < need) { ffgpu_set_error("%s: a workspace of %zu bytes is below the %zu of ffgpu_match_workspace_bytes", what, work_bytes, need); return -1; }
    if ((reinterpret_cast<uintptr_t>(d_q) & 3) || (reinterpret_cast<uintptr_t>(d_out_labels) & 3) || (reinterpret_cast<uintptr_t>(d_sim) & 3) ||
        (reinterpret_cast<uintptr_t>(d_work) & 3)) {
        ffgpu_set_error("%s: queries, labels, matrix and workspace must be 4-byte aligned", what);
        return -1;
    }
    MatchP p;
    memset(&p, 0, sizeof p);
    p.q = d_q; p.q_stride = q_stride; p.nq = nq;
    p.rows = g->d_rows; p.ids = g->d_ids; p.head = g->d_head; p.row_stride = g->row_stride; p.capacity = g->capacity; p.d = g->d;
    p.k = k; p.ntiles = (g->capacity + MT_G - 1) / MT_G;
    p.sim = d_sim; p.sim_stride = sim_stride;
    p.work = (int *)d_work; p.out = (int *)d_out_labels;
    hipLaunchKernelGGL(k_match, dim3((unsigned)((nq + MT_Q - 1) / MT_Q), (unsigned)p.ntiles), dim3(256), 0, (hipStream_t)stream, p);
    LAUNCH_OK("match");
    hipLaunchKernelGGL(k_match_merge, dim3((unsigned)nq), dim3(256), 0, (hipStream_t)stream, p);
    LAUNCH_OK("match (merge)");
    return 0;
}

extern "C" int ffgpu_gallery_enroll_dev(const ffgpu_gallery *g, const float *d_q, int nq, long q_stride, const void *d_labels, int k, float min_value,
                                        void *d_out_labels, void *stream)
{
    const char *const what = "gallery_enroll_dev";
    if (ffgpu_no_device(what)) return -1;
    if (ffgpu_gallery_check(what, g, true)) return -1;
    if (!d_q) { ffgpu_set_error("%s: NULL queries", what); return -1; }
    if (!d_labels) { ffgpu_set_error("%s: NULL labels", what); return -1; }
    if (!d_out_labels) { ffgpu_set_error("%s: NULL output labels", what); return -1; }
    if (nq < 1 || nq > MT_MAX_NQ) { ffgpu_set_error("%s: %d queries (1..%d)", what, nq, MT_MAX_NQ); return -1; }
    if (k < 1 || k > FFGPU_TOPK_MAX) { ffgpu_set_error("%s: k %d is outside 1..%d", what, k, FFGPU_TOPK_MAX); return -1; }
    if (q_stride < g->d) { ffgpu_set_error("%s: q_stride %ld is below the row's %d values", what, q_stride, g->d); return -1; }
    if ((reinterpret_cast<uintptr_t>(d_q) & 3) || (reinterpret_cast<uintptr_t>(d_labels) & 3) || (reinterpret_cast<uintptr_t>(d_out_labels) & 3)) {
        ffgpu_set_error("%s: queries and labels must be 4-byte aligned", what);
        return -1;
    }
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(d_labels), a1 = a0 + 8 * (size_t)nq * k, b0 = reinterpret_cast<uintptr_t>(d_out_labels), b1 = b0 + 8 * (size_t)nq;
    if (a0 < b1 && b0 < a1) { ffgpu_set_error("%s: the output labels must not overlap the labels", what); return -1; }
    EnrollP p;
    memset(&p, 0, sizeof p);
    p.q = d_q; p.q_stride = q_stride; p.nq = nq;
    p.rows = g->d_rows; p.ids = g->d_ids; p.head = g->d_head; p.row_stride = g->row_stride; p.capacity = g->capacity; p.d = g->d;
    p.labels = (const int *)d_labels; p.k = k; p.min_value = min_value;
    p.out = (int *)d_out_labels;
    hipLaunchKernelGGL(k_enroll_decide, dim3(1), dim3(1024), 0, (hipStream_t)stream, p);
    LAUNCH_OK("gallery_enroll");
    hipLaunchKernelGGL(k_enroll_copy, dim3((unsigned)nq), dim3(256), 0, (hipStream_t)stream, p);
    LAUNCH_OK("gallery_enroll (copy)");
    return 0;
}
