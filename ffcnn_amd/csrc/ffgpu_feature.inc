// ffgpu_feature.inc -- the crops classified on the device (ffgpu_features_dev, ffgpu_exec_features, ffgpu_topk_dev, ffgpu_crops_relabel_dev,
// ffgpu_exec_relabel, ffgpu_feature_dim): a CNHW tensor becomes one fp32 row per frame, a row becomes its k best (index, value) pairs, and the best
// pair of each crop slot becomes the class of the first stage's box the crop was cut from.  The contract is in include/ffcnn_hip.h.
//
// No atomic anywhere and every reduction in one fixed order: the same bytes on every run, and a frame's row does not depend on its position in the
// batch or on the batch's size.
//
// Features, launch 1 (k_feat_pool): one WAVE per plane (c, n), a contiguous run of H*W floats.  Lane l owns the quads l, l + 64, ... of the plane and
// takes each quad's elements in ascending order; a quad is one 16-byte load where H*W % 4 == 0 and the plane's address allows it, four 4-byte loads
// otherwise -- the order of the additions is the same either way, so the sum does not depend on the alignment.  The 64 partial results meet in a
// butterfly of cross-lane exchanges (wave_sum, wave_max of ffgpu_block.inc).  MAX compares the values' bits as ordered integers (-0 below +0, exact in any order) and carries "a NaN was seen"
// beside them.  FLAT moves the quads as integers.  Launch 2 (k_feat_post, only with a `post`): one workgroup per row; the row is staged in LDS when it
// has at most FEAT_LDS_ROW floats, else the three passes (maximum, sum, write) read it from the output row itself, which the L2 holds.  A wave reduces by
// cross-lane exchanges, the waves' results meet in LDS and every lane adds them up in wave order (block_sum, block_max).
#define FEAT_LDS_ROW   8192                      // floats of a row staged in LDS (32 KB)
#define FEAT_MAX_PARTS 8                         // == ffgpu_exec::MAXPART
#define FEAT_QNAN      0x7fc00000u

// where frame n of the tensor lies: part[n / pn] is a CNHW tensor of pn frames (one part: pn == N; a split executor: one part per chain)
struct FeatSrc {
    const float *part[FEAT_MAX_PARTS];
    int pn, pad_;
};

__device__ __forceinline__ uint4 feat_quad(const unsigned *pl, int q, int hw, bool vec, unsigned fill)
{
    if (vec) return *reinterpret_cast<const uint4 *>(pl + 4 * (long)q);
    const int i = 4 * q;                                                          // (i < hw: the caller's loop)
    uint4 v;
    v.x = pl[i];
    v.y = i + 1 < hw ? pl[i + 1] : fill;
    v.z = i + 2 < hw ? pl[i + 2] : fill;
    v.w = i + 3 < hw ? pl[i + 3] : fill;
    return v;
}

// the bits of an fp32 value as an integer that orders like the value, with -0 below +0 (its own inverse)
__device__ __forceinline__ int feat_key(unsigned b) { return (int)(b ^ ((unsigned)((int)b >> 31) & 0x7fffffffu)); }

// grid-stride over groups of four planes, 256 lanes = 4 waves; plane p = n * C + c, so a row's outputs are written by neighbouring waves
template <int POOL>
__global__ void __launch_bounds__(256) k_feat_pool(FeatSrc src, int N, int C, int hw, float *out, long out_stride)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (WAVE - 1), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
    const long planes = (long)C * N;
    const int nq = (hw + 3) >> 2;
    for (long p = (long)blockIdx.x * 4 + wave; p < planes; p += (long)gridDim.x * 4) {
        const int n = (int)(p / C), c = (int)(p - (long)n * C);
        const int pi = n / src.pn, ln = n - pi * src.pn;
        const unsigned *pl = reinterpret_cast<const unsigned *>(src.part[pi]) + ((long)c * src.pn + ln) * hw;
        const bool vec = (hw & 3) == 0 && (reinterpret_cast<uintptr_t>(pl) & 15) == 0;
        float *row = out + (long)n * out_stride;
        if (POOL == FFGPU_FEAT_FLAT) {
            unsigned *dst = reinterpret_cast<unsigned *>(row) + (long)c * hw;
            const bool vst = vec && (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
            for (int q = lane; q < nq; q += WAVE) {
                const uint4 v = feat_quad(pl, q, hw, vec, 0u);
                const int i = 4 * q;
                if (vst) { *reinterpret_cast<uint4 *>(dst + i) = v; continue; }
                dst[i] = v.x;
                if (i + 1 < hw) dst[i + 1] = v.y;
                if (i + 2 < hw) dst[i + 2] = v.z;
                if (i + 3 < hw) dst[i + 3] = v.w;
            }
        } else if (POOL == FFGPU_FEAT_MEAN) {
            float acc = 0.f;                                                      // (one chain of additions per lane: nothing to pack)
            for (int q = lane; q < nq; q += WAVE) {
                const uint4 v = feat_quad(pl, q, hw, vec, 0u);                    // (behind the plane's end: + 0)
                acc = acc + __uint_as_float(v.x);
                acc = acc + __uint_as_float(v.y);
                acc = acc + __uint_as_float(v.z);
                acc = acc + __uint_as_float(v.w);
            }
            acc = wave_sum(acc);
            if (lane == 0) row[c] = acc / (float)hw;
        } else {
            int best = (int)0x80000000;                                           // (below every key of a value that is no NaN)
            bool nan = false;
            for (int q = lane; q < nq; q += WAVE) {
                const uint4 v = feat_quad(pl, q, hw, vec, 0xff800000u);           // (behind the plane's end: -Inf)
                const unsigned e[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    nan = nan || (e[k] & 0x7fffffffu) > 0x7f800000u;
                    best = max(best, feat_key(e[k]));
                }
            }
            best = wave_max(best);
            const bool any_nan = __ballot(nan) != 0ull;
            if (lane == 0) reinterpret_cast<unsigned *>(row)[c] = any_nan ? FEAT_QNAN : (unsigned)feat_key((unsigned)best);
        }
    }
}

// grid = rows, 1024 lanes; in place on the output rows
template <int POST>
__global__ void __launch_bounds__(1024) k_feat_post(float *out, long out_stride, int D)
{
#pragma clang fp contract(off)
    __shared__ float s_row[FEAT_LDS_ROW];
    __shared__ float s_red[1024 / WAVE];
    const int tid = threadIdx.x, nt = blockDim.x;
    float *const grow = out + (long)blockIdx.x * out_stride;
    const bool in_lds = D <= FEAT_LDS_ROW;                                         // (uniform)
    if (in_lds) {
        for (int i = tid; i < D; i += nt) s_row[i] = grow[i];
        __syncthreads();
    }
    // a lane reads and rewrites its own elements i = tid, tid + nt, ... only: no pass sees another lane's stores
    auto get = [&](int i) { return in_lds ? s_row[i] : grow[i]; };
    auto put = [&](int i, float v) { if (in_lds) s_row[i] = v; else grow[i] = v; };
    if (POST == FFGPU_POST_SOFTMAX) {
        float m = -INFINITY;
        bool nan = false;
        for (int i = tid; i < D; i += nt) { const float x = get(i); nan = nan || x != x; m = fmaxf(m, x); }
        m = block_max(m, s_red, nt / WAVE);
        const bool bad = __syncthreads_or(nan) || m == INFINITY || m == -INFINITY;
        if (bad) {                                                                 // a NaN, a +Inf, or nothing but -Inf (uniform)
            for (int i = tid; i < D; i += nt) reinterpret_cast<unsigned *>(grow)[i] = FEAT_QNAN;
            return;
        }
        float sum = 0.f;
        for (int i = tid; i < D; i += nt) { const float e = expf(get(i) - m); put(i, e); sum = sum + e; }
        sum = block_sum(sum, s_red, nt / WAVE);
        for (int i = tid; i < D; i += nt) grow[i] = get(i) / sum;
    } else {
        float ss = 0.f;
        for (int i = tid; i < D; i += nt) { const float x = get(i); float sq = x * x; asm volatile("" : "+v"(sq)); ss = ss + sq; }
        const float r = sqrtf(block_sum(ss, s_red, nt / WAVE));
        for (int i = tid; i < D; i += nt) grow[i] = r == 0.f ? 0.f : get(i) / r;
    }
}

// ---- top-k: grid = rows, 256 lanes.  Round r finds the first element, in the contract's total order (value descending, index ascending, no NaN),
// that comes behind round r - 1's (pair_behind, block_first_pair): k <= 16 passes over a row that the L2 holds, no sort, nothing that depends on an arrival order.
__global__ void __launch_bounds__(256) k_topk(const float *in, long in_stride, int D, int k, int2 *out)
{
    __shared__ float s_v[256 / WAVE];
    __shared__ int s_i[256 / WAVE];
    const int tid = threadIdx.x;
    const float *row = in + (long)blockIdx.x * in_stride;
    int2 *o = out + (long)blockIdx.x * k;
    float pv = 0.f;
    int pi = -1;
    int r = 0;
    for (; r < k; r++) {
        float bv = 0.f;
        int bi = -1;
        for (int i = tid; i < D; i += 256) {                                       // (ascending i: of equal values a lane keeps the first)
            const float v = row[i];
            if (v != v) continue;
            if (!pair_behind(v, i, pv, pi, r == 0)) continue;
            if (bi < 0 || v > bv) { bv = v; bi = i; }
        }
        block_first_pair(bv, bi, s_v, s_i, 256 / WAVE);
        if (bi < 0) break;                                                         // (uniform) the row has no further value
        if (tid == 0) o[r] = make_int2(bi, __float_as_int(bv));
        pv = bv; pi = bi;
    }
    for (int j = r + tid; j < k; j += 256) o[j] = make_int2(-1, 0);
}

// ---- relabel: grid = the launch's records, 256 lanes.  The workgroup copies its record and list (unused slots zero), then walks the crop table for
// the entries of its own target; an entry names a box at most once, so no two lanes write one box.
#define RELABEL_ARG_ENTRIES 256
struct RelabelArgs {
    long long first[RELABEL_ARG_ENTRIES];         // record t0 + g: its list's first box in `lists`
    int t0, pad_;
};
__global__ void __launch_bounds__(256) k_relabel(RelabelArgs a, const int *table, int capacity, const int2 *labels, int k, const ffgpu_frame_dets *recs,
                                                 const BBOX *lists, int stride, ffgpu_relabel_spec sp, ffgpu_frame_dets *out_recs, BBOX *out_lists)
{
    const int tid = threadIdx.x;
    const long t = (long)a.t0 + blockIdx.x;
    const ffgpu_frame_dets *rec = recs + t;
    const int nrec = max(0, min(rec->count, FFGPU_MAX_DET)), nlist = lists ? max(0, min(rec->nfull, stride)) : nrec;
    const int *src = reinterpret_cast<const int *>(rec);
    int *dst = reinterpret_cast<int *>(out_recs + t);
    for (int i = tid; i < (int)(sizeof(ffgpu_frame_dets) / sizeof(int)); i += blockDim.x) dst[i] = i < 4 + 6 * nrec ? src[i] : 0;
    if (out_lists) {
        const int *ls = lists ? reinterpret_cast<const int *>(lists + a.first[blockIdx.x]) : src + 4;
        int *ld = reinterpret_cast<int *>(out_lists + t * stride);
        for (long i = tid; i < 6L * stride; i += blockDim.x) ld[i] = i < 6L * nlist ? ls[i] : 0;
    }
    __syncthreads();                                                              // the copies are done (and visible) before a box is patched
    const int taken = max(0, min(table[1], capacity));
    for (int n = tid; n < taken; n += blockDim.x) {
        const int *e = table + 4 + 12 * (long)n;
        if (e[0] != (int)t) continue;
        const int2 lb = labels[(long)n * k];
        const float value = __int_as_float(lb.y);
        if (lb.x < 0 || !(value >= sp.min_value)) continue;
        const int b = e[1], type = (int)((unsigned)sp.type_base + (unsigned)lb.x);
        if (b < 0) continue;
        if (out_lists && b < nlist) {
            BBOX *p = out_lists + t * stride + b;
            p->type = type;
            if (sp.score_mode == FFGPU_RELABEL_LABEL_SCORE) p->score = value;
        }
        if (b < nrec) {
            BBOX *p = out_recs[t].box + b;
            p->type = type;
            if (sp.score_mode == FFGPU_RELABEL_LABEL_SCORE) p->score = value;
        }
    }
}

// ---- host side
extern "C" int ffgpu_feature_dim(int c, int h, int w, int pool)
{
    if (c < 1 || h < 1 || w < 1 || pool < FFGPU_FEAT_FLAT || pool > FFGPU_FEAT_MAX) return 0;
    const long long hw = (long long)h * w, d = pool == FFGPU_FEAT_FLAT ? hw * c : (long long)c;
    if (hw > (1 << 24) || d > (1 << 24)) return 0;
    return (int)d;
}

// what the operator and the executor form check alike; the tensor itself is the caller's business
int ffgpu_feature_args_check(const char *what, int n, int c, int h, int w, int pool, int post, const void *d_out, long out_stride)
{
    if (!d_out) { ffgpu_set_error("%s: NULL output", what); return -1; }
    if (n < 1 || c < 1 || h < 1 || w < 1) { ffgpu_set_error("%s: a tensor of %d frames x %d x %d x %d (every size >= 1)", what, n, c, h, w); return -1; }
    if (pool < FFGPU_FEAT_FLAT || pool > FFGPU_FEAT_MAX) { ffgpu_set_error("%s: pool %d is none of FFGPU_FEAT_FLAT, _MEAN, _MAX", what, pool); return -1; }
    if (post < FFGPU_POST_NONE || post > FFGPU_POST_L2) { ffgpu_set_error("%s: post %d is none of FFGPU_POST_NONE, _SOFTMAX, _L2", what, post); return -1; }
    const int d = ffgpu_feature_dim(c, h, w, pool);
    if (d < 1) { ffgpu_set_error("%s: %d x %d x %d gives a plane or a row of more than 2^24 values", what, c, h, w); return -1; }
    if (out_stride < d) { ffgpu_set_error("%s: out_stride %ld is below the row's %d values", what, out_stride, d); return -1; }
    if (reinterpret_cast<uintptr_t>(d_out) & 3) { ffgpu_set_error("%s: the output must be 4-byte aligned", what); return -1; }
    return 0;
}

// everything has been checked: at most two launches
int ffgpu_launch_features(const float *const *parts, int nparts, int pn, int c, int h, int w, int pool, int post, float *d_out, long out_stride, hipStream_t s)
{
    FeatSrc src;
    memset(&src, 0, sizeof src);
    for (int i = 0; i < nparts; i++) src.part[i] = parts[i];
    src.pn = pn;
    const int N = nparts * pn, hw = h * w, D = ffgpu_feature_dim(c, h, w, pool);
    const unsigned grid = (unsigned)std::min(((long)c * N + 3) / 4, 256L * 64);
    if (pool == FFGPU_FEAT_FLAT)      hipLaunchKernelGGL(k_feat_pool<FFGPU_FEAT_FLAT>, dim3(grid), dim3(256), 0, s, src, N, c, hw, d_out, out_stride);
    else if (pool == FFGPU_FEAT_MEAN) hipLaunchKernelGGL(k_feat_pool<FFGPU_FEAT_MEAN>, dim3(grid), dim3(256), 0, s, src, N, c, hw, d_out, out_stride);
    else                              hipLaunchKernelGGL(k_feat_pool<FFGPU_FEAT_MAX>, dim3(grid), dim3(256), 0, s, src, N, c, hw, d_out, out_stride);
    LAUNCH_OK("features");
    if (post == FFGPU_POST_NONE) return 0;
    if (post == FFGPU_POST_SOFTMAX) hipLaunchKernelGGL(k_feat_post<FFGPU_POST_SOFTMAX>, dim3((unsigned)N), dim3(1024), 0, s, d_out, out_stride, D);
    else                            hipLaunchKernelGGL(k_feat_post<FFGPU_POST_L2>, dim3((unsigned)N), dim3(1024), 0, s, d_out, out_stride, D);
    LAUNCH_OK("features (post)");
    return 0;
}

extern "C" int ffgpu_features_dev(const float *d_in, int n, int c, int h, int w, int pool, int post, float *d_out, long out_stride, void *stream)
{
    const char *const what = "features_dev";
    if (ffgpu_no_device(what)) return -1;
    if (!d_in) { ffgpu_set_error("%s: NULL input", what); return -1; }
    if (ffgpu_feature_args_check(what, n, c, h, w, pool, post, d_out, out_stride)) return -1;
    if (reinterpret_cast<uintptr_t>(d_in) & 3) { ffgpu_set_error("%s: the input must be 4-byte aligned", what); return -1; }
    return ffgpu_launch_features(&d_in, 1, n, c, h, w, pool, post, d_out, out_stride, (hipStream_t)stream);
}

extern "C" int ffgpu_topk_dev(const float *d_in, int n, int d, long in_stride, int k, void *d_out, void *stream)
{
    const char *const what = "topk_dev";
    if (ffgpu_no_device(what)) return -1;
    if (!d_in) { ffgpu_set_error("%s: NULL input", what); return -1; }
    if (!d_out) { ffgpu_set_error("%s: NULL output", what); return -1; }
    if (n < 1 || n > (1 << 24)) { ffgpu_set_error("%s: %d rows (n >= 1)", what, n); return -1; }
    if (d < 1 || d > (1 << 24)) { ffgpu_set_error("%s: rows of %d values (1..2^24)", what, d); return -1; }
    if (in_stride < d) { ffgpu_set_error("%s: in_stride %ld is below the row's %d values", what, in_stride, d); return -1; }
    if (k < 1 || k > FFGPU_TOPK_MAX) { ffgpu_set_error("%s: k %d is outside 1..%d", what, k, FFGPU_TOPK_MAX); return -1; }
    if ((reinterpret_cast<uintptr_t>(d_in) & 3) || (reinterpret_cast<uintptr_t>(d_out) & 3)) { ffgpu_set_error("%s: input and output must be 4-byte aligned", what); return -1; }
    hipLaunchKernelGGL(k_topk, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, d_in, in_stride, d, k, (int2 *)d_out);
    LAUNCH_OK("topk");
    return 0;
}

// what the operator and the executor form check alike, before either looks at its records
int ffgpu_relabel_args_check(const char *what, const void *d_table, int capacity, const void *d_labels, int k, int ntargets, const ffgpu_relabel_spec *spec,
                             const void *d_out_records)
{
    if (!d_table) { ffgpu_set_error("%s: NULL table", what); return -1; }
    if (!d_labels) { ffgpu_set_error("%s: NULL labels", what); return -1; }
    if (!spec) { ffgpu_set_error("%s: NULL spec", what); return -1; }
    if (!d_out_records) { ffgpu_set_error("%s: NULL output records", what); return -1; }
    if (capacity < 1 || capacity > (1 << 24)) { ffgpu_set_error("%s: capacity %d is outside 1..2^24", what, capacity); return -1; }
    if (k < 1 || k > FFGPU_TOPK_MAX) { ffgpu_set_error("%s: k %d is outside 1..%d", what, k, FFGPU_TOPK_MAX); return -1; }
    if (ntargets < 1 || ntargets > (1 << 24)) { ffgpu_set_error("%s: %d targets (ntargets >= 1)", what, ntargets); return -1; }
    if (spec->score_mode != FFGPU_RELABEL_KEEP_SCORE && spec->score_mode != FFGPU_RELABEL_LABEL_SCORE) {
        ffgpu_set_error("%s: score_mode %d is neither FFGPU_RELABEL_KEEP_SCORE nor FFGPU_RELABEL_LABEL_SCORE", what, spec->score_mode);
        return -1;
    }
    if (spec->reserved != 0) { ffgpu_set_error("%s: spec: reserved must be 0", what); return -1; }
    if (reinterpret_cast<uintptr_t>(d_table) & 15) { ffgpu_set_error("%s: the table must be 16-byte aligned", what); return -1; }
    if ((reinterpret_cast<uintptr_t>(d_labels) & 3) || (reinterpret_cast<uintptr_t>(d_out_records) & 3)) { ffgpu_set_error("%s: labels and outputs must be 4-byte aligned", what); return -1; }
    return 0;
}

// everything has been checked
int ffgpu_launch_relabel(const void *d_table, int capacity, const void *d_labels, int k, const DetSource &src, int ntargets, const ffgpu_relabel_spec &spec,
                         void *d_out_records, void *d_out_lists, hipStream_t s)
{
    if ((const void *)src.recs == d_out_records || (src.lists && (const void *)src.lists == d_out_lists)) { ffgpu_set_error("relabel: the outputs must not overlap the inputs"); return -1; }
    for (int t0 = 0; t0 < ntargets; t0 += RELABEL_ARG_ENTRIES) {
        const int nt = std::min(RELABEL_ARG_ENTRIES, ntargets - t0);
        RelabelArgs a;
        memset(&a, 0, sizeof a);
        a.t0 = t0;
        for (int i = 0; i < nt; i++) a.first[i] = src.first[t0 + i];
        hipLaunchKernelGGL(k_relabel, dim3((unsigned)nt), dim3(256), 0, s, a, (const int *)d_table, capacity, (const int2 *)d_labels, k, src.recs, src.lists, src.stride,
                           spec, (ffgpu_frame_dets *)d_out_records, (BBOX *)d_out_lists);
        LAUNCH_OK("crops_relabel");
    }
    return 0;
}

extern "C" int ffgpu_crops_relabel_dev(const void *d_table, int capacity, const void *d_labels, int k, const void *d_records, const void *d_lists,
                                       int list_stride, const int *list_first, int ntargets, const ffgpu_relabel_spec *spec, void *d_out_records,
                                       void *d_out_lists, void *stream)
{
    const char *const what = "crops_relabel_dev";
    if (ffgpu_no_device(what)) return -1;
    if (ffgpu_relabel_args_check(what, d_table, capacity, d_labels, k, ntargets, spec, d_out_records)) return -1;
    DetSource src;
    if (ffgpu_source_dev(what, d_records, d_lists, list_stride, list_first, ntargets, src)) return -1;
    return ffgpu_launch_relabel(d_table, capacity, d_labels, k, src, ntargets, *spec, d_out_records, d_out_lists, (hipStream_t)stream);
}
