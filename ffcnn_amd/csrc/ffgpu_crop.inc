// ffgpu_crop.inc -- the detections cut out of the frames on the device for a second stage (ffgpu_crop_boxes_bgr_dev / _nv12_dev, ffgpu_exec_crop_bgr /
// _nv12, ffgpu_crops_to_source_dev): select the boxes, resample each one's region of its source frame into a slot of the caller's batch buffer as
// net_input (ffcnn.c:259-289) would if the region were an image of its own, and move a second forward's boxes back into the source's coordinates.
// The contract is in include/ffcnn_hip.h.
//
// Order without atomics: k_crop_select is ONE workgroup per launch.  16 lanes walk each target's list, a ballot gives every box its ordinal among
// its target's selected boxes, a scan over the launch's targets gives each target its first slot, and the number of boxes selected so far travels
// from one launch to the next in the table's header, in stream order.  The table is the same byte for byte however the targets are split.
//
// The source table, the class filter and the spec travel as ONE by-value kernel argument (CROP_ARG_TARGETS targets per launch; more targets: more
// launches): nothing is copied from pageable host memory on the stream.
#define CROP_ARG_TARGETS 64
#define CROP_GROUP       16       // lanes per target in k_crop_select (CROP_ARG_TARGETS x CROP_GROUP = the workgroup)
#define CROP_MAX_GRID_Y  65535
struct CropSelArgs {
    CropSrc       t[CROP_ARG_TARGETS];
    unsigned char classes[256];
    int   nt, rec0, first, last;      // targets of this launch, record of target 0, the call's first / last launch
    int   out_w, out_h, per_target, nclasses, num, den;
    float min_score;
    int   pad_;
};
struct CropPixArgs {
    CropSrc t[CROP_ARG_TARGETS];
    int     t0, nt, slot0, tail;      // this launch holds targets t0 .. t0 + nt - 1; block y is slot slot0 + y; tail: it also zeroes the slots >= taken
    int     W, H;
    InputP  p;
};
static_assert(sizeof(CropSrc) == 48 && sizeof(CropSelArgs) + 5 * 8 <= 4096 - 256 && sizeof(CropPixArgs) + 3 * 8 <= 4096 - 256,
              "the tables travel as a kernel argument (4 KB at most, the hidden arguments included)");
static_assert(sizeof(ffgpu_crop) == 48 && sizeof(ffgpu_crop_spec) == 72, "include/ffcnn_hip.h states these sizes");

// One box against the spec and its source's w x h: 0 = does not qualify, 1 = qualifies and is empty, 2 = qualifies, r = { X0, Y0, w, h }.
// Corners as the draw contract (draw_f2i), everything behind them in 64-bit integers: (c - a + 1) num <= 2^32 x 4096.  Sel: a kernel's argument struct
// with the selection's fields min_score, nclasses, classes, num, den (CropSelArgs; RedactArgs of ffgpu_redact.inc).
template <class Sel>
__device__ __forceinline__ int crop_region(const BBOX &b, const Sel &a, int w, int h, int4 &r)
{
    if (!(b.score >= a.min_score)) return 0;                                          // (a NaN score never qualifies)
    if (a.nclasses && !((unsigned)b.type < (unsigned)a.nclasses && a.classes[(unsigned)b.type & 255u])) return 0;
    const long long A = draw_f2i(b.x1), B = draw_f2i(b.y1), C = draw_f2i(b.x2), D = draw_f2i(b.y2);
    if (A > C || B > D) return 1;
    const long long mx = (C - A + 1) * a.num / a.den, my = (D - B + 1) * a.num / a.den;
    const long long X0 = max(A - mx, 0LL), X1 = min(C + mx, (long long)w - 1), Y0 = max(B - my, 0LL), Y1 = min(D + my, (long long)h - 1);
    if (X0 > X1 || Y0 > Y1) return 1;
    r.x = (int)X0; r.y = (int)Y0; r.z = (int)(X1 - X0 + 1); r.w = (int)(Y1 - Y0 + 1);
    return 2;
}

// grid 1, CROP_ARG_TARGETS x CROP_GROUP lanes: lane group g owns target g of the launch.  Counts are clamped to [0, stride] as the draw kernel clamps
// them.  Pass 0 counts each target's selected (at most per_target) and empty boxes, pass 1 walks the lists again and writes the entries whose slot
// lies below the capacity; the last launch of a call fills entries taken .. capacity - 1 with the "no crop" pattern.  table: { total, taken, empty,
// capacity } then capacity x ffgpu_crop, 16-byte aligned.
__global__ void __launch_bounds__(CROP_ARG_TARGETS * CROP_GROUP) k_crop_select(CropSelArgs a, const ffgpu_frame_dets *recs, const BBOX *lists, int stride,
                                                                            int *table, int capacity)
{
    __shared__ int s_sel[CROP_ARG_TARGETS], s_emp[CROP_ARG_TARGETS], s_base[CROP_ARG_TARGETS], s_sum[2];
    const int tid = threadIdx.x, g = tid / CROP_GROUP, l = tid % CROP_GROUP, shift = tid & (WAVE - 1) & ~(CROP_GROUP - 1);
    const int total0 = a.first ? 0 : table[0], empty0 = a.first ? 0 : table[2];
    const bool on = g < a.nt && a.t[g].p0 != nullptr;                                  // (false: a skipped target, or none)
    const ffgpu_frame_dets *rec = recs + a.rec0 + g;
    const int n = on ? max(0, min(lists ? rec->nfull : rec->count, stride)) : 0;
    const BBOX *list = on ? (lists ? lists + a.t[g].first : rec->box) : nullptr;
    const int w = on ? a.t[g].w : 1, h = on ? a.t[g].h : 1;
    for (int pass = 0; pass < 2; pass++) {
        int sel = 0, emp = 0;
        const int base = pass ? total0 + s_base[g] : 0;
        for (int k0 = 0; k0 < n; k0 += CROP_GROUP) {                                   // (n is the same in all lanes of a group)
            const int k = k0 + l;
            int4 r = { 0, 0, 0, 0 };
            BBOX b = { 0, 0.f, 0.f, 0.f, 0.f, 0.f };
            int state = 0;
            if (k < n) { b = list[k]; state = crop_region(b, a, w, h, r); }
            const unsigned ms = (unsigned)(__ballot(state == 2) >> shift) & 0xffffu, me = (unsigned)(__ballot(state == 1) >> shift) & 0xffffu;
            const int ord = sel + __popc(ms & ((1u << l) - 1u));
            if (pass && state == 2 && ord < a.per_target && base + ord < capacity) {
                int sw, sh, s1, s2;                                                    // net_input's letterbox of r.z x r.w into out_w x out_h (ffcnn.c:267-273)
                if ((long long)r.z * a.out_h > (long long)r.w * a.out_w) { sw = a.out_w; sh = (int)((long long)sw * r.w / r.z); s1 = r.z; s2 = sw; }
                else                                                     { sh = a.out_h; sw = (int)((long long)sh * r.z / r.w); s1 = r.w; s2 = sh; }
                int4 *e = reinterpret_cast<int4 *>(table + 4 + 12 * (long)(base + ord));
                e[0] = make_int4(a.rec0 + g, k, b.type, __float_as_int(b.score));
                e[1] = r;
                e[2] = make_int4(sw, sh, s1, s2);
            }
            sel += __popc(ms); emp += __popc(me);
        }
        if (pass) break;
        if (l == 0) { s_sel[g] = min(sel, a.per_target); s_emp[g] = emp; }
        __syncthreads();
        if (tid < WAVE) {                                                              // (CROP_ARG_TARGETS == WAVE: one wave scans the launch's targets)
            const int v = s_sel[tid];
            int inc = v, es = s_emp[tid];
            for (int d = 1; d < WAVE; d <<= 1) {
                const int up = __shfl_up(inc, d), ue = __shfl_up(es, d);
                if (tid >= d) { inc += up; es += ue; }
            }
            s_base[tid] = inc - v;
            if (tid == WAVE - 1) { s_sum[0] = inc; s_sum[1] = es; }
        }
        __syncthreads();
    }
    const int total = total0 + s_sum[0], taken = min(total, capacity);
    if (a.last)
        for (long i = taken + tid; i < capacity; i += blockDim.x) {
            int4 *e = reinterpret_cast<int4 *>(table + 4 + 12 * i);
            e[0] = make_int4(-1, 0, 0, 0); e[1] = make_int4(0, 0, 0, 0); e[2] = make_int4(0, 0, 1, 1);
        }
    if (tid == 0) *reinterpret_cast<int4 *>(table) = make_int4(total, taken, empty0 + s_sum[1], capacity);
}
static_assert(CROP_ARG_TARGETS == WAVE && WAVE % CROP_GROUP == 0, "k_crop_select: one wave scans the targets, a group lies inside one wave");

// NV12: the four source pixels of output pixels x0 .. x0 + 3 of row y of a region with origin (ox, oy), converted at the PICTURE's coordinates: the
// chroma pair of source pixel (xs, ys) is UV[ys >> 1][xs >> 1] whatever the origin's parity.  Not resized and Y rows dword aligned: the four Y
// bytes as one dword.  (BGR regions go through BgrPixels::load4 with a shifted base.)
__device__ __forceinline__ void crop_load4_nv12(const CropSrc &s, int ox, int oy, int sw, int s1, int s2, int x0, int y, unsigned px[4])
{
    const YuvMat m = yuv_mat(s.fmt);
    const long ys = oy + (long)y * s1 / s2;
    const unsigned char *yrow = s.p0 + ys * s.pitch, *crow = s.p1 + (ys >> 1) * s.pitch_uv;
    if (s1 == s2 && x0 + 3 < sw && ((reinterpret_cast<uintptr_t>(s.p0 + ox) | (unsigned)s.pitch) & 3) == 0) {
        const long xb = (long)ox + x0;
        const unsigned yy = *reinterpret_cast<const unsigned *>(yrow + xb);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const unsigned pr = *reinterpret_cast<const unsigned short *>(crow + ((xb + i) & ~1L));
            px[i] = nv12_to_bgr((int)((yy >> (8 * i)) & 0xffu), (int)(pr & 0xffu), (int)(pr >> 8), m);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int x = min(x0 + i, sw - 1);
            const long xs = ox + (long)x * s1 / s2;
            const unsigned pr = *reinterpret_cast<const unsigned short *>(crow + (xs & ~1L));
            px[i] = nv12_to_bgr((int)yrow[xs], (int)(pr & 0xffu), (int)(pr >> 8), m);
        }
    }
}

// k_input4's shape: a thread owns 4 consecutive output pixels of one row of slot slot0 + blockIdx.y and reads that slot's entry once.  Slots below
// `taken` whose target this launch holds are resampled, the slots from `taken` on are zeroed by the launch with a.tail set, every other block leaves.
// F32: planes R G B of H x W fp32, (byte - mean) * norm with two roundings (front_cvt), one 16-byte store per plane where W % 4 == 0.  U8: rows of ALIGN(3 W, 4) bytes B G R, three dwords per
// lane (fewer where the row ends), padding bytes zero.
template <bool NV12, bool U8>
__global__ void __launch_bounds__(256) k_crop_pixels(CropPixArgs a, const int *table, void *out, int capacity)
{
    typedef float f4 __attribute__((ext_vector_type(4)));
    const int W = a.W, H = a.H;
    const unsigned wq = ((unsigned)W + 3) >> 2, t = blockIdx.x * 256 + threadIdx.x;
    if (t >= wq * (unsigned)H) return;
    const int y = (int)(t / wq), x0 = (int)(t - (unsigned)y * wq) * 4;
    const long n = (long)a.slot0 + blockIdx.y;                                       // (< capacity: the host sizes the grid)
    const int taken = min(max(table[1], 0), capacity);
    unsigned px[4] = { 0, 0, 0, 0 };
    int lim = 0;                                                                      // pixels x < lim of this row come from the source
    if (n < taken) {
        const int4 *e = reinterpret_cast<const int4 *>(table + 4 + 12 * n);
        const int4 e0 = e[0], e1 = e[1], e2 = e[2];                                   // target box type score | x0 y0 w h | sw sh s1 s2
        const int ti = __builtin_amdgcn_readfirstlane(e0.x) - a.t0;
        if ((unsigned)ti >= (unsigned)a.nt) return;                                   // another launch's target (uniform)
        const CropSrc &s = a.t[ti];
        if (s.p0 && y < e2.y && x0 < e2.x) {
            lim = e2.x;
            if (NV12) crop_load4_nv12(s, e1.x, e1.y, e2.x, e2.z, e2.w, x0, y, px);
            else {
                FrameDesc fd;
                fd.bgr = s.p0 + (long)e1.y * s.pitch + 3L * e1.x; fd.w = e1.z; fd.h = e1.w; fd.pitch = s.pitch;
                fd.sw = e2.x; fd.sh = e2.y; fd.s1 = e2.z; fd.s2 = e2.w; fd.fmt = 0; fd.uv = nullptr; fd.pitch_uv = 0; fd.pad_ = 0;
                BgrPixels::load4(fd, x0, y, px);
            }
        }
    } else if (!a.tail) return;
#pragma unroll
    for (int i = 0; i < 4; i++) if (x0 + i >= lim) px[i] = 0;
    if (U8) {
        const long P = (3L * W + 3) & ~3L;
        unsigned *o = reinterpret_cast<unsigned *>(static_cast<unsigned char *>(out) + (n * H + y) * P + 3L * x0);
        const int nd = (3 * min(4, W - x0) + 3) >> 2;                                 // dwords to the end of the row's padding: 1, 2 or 3
        o[0] = px[0] | (px[1] << 24);
        if (nd > 1) o[1] = (px[1] >> 8) | (px[2] << 16);
        if (nd > 2) o[2] = (px[2] >> 16) | (px[3] << 8);
    } else {
        f4 r, g, b;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const bool in = x0 + i < lim;
            r[i] = in ? front_cvt((px[i] >> 16) & 0xffu, a.p.mean[0], a.p.norm[0]) : 0.f;       // (front_cvt: never paired into packed fp32, tools/isa_lint.py)
            g[i] = in ? front_cvt((px[i] >> 8) & 0xffu, a.p.mean[1], a.p.norm[1]) : 0.f;
            b[i] = in ? front_cvt(px[i] & 0xffu, a.p.mean[2], a.p.norm[2]) : 0.f;
        }
        float *o = static_cast<float *>(out) + n * 3 * H * W + (long)y * W + x0;
        if ((W & 3) == 0) {
            *reinterpret_cast<f4 *>(o) = r;
            *reinterpret_cast<f4 *>(o + (long)H * W) = g;
            *reinterpret_cast<f4 *>(o + 2L * H * W) = b;
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (x0 + i < W) { o[i] = r[i]; o[i + (long)H * W] = g[i]; o[i + 2L * H * W] = b[i]; }
        }
    }
}

// one box: type and score copied, every coordinate v * s1 / s2 + origin -- k_nms's rescale (multiply, divide) then the merge's translation (add), fp32,
// not contracted.  One coordinate per trip of a loop that stays a loop: the four are never paired into packed fp32 instructions (tools/isa_lint.py).
__device__ __forceinline__ void crop_move(const BBOX *in, BBOX *out, float fs1, float fs2, float fx, float fy)
{
#pragma clang fp contract(off)
    const int type = in->type;
    const float score = in->score;
    out->type = type; out->score = score;
    const float *s = &in->x1;
    float *d = &out->x1;
#pragma clang loop unroll(disable)
    for (int i = 0; i < 4; i++) d[i] = s[i] * fs1 / fs2 + ((i & 1) ? fy : fx);
}

// grid capacity, 128 lanes: record n of a forward over the slots back into its source's coordinates.  Slots from `taken` on give zero records.  In
// place is legal: a lane reads what it writes, and every lane has the counters before lane 0 writes them.
__global__ void __launch_bounds__(FFGPU_MAX_DET) k_crops_to_source(const int *table, int capacity, const ffgpu_frame_dets *recs, const BBOX *lists, int stride,
                                                                  ffgpu_frame_dets *out_recs, BBOX *out_lists)
{
    const int n = blockIdx.x, tid = threadIdx.x;
    const bool live = n < min(max(table[1], 0), capacity);
    const int4 e1 = *reinterpret_cast<const int4 *>(table + 4 + 12 * (long)n + 4), e2 = *reinterpret_cast<const int4 *>(table + 4 + 12 * (long)n + 8);
    const float fs1 = (float)e2.z, fs2 = (float)e2.w, fx = (float)e1.x, fy = (float)e1.y;
    const ffgpu_frame_dets *rec = recs + n;
    const int count = rec->count, ncand = rec->ncand, overflow = rec->overflow, nfull = rec->nfull;
    const int nb = live ? max(0, min(count, FFGPU_MAX_DET)) : 0, nl = live && lists && out_lists ? max(0, min(nfull, stride)) : 0;
    __syncthreads();                                                                  // every lane has read the counters
    if (tid < nb) crop_move(rec->box + tid, out_recs[n].box + tid, fs1, fs2, fx, fy);
    else out_recs[n].box[tid] = BBOX{ 0, 0.f, 0.f, 0.f, 0.f, 0.f };
    if (tid == 0) {
        out_recs[n].count = live ? count : 0; out_recs[n].ncand = live ? ncand : 0;
        out_recs[n].overflow = live ? overflow : 0; out_recs[n].nfull = live ? nfull : 0;
    }
    for (int i = tid; i < nl; i += blockDim.x) crop_move(lists + (long)n * stride + i, out_lists + (long)n * stride + i, fs1, fs2, fx, fy);
}

// ---- host side: the spec and the descriptors checked once for the operators and the executor forms; -1 with the target's index in the message
// the selection's class table and margin, as the crop and the redact specs carry them
int ffgpu_box_sel_check(const char *what, int nclasses, const unsigned char *classes, int margin_num, int margin_den)
{
    if (ffgpu_class_table_check(what, classes, nclasses)) return -1;
    if (margin_den < 1 || margin_den > 1024 || margin_num < 0 || margin_num > 4 * margin_den) {
        ffgpu_set_error("%s: margin %d / %d (den 1..1024, num 0..4 den)", what, margin_num, margin_den);
        return -1;
    }
    return 0;
}

int ffgpu_crop_spec_check(const char *what, const ffgpu_crop_spec *sp, CropPlan &pl)
{
    if (!sp) { ffgpu_set_error("%s: NULL spec", what); return -1; }
    if (sp->out_w < 1 || sp->out_w > 4096 || sp->out_h < 1 || sp->out_h > 4096) { ffgpu_set_error("%s: out size %d x %d is outside 1..4096", what, sp->out_w, sp->out_h); return -1; }
    if (sp->form != FFGPU_CROP_F32 && sp->form != FFGPU_CROP_U8) { ffgpu_set_error("%s: form %d is neither FFGPU_CROP_F32 nor FFGPU_CROP_U8", what, sp->form); return -1; }
    if (sp->per_target < 1 || sp->per_target > (1 << 24)) { ffgpu_set_error("%s: per_target %d is outside 1..2^24", what, sp->per_target); return -1; }
    if (ffgpu_box_sel_check(what, sp->nclasses, sp->classes, sp->margin_num, sp->margin_den)) return -1;
    if (sp->reserved != 0) { ffgpu_set_error("%s: spec: reserved must be 0", what); return -1; }
    memset(&pl, 0, sizeof pl);
    pl.out_w = sp->out_w; pl.out_h = sp->out_h; pl.form = sp->form; pl.per_target = sp->per_target; pl.min_score = sp->min_score;
    pl.nclasses = sp->nclasses; pl.num = sp->margin_num; pl.den = sp->margin_den;
    for (int i = 0; i < 3; i++) { pl.mean[i] = sp->mean[i]; pl.norm[i] = sp->norm[i]; }
    if (sp->classes) memcpy(pl.classes, sp->classes, (size_t)sp->nclasses);
    return 0;
}

int ffgpu_crop_buffers_check(const char *what, const void *d_out, const void *d_table, int capacity)
{
    if (!d_out) { ffgpu_set_error("%s: NULL output", what); return -1; }
    if (!d_table) { ffgpu_set_error("%s: NULL table", what); return -1; }
    if (capacity < 1 || capacity > (1 << 24)) { ffgpu_set_error("%s: capacity %d is outside 1..2^24", what, capacity); return -1; }
    if ((reinterpret_cast<uintptr_t>(d_out) | reinterpret_cast<uintptr_t>(d_table)) & 15) { ffgpu_set_error("%s: the output and the table must be 16-byte aligned", what); return -1; }
    return 0;
}

// sources[t] takes its boxes from record t of `src`; every byte of the table and of `capacity` slots is written
int ffgpu_launch_crop(bool nv12, const DetSource &src, const std::vector<CropSrc> &sources, const CropPlan &pl, void *d_out, void *d_table, int capacity, hipStream_t s)
{
    const int n = (int)sources.size(), stride = src.stride;
    if ((long long)n * stride > 0x7fffffffLL) { ffgpu_set_error("crop_boxes: %d targets of up to %d boxes is too large", n, stride); return -1; }
    for (int t0 = 0; t0 < n; t0 += CROP_ARG_TARGETS) {
        const int nt = std::min(CROP_ARG_TARGETS, n - t0);
        CropSelArgs a;
        memset(&a, 0, sizeof a);
        memcpy(a.t, sources.data() + t0, sizeof(CropSrc) * (size_t)nt);
        for (int i = 0; i < nt; i++) a.t[i].first = src.first[t0 + i];
        memcpy(a.classes, pl.classes, sizeof a.classes);
        a.nt = nt; a.rec0 = t0; a.first = t0 == 0; a.last = t0 + nt == n;
        a.out_w = pl.out_w; a.out_h = pl.out_h; a.per_target = pl.per_target; a.nclasses = pl.nclasses; a.num = pl.num; a.den = pl.den; a.min_score = pl.min_score;
        hipLaunchKernelGGL(k_crop_select, dim3(1), dim3(CROP_ARG_TARGETS * CROP_GROUP), 0, s, a, src.recs, src.lists, stride, (int *)d_table, capacity);
        LAUNCH_OK("crop_select");
    }
    const unsigned gx = (unsigned)(((long)((pl.out_w + 3) / 4) * pl.out_h + 255) / 256);
    const bool u8 = pl.form == FFGPU_CROP_U8;
    for (int t0 = 0; t0 < n; t0 += CROP_ARG_TARGETS)
        for (int slot0 = 0; slot0 < capacity; slot0 += CROP_MAX_GRID_Y) {
            CropPixArgs a;
            memset(&a, 0, sizeof a);
            a.nt = std::min(CROP_ARG_TARGETS, n - t0); a.t0 = t0; a.slot0 = slot0; a.tail = t0 == 0; a.W = pl.out_w; a.H = pl.out_h;
            memcpy(a.t, sources.data() + t0, sizeof(CropSrc) * (size_t)a.nt);
            for (int i = 0; i < 3; i++) { a.p.mean[i] = pl.mean[i]; a.p.norm[i] = pl.norm[i]; }
            const dim3 grid(gx, (unsigned)std::min(CROP_MAX_GRID_Y, capacity - slot0));
            if (nv12) {
                if (u8) hipLaunchKernelGGL((k_crop_pixels<true, true>), grid, dim3(256), 0, s, a, (const int *)d_table, d_out, capacity);
                else    hipLaunchKernelGGL((k_crop_pixels<true, false>), grid, dim3(256), 0, s, a, (const int *)d_table, d_out, capacity);
            } else {
                if (u8) hipLaunchKernelGGL((k_crop_pixels<false, true>), grid, dim3(256), 0, s, a, (const int *)d_table, d_out, capacity);
                else    hipLaunchKernelGGL((k_crop_pixels<false, false>), grid, dim3(256), 0, s, a, (const int *)d_table, d_out, capacity);
            }
            LAUNCH_OK("crop_pixels");
        }
    return 0;
}

template <class Frame>
static int crop_boxes_dev(const char *what, const void *d_records, const void *d_lists, int list_stride, const int *list_first,
                          const Frame *sources, int ntargets, const ffgpu_crop_spec *spec, void *d_out, void *d_table, int capacity, void *stream)
{
    if (ffgpu_no_device(what)) return -1;
    if (!sources) { ffgpu_set_error("%s: NULL targets", what); return -1; }
    CropPlan pl;
    if (ffgpu_crop_spec_check(what, spec, pl) || ffgpu_crop_buffers_check(what, d_out, d_table, capacity)) return -1;
    if (ntargets < 1 || ntargets > (1 << 24)) { ffgpu_set_error("%s: %d targets (ntargets >= 1)", what, ntargets); return -1; }
    DetSource src;
    if (ffgpu_source_dev(what, d_records, d_lists, list_stride, list_first, ntargets, src)) return -1;
    std::vector<CropSrc> tab;
    if (ffgpu_frame_table(what, FRAME_DRAW, sources, ntargets, tab)) return -1;
    return ffgpu_launch_crop(std::is_same<Frame, ffgpu_nv12_frame>::value, src, tab, pl, d_out, d_table, capacity, (hipStream_t)stream);
}

extern "C" int ffgpu_crop_boxes_bgr_dev(const void *d_records, const void *d_lists, int list_stride, const int *list_first, const ffgpu_bgr_frame *sources,
                                        int ntargets, const ffgpu_crop_spec *spec, void *d_out, void *d_table, int capacity, void *stream)
{
    return crop_boxes_dev("crop_boxes_bgr_dev", d_records, d_lists, list_stride, list_first, sources, ntargets, spec, d_out, d_table, capacity, stream);
}

extern "C" int ffgpu_crop_boxes_nv12_dev(const void *d_records, const void *d_lists, int list_stride, const int *list_first, const ffgpu_nv12_frame *sources,
                                         int ntargets, const ffgpu_crop_spec *spec, void *d_out, void *d_table, int capacity, void *stream)
{
    return crop_boxes_dev("crop_boxes_nv12_dev", d_records, d_lists, list_stride, list_first, sources, ntargets, spec, d_out, d_table, capacity, stream);
}

extern "C" int ffgpu_crops_to_source_dev(const void *d_table, int capacity, const void *d_records, const void *d_lists, int list_stride,
                                         void *d_out_records, void *d_out_lists, void *stream)
{
    const char *const what = "crops_to_source_dev";
    if (ffgpu_no_device(what)) return -1;
    if (!d_table) { ffgpu_set_error("%s: NULL table", what); return -1; }
    if (!d_records || !d_out_records) { ffgpu_set_error("%s: NULL records", what); return -1; }
    if (capacity < 1 || capacity > (1 << 24)) { ffgpu_set_error("%s: capacity %d is outside 1..2^24", what, capacity); return -1; }
    if (reinterpret_cast<uintptr_t>(d_table) & 15) { ffgpu_set_error("%s: the table must be 16-byte aligned", what); return -1; }
    if (ffgpu_list_stride(what, d_lists, list_stride) < 0) return -1;
    hipLaunchKernelGGL(k_crops_to_source, dim3((unsigned)capacity), dim3(FFGPU_MAX_DET), 0, (hipStream_t)stream, (const int *)d_table, capacity,
                       (const ffgpu_frame_dets *)d_records, (const BBOX *)d_lists, d_lists ? list_stride : 0, (ffgpu_frame_dets *)d_out_records, (BBOX *)d_out_lists);
    LAUNCH_OK("crops_to_source");
    return 0;
}

extern "C" size_t ffgpu_crop_table_bytes(int capacity) { return capacity < 1 ? 0 : 16 + sizeof(ffgpu_crop) * (size_t)capacity; }

extern "C" size_t ffgpu_crop_slot_bytes(int out_w, int out_h, int form)
{
    if (out_w < 1 || out_h < 1 || out_w > 4096 || out_h > 4096) return 0;
    if (form == FFGPU_CROP_F32) return sizeof(float) * 3 * (size_t)out_w * (size_t)out_h;
    return form == FFGPU_CROP_U8 ? (size_t)out_h * (((size_t)3 * out_w + 3) & ~(size_t)3) : 0;
}
