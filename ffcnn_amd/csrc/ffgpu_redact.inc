// ffgpu_redact.inc -- the detections' regions (or everything but them) replaced in the frames on the device by a solid colour or a mosaic
// (ffgpu_redact_boxes_bgr_dev / _nv12_dev, ffgpu_exec_redact_bgr / _nv12): privacy masking where the frames and the records lie.  The contract is
// in include/ffcnn_hip.h.
//
// Frame-driven, one owner per byte: a target is cut into square blocks of REDACT_SIDE(cell) pixels anchored at its pixel (0, 0) -- a whole number of
// mosaic cells, even, so an NV12 chroma sample's luma pixels lie in one block -- and one workgroup owns a block: it alone reads and writes the block's
// bytes.  It first turns the list into the block's coverage, one 64-bit mask per pixel row (the boxes staged in LDS 256 at a time; each lane ORs
// into a row of its own, so no atomic and no order), leaves if nothing is covered, and then takes the block four cell rows at a time, a wave per
// cell row and a lane per pixel column: the wave sums the cells that have a covered pixel (loads along a row, a strided scan across the lanes),
// the workgroup passes a barrier, the wave stores the covered pixels.  Everything is integer arithmetic; the result is the same bytes on every run.
//
// The target table, the class filter and the spec travel as ONE by-value kernel argument (REDACT_ARG_TARGETS targets per launch; more targets: more
// launches), as the draw's do.
#define REDACT_ARG_TARGETS 64
#define REDACT_LDS_BOXES   256                 // boxes staged per trip
#define REDACT_MAX_BLOCKS  (1 << 23)           // per target: the grid's x extent
#define REDACT_SIDE(cell)  ((cell) > 0 ? (cell) * (64 / (cell)) : 64)      // 33 .. 64; FILL: 64
struct RedactArgs {
    DrawTarget    t[REDACT_ARG_TARGETS];
    unsigned char classes[256];
    int   nclasses, num, den;                  // (these four and classes: what crop_region reads)
    float min_score;
    int   mode, cell, outside, rec0;
    unsigned colour;                           // byte 0, 1, 2: B G R / Y U V
    int   pad_[3];
};
static_assert(sizeof(RedactArgs) + 3 * 8 <= 4096 - 256, "the tables travel as a kernel argument (4 KB at most, the hidden arguments included)");
static_assert(sizeof(ffgpu_redact_spec) == 40, "include/ffcnn_hip.h states this size");
static_assert(WAVE == 64, "k_redact: a lane per pixel column of a block, a 64-bit mask per pixel row");

// bits lo .. hi (0 <= lo <= hi <= 63)
__device__ __forceinline__ unsigned long long redact_bits(int lo, int hi) { return (~0ull >> (63 - (hi - lo))) << lo; }

// The sum of v over lanes f, f + step, .. e of the wave (f and e are this lane's own; step 1 or 2), in every lane: an inclusive scan over the lanes of
// one residue, then two reads.  Integers: exact whatever the order.  Every lane of the wave calls it.
__device__ __forceinline__ unsigned redact_seg_sum(unsigned v, int step, int f, int e)
{
    const int lane = threadIdx.x & (WAVE - 1);
    for (int d = step; d < WAVE; d <<= 1) { const unsigned up = __shfl_up(v, d); if (lane >= d) v += up; }
    const unsigned hi = __shfl(v, e), lo = __shfl(v, max(f - step, 0));
    return hi - (f >= step ? lo : 0u);
}

// m[c] += byte c of rows y0 .. y1 - 1 of this lane's column (p: the column in row 0 of the block, pitch in bytes).  The loads of eight, then of four
// rows are issued before the first is added: a cell row is bound by the latency of its loads, not by their number.
template <int NC, int ROWS>
__device__ __forceinline__ void redact_col_rows(const unsigned char *p, size_t pitch, int y, unsigned m[NC])
{
    unsigned v[ROWS][NC];
#pragma unroll
    for (int i = 0; i < ROWS; i++)
#pragma unroll
        for (int c = 0; c < NC; c++) v[i][c] = p[(size_t)(y + i) * pitch + c];
#pragma unroll
    for (int i = 0; i < ROWS; i++)
#pragma unroll
        for (int c = 0; c < NC; c++) m[c] += v[i][c];
}
template <int NC>
__device__ __forceinline__ void redact_col_sum(const unsigned char *p, size_t pitch, int y0, int y1, unsigned m[NC])
{
    int y = y0;
    for (; y + 8 <= y1; y += 8) redact_col_rows<NC, 8>(p, pitch, y, m);
    if (y + 4 <= y1) { redact_col_rows<NC, 4>(p, pitch, y, m); y += 4; }
    for (; y < y1; y++) redact_col_rows<NC, 1>(p, pitch, y, m);
}

// S of one block (bx0, by0, bw x bh pixels of a w x h target) into s_cov, a 64-bit mask per pixel row (rows >= bh: 0): the first stage of k_redact
// and of k_blur (ffgpu_blur.inc).  Args: the kernel's argument struct with crop_region's selection fields and `outside`.  The list is staged
// REDACT_LDS_BOXES at a time; lane (wv, row) ORs the columns of boxes wv, wv + 4, .. of every trip into its own register.  Every lane of the 256
// calls it; true in every lane when a bit is set.  The LDS arrays are the caller's: s_xm, s_ya, s_yb [REDACT_LDS_BOXES], s_part [4][WAVE], s_cov [WAVE].
template <class Args>
__device__ __forceinline__ bool redact_coverage(const Args &a, const BBOX *list, int n, int w, int h, int bx0, int by0, int bw, int bh,
                                                unsigned long long *s_xm, int *s_ya, int *s_yb, unsigned long long (*s_part)[WAVE], unsigned long long *s_cov)
{
    typedef unsigned long long u64;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
    u64 acc = 0;
    for (int c0 = 0; c0 < n; c0 += REDACT_LDS_BOXES) {
        u64 xm = 0;
        int ya = 1, yb = 0;
        int4 r;
        if (c0 + tid < n && crop_region(list[c0 + tid], a, w, h, r) == 2) {
            const int xa = max(r.x, bx0) - bx0, xb = min(r.x + r.z - 1, bx0 + bw - 1) - bx0;
            const int y0 = max(r.y, by0) - by0, y1 = min(r.y + r.w - 1, by0 + bh - 1) - by0;
            if (xa <= xb && y0 <= y1) { xm = redact_bits(xa, xb); ya = y0; yb = y1; }
        }
        s_xm[tid] = xm; s_ya[tid] = ya; s_yb[tid] = yb;
        __syncthreads();
        const int cnt = min(REDACT_LDS_BOXES, n - c0);
        for (int k = wv; k < cnt; k += 4) if (s_ya[k] <= lane && lane <= s_yb[k]) acc |= s_xm[k];
        __syncthreads();
    }
    s_part[wv][lane] = acc;
    __syncthreads();
    u64 mine = 0;
    if (tid < WAVE) {
        const u64 u = s_part[0][tid] | s_part[1][tid] | s_part[2][tid] | s_part[3][tid];
        mine = tid < bh ? (a.outside ? ~u : u) & redact_bits(0, bw - 1) : 0;
        s_cov[tid] = mine;
    }
    return __syncthreads_or(mine != 0);
}

// grid (blocks of the launch's largest target, targets of this launch), 256 lanes.  Target blockIdx.y reads record rec0 + blockIdx.y as k_draw_boxes
// does (counts clamped to [0, stride]); a workgroup beyond its target's own blocks leaves.  Every load and store lies inside the block, clipped to the
// target's w x h.
template <bool NV12>
__global__ void __launch_bounds__(256) k_redact(RedactArgs a, const ffgpu_frame_dets *recs, const BBOX *lists, int stride)
{
    typedef unsigned long long u64;
    __shared__ u64 s_xm[REDACT_LDS_BOXES];                // a staged box inside this block: its columns ...
    __shared__ int s_ya[REDACT_LDS_BOXES], s_yb[REDACT_LDS_BOXES];   // ... and its rows (ya > yb: none)
    __shared__ u64 s_part[4][WAVE], s_cov[WAVE];          // row y's covered columns: each wave's share of the boxes, then S itself
    const DrawTarget &t = a.t[blockIdx.y];
    if (!t.p0) return;                                                                // a skipped target (uniform)
    const int w = t.w, h = t.h, side = REDACT_SIDE(a.cell);
    const long long nbx = ((long long)w + side - 1) / side, nby = ((long long)h + side - 1) / side;
    if ((long long)blockIdx.x >= nbx * nby) return;                                   // (uniform)
    const int bx0 = (int)(blockIdx.x % nbx) * side, by0 = (int)(blockIdx.x / nbx) * side, bw = min(side, w - bx0), bh = min(side, h - by0);
    const ffgpu_frame_dets *rec = recs + a.rec0 + blockIdx.y;
    const int n = max(0, min(lists ? rec->nfull : rec->count, stride));
    if (n == 0 && !a.outside) return;                                                 // (uniform)
    const BBOX *list = lists ? lists + t.first : rec->box;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;

    // ---- S of this block
    if (!redact_coverage(a, list, n, w, h, bx0, by0, bw, bh, s_xm, s_ya, s_yb, s_part, s_cov)) return;   // nothing to write: no pixel is touched

    const unsigned c0 = a.colour & 0xffu, c1 = (a.colour >> 8) & 0xffu, c2 = (a.colour >> 16) & 0xffu;
    unsigned char *const row0 = t.p0 + (size_t)by0 * (size_t)t.pitch + (NV12 ? 1 : 3) * (size_t)bx0;     // pixel (bx0, by0)
    auto put = [&](int y, unsigned v0, unsigned v1, unsigned v2) {                     // pixel (bx0 + lane, by0 + y)
        unsigned char *px = row0 + (size_t)y * (size_t)t.pitch + (NV12 ? 1 : 3) * lane;
        px[0] = (unsigned char)v0;
        if (!NV12) { px[1] = (unsigned char)v1; px[2] = (unsigned char)v2; }
    };
    // NV12: the block's chroma samples, (bw + 1) / 2 x (bh + 1) / 2 of them from sample (bx0 / 2, by0 / 2); sample (i, jj) is covered when any bit
    // 2 i, 2 i + 1 of rows 2 jj, 2 jj + 1 is (rows and columns outside w x h hold no bit)
    unsigned char *const uv0 = NV12 ? t.p1 + (size_t)(by0 >> 1) * (size_t)t.pitch_uv + 2 * (size_t)(bx0 >> 1) : nullptr;
    const int cbw = (bw + 1) >> 1, cbh = (bh + 1) >> 1, smp = lane >> 1;
    auto cov_uv = [&](int jj) { return s_cov[2 * jj] | s_cov[2 * jj + 1]; };           // (2 jj + 1 <= 63: side is even)

    if (a.mode == FFGPU_REDACT_FILL) {
        for (int y = wv; y < bh; y += 4)
            if ((s_cov[y] >> lane) & 1) put(y, c0, c1, c2);
        if (NV12)
            for (int jj = wv; jj < cbh; jj += 4)
                if (lane < cbw && ((cov_uv(jj) >> (2 * lane)) & 3))
                    *reinterpret_cast<unsigned short *>(uv0 + (size_t)jj * (size_t)t.pitch_uv + 2 * lane) = (unsigned short)(c1 | c2 << 8);
        return;
    }

    // ---- MOSAIC.  Pixels (BGR; NV12: luma): lane = column, this lane's cell is columns f .. e of the block.
    {
        const int s = a.cell, ncy = (bh + s - 1) / s;
        const int f = lane < bw ? lane / s * s : 0, e = lane < bw ? min(f + s, bw) - 1 : 0;
        const u64 cellbits = lane < bw ? redact_bits(f, e) : 0;
        for (int j0 = 0; j0 < ncy; j0 += 4) {                                          // (ncy: the same in every wave, so is the barrier)
            const int j = j0 + wv, y0 = j * s, y1 = j < ncy ? min(y0 + s, bh) : y0;
            u64 any = 0;
            for (int y = y0; y < y1; y++) any |= s_cov[y];                             // (the same in every lane of the wave)
            unsigned m[3] = { 0, 0, 0 };
            if (any) {
                if (any & cellbits)                                                    // a cell with no covered pixel is not read
                    redact_col_sum<NV12 ? 1 : 3>(row0 + (NV12 ? 1 : 3) * lane, (size_t)t.pitch, y0, y1, m);
                const unsigned np = (unsigned)((e - f + 1) * (y1 - y0));
                for (int c = 0; c < (NV12 ? 1 : 3); c++) m[c] = (redact_seg_sum(m[c], 1, f, e) + np / 2) / np;
            }
            __syncthreads();                                                           // every load of these cells is complete
            for (int y = y0; y < y1; y++)
                if ((s_cov[y] >> lane) & 1) put(y, m[0], m[1], m[2]);
        }
    }
    // ---- NV12 chroma: lane = byte of a U V row (sample lane / 2, U or V by its parity), cells of s / 2 samples, the sums over lanes of one parity
    if (NV12) {
        const int hs = a.cell >> 1, ncy = (cbh + hs - 1) / hs, par = lane & 1;
        const int f = smp < cbw ? smp / hs * hs : 0, e = smp < cbw ? min(f + hs, cbw) - 1 : 0;
        const u64 cellbits = smp < cbw ? redact_bits(2 * f, 2 * e + 1) : 0;
        for (int j0 = 0; j0 < ncy; j0 += 4) {
            const int j = j0 + wv, y0 = j * hs, y1 = j < ncy ? min(y0 + hs, cbh) : y0;
            u64 any = 0;
            for (int jj = y0; jj < y1; jj++) any |= cov_uv(jj);
            unsigned m = 0;
            if (any) {
                if (any & cellbits) redact_col_sum<1>(uv0 + lane, (size_t)t.pitch_uv, y0, y1, &m);
                const unsigned np = (unsigned)((e - f + 1) * (y1 - y0));
                m = (redact_seg_sum(m, 2, 2 * f + par, 2 * e + par) + np / 2) / np;
            }
            __syncthreads();
            for (int jj = y0; jj < y1; jj++)
                if (smp < cbw && ((cov_uv(jj) >> (2 * smp)) & 3)) uv0[(size_t)jj * (size_t)t.pitch_uv + lane] = (unsigned char)m;
        }
    }
}

// ---- host side: the caller's spec checked once for the operators and the executor forms (the descriptors: ffgpu_frame_table, role FRAME_DRAW)
int ffgpu_redact_spec_check(const char *what, const ffgpu_redact_spec *sp, bool nv12, RedactPlan &pl)
{
    if (!sp) { ffgpu_set_error("%s: NULL spec", what); return -1; }
    if (sp->mode != FFGPU_REDACT_FILL && sp->mode != FFGPU_REDACT_MOSAIC) { ffgpu_set_error("%s: mode %d is neither FFGPU_REDACT_FILL nor FFGPU_REDACT_MOSAIC", what, sp->mode); return -1; }
    if (sp->flags & ~FFGPU_REDACT_OUTSIDE) { ffgpu_set_error("%s: unknown flags 0x%x", what, (unsigned)sp->flags); return -1; }
    if (sp->mode == FFGPU_REDACT_FILL ? sp->cell != 0 : (sp->cell < 2 || sp->cell > 64)) {
        ffgpu_set_error("%s: cell %d (0 with FFGPU_REDACT_FILL, 2..64 with FFGPU_REDACT_MOSAIC)", what, sp->cell);
        return -1;
    }
    if (nv12 && (sp->cell & 1)) { ffgpu_set_error("%s: cell %d is odd (NV12 targets: a chroma cell is half a luma cell)", what, sp->cell); return -1; }
    if (ffgpu_box_sel_check(what, sp->nclasses, sp->classes, sp->margin_num, sp->margin_den)) return -1;
    memset(&pl, 0, sizeof pl);
    pl.mode = sp->mode; pl.cell = sp->cell; pl.outside = sp->flags & FFGPU_REDACT_OUTSIDE; pl.min_score = sp->min_score;
    pl.nclasses = sp->nclasses; pl.num = sp->margin_num; pl.den = sp->margin_den;
    pl.colour = ffgpu_pack_colour(sp->color);
    if (sp->classes) memcpy(pl.classes, sp->classes, (size_t)sp->nclasses);
    return 0;
}

// targets[t] is redacted by record t of `src`; REDACT_ARG_TARGETS targets per launch, the grid sized by the launch's largest target
int ffgpu_launch_redact(const char *what, bool nv12, const DetSource &src, const std::vector<DrawTarget> &targets, const RedactPlan &pl, hipStream_t s)
{
    const int n = (int)targets.size(), side = REDACT_SIDE(pl.cell);
    auto blocks = [side](const DrawTarget &t) { return t.p0 ? (((long long)t.w + side - 1) / side) * (((long long)t.h + side - 1) / side) : 0LL; };
    for (int k = 0; k < n; k++)
        if (blocks(targets[k]) > REDACT_MAX_BLOCKS) {
            ffgpu_set_error("%s: target %d: %d x %d is more than 2^23 blocks of %d x %d pixels", what, k, targets[k].w, targets[k].h, side, side);
            return -1;
        }
    for (int t0 = 0; t0 < n; t0 += REDACT_ARG_TARGETS) {
        const int nt = std::min(REDACT_ARG_TARGETS, n - t0);
        RedactArgs a;
        memset(&a, 0, sizeof a);
        memcpy(a.t, targets.data() + t0, sizeof(DrawTarget) * (size_t)nt);
        long long most = 0;
        for (int i = 0; i < nt; i++) { a.t[i].first = src.first[t0 + i]; most = std::max(most, blocks(a.t[i])); }
        if (most == 0) continue;                                                       // every target of this launch is skipped
        memcpy(a.classes, pl.classes, sizeof a.classes);
        a.nclasses = pl.nclasses; a.num = pl.num; a.den = pl.den; a.min_score = pl.min_score;
        a.mode = pl.mode; a.cell = pl.cell; a.outside = pl.outside; a.rec0 = t0; a.colour = pl.colour;
        const dim3 grid((unsigned)most, (unsigned)nt);
        if (nv12) hipLaunchKernelGGL(k_redact<true>, grid, dim3(256), 0, s, a, src.recs, src.lists, src.stride);
        else      hipLaunchKernelGGL(k_redact<false>, grid, dim3(256), 0, s, a, src.recs, src.lists, src.stride);
        LAUNCH_OK("redact");
    }
    return 0;
}

template <class Frame>
static int redact_boxes_dev(const char *what, const void *d_records, const void *d_lists, int list_stride, const int *list_first,
                            const Frame *targets, int ntargets, const ffgpu_redact_spec *spec, void *stream)
{
    const bool nv12 = std::is_same<Frame, ffgpu_nv12_frame>::value;
    if (ffgpu_no_device(what)) return -1;
    if (!targets) { ffgpu_set_error("%s: NULL targets", what); return -1; }
    RedactPlan pl;
    if (ffgpu_redact_spec_check(what, spec, nv12, pl)) return -1;
    if (ntargets < 1 || ntargets > (1 << 24)) { ffgpu_set_error("%s: %d targets (ntargets >= 1)", what, ntargets); return -1; }
    DetSource src;
    if (ffgpu_source_dev(what, d_records, d_lists, list_stride, list_first, ntargets, src)) return -1;
    std::vector<DrawTarget> tab;
    if (ffgpu_frame_table(what, FRAME_DRAW, targets, ntargets, tab)) return -1;
    return ffgpu_launch_redact(what, nv12, src, tab, pl, (hipStream_t)stream);
}

extern "C" int ffgpu_redact_boxes_bgr_dev(const void *d_records, const void *d_lists, int list_stride, const int *list_first,
                                          const ffgpu_bgr_frame *targets, int ntargets, const ffgpu_redact_spec *spec, void *stream)
{
    return redact_boxes_dev("redact_boxes_bgr_dev", d_records, d_lists, list_stride, list_first, targets, ntargets, spec, stream);
}

extern "C" int ffgpu_redact_boxes_nv12_dev(const void *d_records, const void *d_lists, int list_stride, const int *list_first,
                                           const ffgpu_nv12_frame *targets, int ntargets, const ffgpu_redact_spec *spec, void *stream)
{
    return redact_boxes_dev("redact_boxes_nv12_dev", d_records, d_lists, list_stride, list_first, targets, ntargets, spec, stream);
}
