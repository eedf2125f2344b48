// ffgpu_blur.inc -- the detections' regions (or everything but them) box-blurred in the frames on the device (ffgpu_blur_boxes_bgr_dev / _nv12_dev,
// ffgpu_exec_blur_bgr / _nv12).  The contract is in include/ffcnn_hip.h.
//
// A blur window reaches into pixels that another workgroup rewrites, so a pass is TWO launches of one kernel and a scratch surface of the caller's:
// the blur launch (source = target, destination = scratch, radius r) reads the target everywhere and writes the blurred values of the covered set S
// into the scratch -- nobody writes the target during it; the copy-back launch (source = scratch, destination = target, radius 0: the identity
// mean) copies S back -- nobody reads outside its own block during it.  Stream order between the two is the barrier.  Every byte has one owner per
// launch: a workgroup owns a 64 x 64 block of the DESTINATION, anchored at pixel (0, 0), and only lanes whose coverage bit is set store.
//
// The kernel: coverage exactly as k_redact's first stage (redact_coverage, ffgpu_redact.inc), then per plane (BGR; NV12: luma, then chroma with
// rc = (r + 1) / 2 on the samples the FILL rule covers) a separable window sum through LDS.  Horizontal: a wave takes a row of the tile (the block's
// covered rows +- r, clipped to the plane), stages its bytes in LDS along the row -- consecutive lanes on consecutive dwords where the address is
// aligned, single bytes at the two ends, nothing outside the row segment --, a lane takes a pixel, an inclusive scan over the lanes gives the
// prefix sums P and two reads the window sum P[x + r] - P[x - r - 1] with the clip; the sums (at most 63 x 255) go to LDS as 16-bit values.  A
// barrier.  Vertical: a lane takes a column and a wave 16 rows; a running column sum adds the entering row and subtracts the leaving one, n is
// closed form from the clipped extents and the rounding division is exact.  Integers throughout, plain C++, no atomics.
//
// The two surface tables, the class filter and the spec travel as ONE by-value kernel argument: 64 BGR targets or 48 NV12 targets per launch (an
// NV12 target and its scratch are four planes: 64 bytes an entry, and 64 of them are the 4 KB themselves).
#define BLUR_ARG_TARGETS(nv12) ((nv12) ? 48 : 64)
#define BLUR_TILE    126                       // rows (and columns) of a tile: a block's 64 and 31 on either side
#define BLUR_RAW_DW  96                        // a wave's staged row segment: 3 bytes of misalignment + 3 x 126 bytes
#define BLUR_ROWS    8                         // tile rows whose loads a wave has in flight
struct BlurSurf {                              // one target and its scratch as a launch reads them: s = this launch's source, d = its destination
    unsigned char *s0, *d0;                    // row 0 of the BGR pixels / of the Y plane; s0 == NULL: a skipped target
    long long first;
    int w, h, spitch, dpitch;
};
struct BlurSurfUV {
    unsigned char *s1, *d1;                    // NV12: row 0 of the interleaved U V plane
    int spitch_uv, dpitch_uv;
};
template <bool NV12>
struct BlurArgs {
    BlurSurf      t[BLUR_ARG_TARGETS(NV12)];
    BlurSurfUV    uv[NV12 ? BLUR_ARG_TARGETS(NV12) : 1];
    unsigned char classes[256];
    int   nclasses, num, den;                  // (these four and classes: what crop_region reads)
    float min_score;
    int   radius, outside, rec0, pad_;
};
static_assert(sizeof(BlurArgs<false>) + 3 * 8 <= 4096 - 256 && sizeof(BlurArgs<true>) + 3 * 8 <= 4096 - 256,
              "the tables travel as a kernel argument (4 KB at most, the hidden arguments included)");
static_assert(sizeof(ffgpu_blur_spec) == 40, "include/ffcnn_hip.h states this size");
static_assert(2 * 31 + 64 == BLUR_TILE && 3 + 3 * BLUR_TILE <= 4 * BLUR_RAW_DW && 63 * 255 < 65536 && 126 * 255 < 32768,
              "k_blur: a window sum is a 16-bit value, two prefix sums share a register");

// (s + n / 2 has been added by the caller) s / n for s <= 63 * 63 * 255 + n / 2, n <= 3 969 and rn = 1.0f / n: the quotient is at most 255, so the float
// product is off by far less than 1 / n and its floor by at most one, which the remainder shows and the two corrections mend: exact.
__device__ __forceinline__ unsigned blur_div(unsigned s, unsigned n, float rn)
{
    unsigned q = (unsigned)((float)s * rn);
    const int rem = (int)(s - q * n);
    if (rem < 0) q--; else if (rem >= (int)n) q++;
    return q;
}

// which pixels of a block's row the lanes store: the luma pixels / BGR pixels of S, and the chroma samples of the FILL rule (sample i of sample row
// jj is covered when any bit 2 i, 2 i + 1 of rows 2 jj, 2 jj + 1 is; rows and columns outside w x h hold no bit)
struct BlurCovPix {
    const unsigned long long *cov;
    __device__ __forceinline__ bool any(int y) const { return cov[y] != 0; }
    __device__ __forceinline__ bool bit(int y, int lane) const { return (cov[y] >> lane) & 1; }
};
struct BlurCovUV {
    const unsigned long long *cov;
    __device__ __forceinline__ unsigned long long row(int jj) const { return cov[2 * jj] | cov[2 * jj + 1]; }
    __device__ __forceinline__ bool any(int jj) const { return row(jj) != 0; }
    __device__ __forceinline__ bool bit(int jj, int lane) const { return lane < 32 && ((row(jj) >> (2 * (lane & 31))) & 3); }
};

// One plane of NC interleaved channels, pw x ph pixels: the block at (x0, y0), bw x bh pixels (at most 64 x 64), blurred with radius r from src
// into dst at the pixels cov names.  Every lane of the 256 calls it.  Loads: rows 0 .. ph - 1, bytes 0 .. NC pw - 1 of src; stores: the block's
// covered pixels in dst.
template <int NC, class Cov>
__device__ __forceinline__ void blur_plane(const unsigned char *src_, size_t spitch, unsigned char *dst_, size_t dpitch, int pw, int ph,
                                           int x0, int y0, int bw, int bh, int r, const Cov cov,
                                           unsigned (*s_h32)[WAVE], unsigned short (*s_h16)[WAVE], unsigned *s_raw)
{
    typedef unsigned long long u64;
    constexpr int NREG = (NC + 1) / 2;                                                 // two channels' prefix sums share a register
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
    const FFG unsigned char *const src = (const FFG unsigned char *)src_;              // (the surfaces ARE global memory: global_load / _store, vmcnt only)
    FFG unsigned char *const dst = (FFG unsigned char *)dst_;
    FFG unsigned char *const drow0 = dst + (size_t)y0 * dpitch + NC * (size_t)x0;      // pixel (x0, y0)
    if (r == 0) {                                                                      // the copy-back: the mean of one pixel, no tile
        const FFG unsigned char *const srow0 = src + (size_t)y0 * spitch + NC * (size_t)x0;
        for (int yg = wv; yg < bh; yg += 16) {                                         // four rows' loads, then their stores
            unsigned char v[4][NC];
            bool on[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int y = yg + 4 * i;
                on[i] = y < bh && cov.bit(min(y, bh - 1), lane);
                if (on[i]) {
#pragma unroll
                    for (int c = 0; c < NC; c++) v[i][c] = srow0[(size_t)y * spitch + NC * lane + c];
                }
            }
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (on[i]) {
#pragma unroll
                    for (int c = 0; c < NC; c++) drow0[(size_t)(yg + 4 * i) * dpitch + NC * lane + c] = v[i][c];
                }
        }
        return;
    }
    const u64 rows = __ballot(lane < bh && cov.any(min(lane, bh - 1)));                // the block's rows with a covered pixel (the same in every wave)
    if (!rows) return;                                                                 // (uniform)
    const int ymin = __ffsll(rows) - 1, ymax = 63 - __clzll(rows);
    const int tx0 = max(x0 - r, 0), nt = min(x0 + bw - 1 + r, pw - 1) - tx0 + 1;       // the tile's columns tx0 .. tx0 + nt - 1: at most 126
    const int tyA = max(y0 + ymin - r, 0), tyB = min(y0 + ymax + r, ph - 1);           // its rows: at most 126
    const int X = x0 + min(lane, bw - 1), xa = max(X - r, 0), xb = min(X + r, pw - 1); // this lane's column and its window (lanes >= bw: the last column's)

    // ---- horizontal: the window sums of the block's columns in every row of the tile
    unsigned char *const raw = reinterpret_cast<unsigned char *>(s_raw);
    // A row segment is len bytes at p: head bytes up to the first aligned address, ndw dwords (at most 95: lanes l and 64 + l), the rest single
    // bytes; lanes 0 .. 2 take the head's bytes, lanes 3 .. 5 the tail's.  The loads of BLUR_ROWS rows are issued before the first row is worked on: a
    // wave with one row in flight is bound by the latency of that load, as 5.22 found for the mosaic.
    const int len = NC * nt;
    for (int tyg = tyA + wv; tyg <= tyB; tyg += 4 * BLUR_ROWS) {
      unsigned d0[BLUR_ROWS], d1[BLUR_ROWS], de[BLUR_ROWS];
#pragma unroll
      for (int i = 0; i < BLUR_ROWS; i++) {
        d0[i] = d1[i] = de[i] = 0;
        if (tyg + 4 * i <= tyB) {                                                      // (uniform)
            const FFG unsigned char *p = src + (size_t)(tyg + 4 * i) * spitch + NC * (size_t)tx0;
            const int mis = (int)((uintptr_t)p & 3), head = min((4 - mis) & 3, len), ndw = (len - head) >> 2, tail = head + 4 * ndw;
            const int eb = lane < 3 ? (lane < head ? lane : -1) : (lane < 6 && tail + lane - 3 < len ? tail + lane - 3 : -1);
            if (lane < ndw) d0[i] = *(const FFG unsigned *)(p + head + 4 * lane);
            if (lane + WAVE < ndw) d1[i] = *(const FFG unsigned *)(p + head + 4 * (lane + WAVE));
            if (eb >= 0) de[i] = p[eb];
        }
      }
#pragma unroll
      for (int i = 0; i < BLUR_ROWS; i++) {
        const int ty = tyg + 4 * i;
        if (ty > tyB) continue;                                                        // (uniform)
        const FFG unsigned char *p = src + (size_t)ty * spitch + NC * (size_t)tx0;
        const int mis = (int)((uintptr_t)p & 3), head = min((4 - mis) & 3, len), ndw = (len - head) >> 2, tail = head + 4 * ndw;
        const int eb = lane < 3 ? (lane < head ? lane : -1) : (lane < 6 && tail + lane - 3 < len ? tail + lane - 3 : -1);
        if (lane < ndw) s_raw[((mis + head) >> 2) + lane] = d0[i];
        if (lane + WAVE < ndw) s_raw[((mis + head) >> 2) + lane + WAVE] = d1[i];
        if (eb >= 0) raw[mis + eb] = (unsigned char)de[i];
        __builtin_amdgcn_wave_barrier();                                               // (the wave's own stores, then its own loads: program order)
        unsigned lo[NREG], hi[NREG];                                                   // pixels lane and 64 + lane of the segment
#pragma unroll
        for (int k = 0; k < NREG; k++) lo[k] = hi[k] = 0;
        if (lane < nt) {
            const unsigned char *q = raw + mis + NC * lane;
            lo[0] = NC > 1 ? q[0] | (unsigned)q[1] << 16 : q[0];
            if (NC == 3) lo[NREG - 1] = q[2];
        }
        if (lane + WAVE < nt) {
            const unsigned char *q = raw + mis + NC * (lane + WAVE);
            hi[0] = NC > 1 ? q[0] | (unsigned)q[1] << 16 : q[0];
            if (NC == 3) hi[NREG - 1] = q[2];
        }
        __builtin_amdgcn_wave_barrier();                                               // (before the next row's stores)
#pragma unroll
        for (int k = 0; k < NREG; k++) {
            for (int d = 1; d < WAVE; d <<= 1) { const unsigned up = __shfl_up(lo[k], d); if (lane >= d) lo[k] += up; }
            if (nt > WAVE) {                                                           // (uniform)
                for (int d = 1; d < WAVE; d <<= 1) { const unsigned up = __shfl_up(hi[k], d); if (lane >= d) hi[k] += up; }
                hi[k] += __shfl(lo[k], WAVE - 1);
            }
            const int ib = xb - tx0, ia = max(xa - tx0 - 1, 0);                        // P[ib] - P[xa - tx0 - 1] (none below the tile's first column)
            unsigned pb = __shfl(lo[k], ib & (WAVE - 1)), pa = __shfl(lo[k], ia & (WAVE - 1));
            if (nt > WAVE) {
                const unsigned qb = __shfl(hi[k], ib & (WAVE - 1)), qa = __shfl(hi[k], ia & (WAVE - 1));
                pb = ib < WAVE ? pb : qb; pa = ia < WAVE ? pa : qa;
            }
            const unsigned hsum = pb - (xa > tx0 ? pa : 0u);                           // (no borrow between the halves: a prefix sum only grows)
            if (NC != 2 && k == NREG - 1) s_h16[ty - tyA][lane] = (unsigned short)hsum;
            else s_h32[ty - tyA][lane] = hsum;
        }
      }
    }
    __syncthreads();                                                                  // the last write of the window sums | their first read

    // ---- vertical: wave wv owns rows 16 wv .. 16 wv + 15 of the block, of which ya .. yb have a covered pixel
    const unsigned m16 = (unsigned)(rows >> (16 * wv)) & 0xffffu;
    if (!m16) return;                                                                  // (no barrier follows)
    const int ya = 16 * wv + __ffs(m16) - 1, yb = 16 * wv + 31 - __clz(m16);
    auto column = [&](int trow, unsigned v[NC]) {                                      // this lane's window sums in row trow of the tile
        if constexpr (NC != 2) v[NC - 1] = s_h16[trow][lane];
        if constexpr (NC != 1) { const unsigned u = s_h32[trow][lane]; v[0] = u & 0xffffu; v[1] = u >> 16; }
    };
    unsigned sum[NC], v[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) sum[c] = 0;
    int wa = max(y0 + ya - r, 0), wb = min(y0 + ya + r, ph - 1);                       // the window's rows, clipped
    for (int q = wa; q <= wb; q++) {
        column(q - tyA, v);
#pragma unroll
        for (int c = 0; c < NC; c++) sum[c] += v[c];
    }
    const unsigned nx = (unsigned)(xb - xa + 1);
    for (int y = ya; ; y++) {
        if (cov.bit(y, lane)) {
            const unsigned n = nx * (unsigned)(wb - wa + 1);
            const float rn = 1.0f / (float)n;
            FFG unsigned char *px = drow0 + (size_t)y * dpitch + NC * lane;
#pragma unroll
            for (int c = 0; c < NC; c++) px[c] = (unsigned char)blur_div(sum[c] + n / 2, n, rn);
        }
        if (y == yb) break;
        if (y0 + y - r >= 0) {                                                         // row y0 + y - r leaves
            column(wa - tyA, v);
#pragma unroll
            for (int c = 0; c < NC; c++) sum[c] -= v[c];
            wa++;
        }
        if (y0 + y + 1 + r <= ph - 1) {                                                // row y0 + y + 1 + r enters
            wb++;
            column(wb - tyA, v);
#pragma unroll
            for (int c = 0; c < NC; c++) sum[c] += v[c];
        }
    }
}

// grid (blocks of the launch's largest target, targets of this launch), 256 lanes, as k_redact: target blockIdx.y reads record rec0 + blockIdx.y
// (counts clamped to [0, stride]); a workgroup beyond its target's own blocks, of a skipped target, or with no covered pixel leaves before it touches
// a pixel.  radius 0: the copy-back.
template <bool NV12>
__global__ void __launch_bounds__(256) k_blur(BlurArgs<NV12> a, const ffgpu_frame_dets *recs, const BBOX *lists, int stride)
{
    typedef unsigned long long u64;
    __shared__ u64 s_xm[REDACT_LDS_BOXES];
    __shared__ int s_ya[REDACT_LDS_BOXES], s_yb[REDACT_LDS_BOXES];
    __shared__ u64 s_part[4][WAVE], s_cov[WAVE];
    __shared__ unsigned s_h32[BLUR_TILE][WAVE];                                        // the window sums of two channels (BGR: B, G; chroma: U, V) ...
    __shared__ unsigned short s_h16[BLUR_TILE][WAVE];                                  // ... and of one (BGR: R; luma)
    __shared__ unsigned s_raw[4][BLUR_RAW_DW];                                         // a row segment's bytes, per wave
    const BlurSurf &t = a.t[blockIdx.y];
    if (!t.s0) return;                                                                // a skipped target (uniform)
    const int w = t.w, h = t.h;
    const long long nbx = ((long long)w + 63) / 64, nby = ((long long)h + 63) / 64;
    if ((long long)blockIdx.x >= nbx * nby) return;                                   // (uniform)
    const int bx0 = (int)(blockIdx.x % nbx) * 64, by0 = (int)(blockIdx.x / nbx) * 64, bw = min(64, w - bx0), bh = min(64, h - by0);
    const ffgpu_frame_dets *rec = recs + a.rec0 + blockIdx.y;
    const int n = max(0, min(lists ? rec->nfull : rec->count, stride));
    if (n == 0 && !a.outside) return;                                                 // (uniform)
    const BBOX *list = lists ? lists + t.first : rec->box;
    if (!redact_coverage(a, list, n, w, h, bx0, by0, bw, bh, s_xm, s_ya, s_yb, s_part, s_cov)) return;   // nothing to write: no pixel is touched
    unsigned *const raw = s_raw[threadIdx.x / WAVE];
    if (!NV12) {
        blur_plane<3>(t.s0, (size_t)t.spitch, t.d0, (size_t)t.dpitch, w, h, bx0, by0, bw, bh, a.radius, BlurCovPix{ s_cov }, s_h32, s_h16, raw);
    } else {                                                                          // (luma's sums lie in s_h16, chroma's in s_h32: no barrier between)
        const BlurSurfUV &c = a.uv[NV12 ? blockIdx.y : 0];
        blur_plane<1>(t.s0, (size_t)t.spitch, t.d0, (size_t)t.dpitch, w, h, bx0, by0, bw, bh, a.radius, BlurCovPix{ s_cov }, s_h32, s_h16, raw);
        blur_plane<2>(c.s1, (size_t)c.spitch_uv, c.d1, (size_t)c.dpitch_uv, (w + 1) >> 1, (h + 1) >> 1, bx0 >> 1, by0 >> 1, (bw + 1) >> 1, (bh + 1) >> 1,
                      (a.radius + 1) >> 1, BlurCovUV{ s_cov }, s_h32, s_h16, raw);
    }
}

// ---- host side: the caller's spec checked once for the operators and the executor forms
int ffgpu_blur_spec_check(const char *what, const ffgpu_blur_spec *sp, BlurPlan &pl)
{
    if (!sp) { ffgpu_set_error("%s: NULL spec", what); return -1; }
    if (sp->radius < 1 || sp->radius > 31) { ffgpu_set_error("%s: radius %d (1..31)", what, sp->radius); return -1; }
    if (sp->passes < 1 || sp->passes > 3) { ffgpu_set_error("%s: passes %d (1..3)", what, sp->passes); return -1; }
    if (sp->flags & ~FFGPU_BLUR_OUTSIDE) { ffgpu_set_error("%s: unknown flags 0x%x", what, (unsigned)sp->flags); return -1; }
    if (sp->reserved != 0) { ffgpu_set_error("%s: spec: reserved must be 0", what); return -1; }
    if (ffgpu_box_sel_check(what, sp->nclasses, sp->classes, sp->margin_num, sp->margin_den)) return -1;
    memset(&pl, 0, sizeof pl);
    pl.radius = sp->radius; pl.passes = sp->passes; pl.outside = sp->flags & FFGPU_BLUR_OUTSIDE; pl.min_score = sp->min_score;
    pl.nclasses = sp->nclasses; pl.num = sp->margin_num; pl.den = sp->margin_den;
    if (sp->classes) memcpy(pl.classes, sp->classes, (size_t)sp->nclasses);
    return 0;
}

// The scratch table against the targets: NULL exactly where the target is, the same w x h, and no scratch byte shared with another scratch or with
// a target.  A surface is the bytes from the first to the last of each of its planes.  The spans sorted by their first byte: one overlaps an earlier
// one exactly when it starts before the farthest end seen.
struct BlurSpan { uintptr_t b, e; int idx; bool scratch; };
static void blur_spans(const DrawTarget &t, bool nv12, int idx, bool scratch, std::vector<BlurSpan> &out)
{
    if (!t.p0) return;
    const uintptr_t y = reinterpret_cast<uintptr_t>(t.p0);
    out.push_back(BlurSpan{ y, y + (size_t)t.pitch * (size_t)(t.h - 1) + (size_t)(nv12 ? 1 : 3) * (size_t)t.w, idx, scratch });
    if (!nv12) return;
    const uintptr_t c = reinterpret_cast<uintptr_t>(t.p1);
    out.push_back(BlurSpan{ c, c + (size_t)t.pitch_uv * (size_t)((t.h + 1) / 2 - 1) + 2 * (size_t)((t.w + 1) / 2), idx, scratch });
}
static int blur_scratch_check(const char *what, bool nv12, const std::vector<DrawTarget> &targets, const std::vector<DrawTarget> &scratch)
{
    const int n = (int)targets.size();
    std::vector<BlurSpan> spans;
    for (int k = 0; k < n; k++) {
        const DrawTarget &t = targets[k], &c = scratch[k];
        if (t.p0 && !c.p0) { ffgpu_set_error("%s: scratch %d is NULL where its target is not", what, k); return -1; }
        if (!t.p0 && c.p0) { ffgpu_set_error("%s: scratch %d is not NULL where its target is", what, k); return -1; }
        if (t.p0 && (t.w != c.w || t.h != c.h)) { ffgpu_set_error("%s: scratch %d: %d x %d is not its target's %d x %d", what, k, c.w, c.h, t.w, t.h); return -1; }
        blur_spans(t, nv12, k, false, spans);
        blur_spans(c, nv12, k, true, spans);
    }
    std::sort(spans.begin(), spans.end(), [](const BlurSpan &a, const BlurSpan &b) { return a.b < b.b; });
    const BlurSpan *far_s = nullptr, *far_t = nullptr;                                  // the farthest end so far among the scratch / the target spans
    for (const BlurSpan &v : spans) {
        if (far_s && v.b < far_s->e) {
            if (v.scratch) ffgpu_set_error("%s: scratch %d overlaps scratch %d", what, std::min(v.idx, far_s->idx), std::max(v.idx, far_s->idx));
            else ffgpu_set_error("%s: scratch %d overlaps target %d", what, far_s->idx, v.idx);
            return -1;
        }
        if (v.scratch && far_t && v.b < far_t->e) { ffgpu_set_error("%s: scratch %d overlaps target %d", what, v.idx, far_t->idx); return -1; }
        const BlurSpan *&far = v.scratch ? far_s : far_t;
        if (!far || v.e > far->e) far = &v;
    }
    return 0;
}

template <bool NV12>
static int blur_launch(const DetSource &src, const std::vector<DrawTarget> &targets, const std::vector<DrawTarget> &scratch, const BlurPlan &pl, hipStream_t s)
{
    const int n = (int)targets.size(), per = BLUR_ARG_TARGETS(NV12);
    auto blocks = [](const DrawTarget &t) { return t.p0 ? (((long long)t.w + 63) / 64) * (((long long)t.h + 63) / 64) : 0LL; };
    for (int t0 = 0; t0 < n; t0 += per) {
        const int nt = std::min(per, n - t0);
        BlurArgs<NV12> a;
        memset(&a, 0, sizeof a);
        long long most = 0;
        for (int i = 0; i < nt; i++) most = std::max(most, blocks(targets[t0 + i]));
        if (most == 0) continue;                                                       // every target of this group is skipped
        memcpy(a.classes, pl.classes, sizeof a.classes);
        a.nclasses = pl.nclasses; a.num = pl.num; a.den = pl.den; a.min_score = pl.min_score; a.outside = pl.outside; a.rec0 = t0;
        const dim3 grid((unsigned)most, (unsigned)nt);
        for (int launch = 0; launch < 2 * pl.passes; launch++) {                       // blur into the scratch, copy back, once per pass
            const bool back = launch & 1;
            const std::vector<DrawTarget> &from = back ? scratch : targets, &to = back ? targets : scratch;
            for (int i = 0; i < nt; i++) {
                const DrawTarget &f = from[t0 + i], &d = to[t0 + i];
                a.t[i] = BlurSurf{ f.p0, d.p0, src.first[t0 + i], f.w, f.h, f.pitch, d.pitch };
                if (NV12) a.uv[i] = BlurSurfUV{ f.p1, d.p1, f.pitch_uv, d.pitch_uv };
            }
            a.radius = back ? 0 : pl.radius;
            hipLaunchKernelGGL(k_blur<NV12>, grid, dim3(256), 0, s, a, src.recs, src.lists, src.stride);
            LAUNCH_OK("blur");
        }
    }
    return 0;
}

// targets[t] is blurred by record t of `src` through scratch[t]; BLUR_ARG_TARGETS targets per launch, the grid sized by the launch's largest target
int ffgpu_launch_blur(const char *what, bool nv12, const DetSource &src, const std::vector<DrawTarget> &targets, const std::vector<DrawTarget> &scratch,
                      const BlurPlan &pl, hipStream_t s)
{
    const int n = (int)targets.size();
    for (int k = 0; k < n; k++)
        if (targets[k].p0 && (((long long)targets[k].w + 63) / 64) * (((long long)targets[k].h + 63) / 64) > REDACT_MAX_BLOCKS) {
            ffgpu_set_error("%s: target %d: %d x %d is more than 2^23 blocks of 64 x 64 pixels", what, k, targets[k].w, targets[k].h);
            return -1;
        }
    if (blur_scratch_check(what, nv12, targets, scratch)) return -1;
    return nv12 ? blur_launch<true>(src, targets, scratch, pl, s) : blur_launch<false>(src, targets, scratch, pl, s);
}

template <class Frame>
static int blur_boxes_dev(const char *what, const void *d_records, const void *d_lists, int list_stride, const int *list_first,
                          const Frame *targets, const Frame *scratch, int ntargets, const ffgpu_blur_spec *spec, void *stream)
{
    const bool nv12 = std::is_same<Frame, ffgpu_nv12_frame>::value;
    if (ffgpu_no_device(what)) return -1;
    if (!targets) { ffgpu_set_error("%s: NULL targets", what); return -1; }
    if (!scratch) { ffgpu_set_error("%s: NULL scratch", what); return -1; }
    BlurPlan pl;
    if (ffgpu_blur_spec_check(what, spec, pl)) return -1;
    if (ntargets < 1 || ntargets > (1 << 24)) { ffgpu_set_error("%s: %d targets (ntargets >= 1)", what, ntargets); return -1; }
    DetSource src;
    if (ffgpu_source_dev(what, d_records, d_lists, list_stride, list_first, ntargets, src)) return -1;
    std::vector<DrawTarget> tab, stab;
    if (ffgpu_frame_table(what, FRAME_DRAW, targets, ntargets, tab) || ffgpu_frame_table(what, FRAME_SCRATCH, scratch, ntargets, stab)) return -1;
    return ffgpu_launch_blur(what, nv12, src, tab, stab, pl, (hipStream_t)stream);
}

extern "C" int ffgpu_blur_boxes_bgr_dev(const void *d_records, const void *d_lists, int list_stride, const int *list_first,
                                        const ffgpu_bgr_frame *targets, const ffgpu_bgr_frame *scratch, int ntargets, const ffgpu_blur_spec *spec, void *stream)
{
    return blur_boxes_dev("blur_boxes_bgr_dev", d_records, d_lists, list_stride, list_first, targets, scratch, ntargets, spec, stream);
}

extern "C" int ffgpu_blur_boxes_nv12_dev(const void *d_records, const void *d_lists, int list_stride, const int *list_first,
                                         const ffgpu_nv12_frame *targets, const ffgpu_nv12_frame *scratch, int ntargets, const ffgpu_blur_spec *spec, void *stream)
{
    return blur_boxes_dev("blur_boxes_nv12_dev", d_records, d_lists, list_stride, list_first, targets, scratch, ntargets, spec, stream);
}
