// ffgpu_preview.inc -- preview surfaces: frames scaled by area averaging into panes of destination surfaces, several streams composed into one wall
// (ffgpu_preview_bgr_dev / _nv12_dev, ffgpu_preview_spec_check, ffgpu_preview_rect, ffgpu_preview_grid, ffgpu_preview_tile).  The contract is in
// include/ffcnn_hip.h; the host side (resolve, the checks, the overlap test, the grid and the planes of a call) is ffgpu_preview_host.hpp.
//
// k_preview<CH>: one template for the three kinds of plane -- BGR (3 interleaved channels), the Y plane (1) and the U V plane (2, at half the size;
// the host halves the rectangles by the contract's ownership rule).  The second kernel of the tree that reads whole frames: a streaming kernel, CH
// source bytes per source sample and CH destination bytes per pane sample.  A workgroup owns a tile of 64 x 16 destination samples of one pane,
// anchored at the pane's origin, image and bars alike, and is the only writer of those bytes.  The source samples under the tile's part of the image
// are taken in CHUNKS of 16 source rows by at most 1020 row bytes: lane t loads the t-th ALIGNED dword that covers a row's bytes -- whole where it lies
// inside the frame's row, byte by byte where it sticks out of it, as motion_load does -- into LDS, so the source bytes are read once (the samples a
// tile seam cuts: once per tile).  The horizontal sums  sum_x wx(i, x) v(x, y)  are taken once per source row from those bytes and held in LDS (added
// up over the column chunks of a row); the vertical sums run over them into the lane's own accumulators, one destination column and four rows a
// lane.  The weights are closed forms of (i, sw, ow).  The division by D = sw sh is exact: where 255 D < 2^32 the sums stay in 32 bits and the
// quotient is an estimate from below (umulhi with floor((2^32 - 1) / D), one division a lane) corrected by subtraction, with the remainder's rounding;
// where not, a carry word is kept and the division is 64-bit -- chosen per pane (uniform in the workgroup).  No atomics, no scratch.  Measured: DESIGN 5.32.
struct PreviewArgs { PreviewJob j[PREVIEW_ARG_JOBS]; };
static_assert(sizeof(PreviewArgs) <= 4096 - 256, "the table travels as a kernel argument (4 KB at most, the hidden arguments included)");
#define PREVIEW_ROWS 16                               // source rows of a chunk
#define PREVIEW_SEG  1024                             // bytes of LDS per source row of a chunk: 256 dwords, one per lane
static_assert(PREVIEW_TW == 64 && PREVIEW_TH == 16 && PREVIEW_ROWS == 16 && PREVIEW_SEG == 4 * 256 && WAVE == 64, "k_preview: a lane owns column tid & 63 and rows tid >> 6 + 4 k");

// wx(i, x) of the contract (and wy with sh, oh): the length of [i s, (i + 1) s) cut with [x o, (x + 1) o)
__device__ __forceinline__ int preview_weight(int i, int x, int s, int o) { return min((i + 1) * s, (x + 1) * o) - max(i * s, x * o); }

// grid (tiles of the launch's largest pane, planes of this launch), 256 lanes.  Every load lies inside srow bytes of a source row sy .. sy + sh - 1,
// every store inside the pane.  The loops are kept rolled where the registers allow it: the kernel's time follows its code size.
template <int CH>
__global__ void __launch_bounds__(256) k_preview(PreviewArgs a)
{
    constexpr int SEGX = (PREVIEW_SEG - 4) / CH;                                      // samples of a column chunk: their bytes and a misalignment of 3 fit a row of LDS
    __shared__ unsigned s_src[PREVIEW_ROWS][PREVIEW_SEG / 4];
    __shared__ unsigned s_h[PREVIEW_ROWS][PREVIEW_TW * CH];
    const PreviewJob J = a.j[blockIdx.y];                                             // (a copy: uniform loads from the kernel argument)
    const int ntx = (J.pw + PREVIEW_TW - 1) / PREVIEW_TW, nty = (J.ph + PREVIEW_TH - 1) / PREVIEW_TH;
    if ((int)blockIdx.x >= ntx * nty) return;                                         // a smaller pane than the launch's largest (uniform)
    const int tid = threadIdx.x, tx = tid & 63, ty = tid >> 6;
    const int tx0 = (int)(blockIdx.x % ntx) * PREVIEW_TW, ty0 = (int)(blockIdx.x / ntx) * PREVIEW_TH;      // the tile in the pane
    const int ox = J.ix - J.px, oy = J.iy - J.py, sw = J.sw, sh = J.sh, ow = J.ow, oh = J.oh;
    // the image samples of the tile: [i_lo, i_hi) x [j_lo, j_hi)
    const int i_lo = max(tx0 - ox, 0), i_hi = min(tx0 + PREVIEW_TW - ox, ow), j_lo = max(ty0 - oy, 0), j_hi = min(ty0 + PREVIEW_TH - oy, oh);
    const int i = tx0 + tx - ox, j0 = ty0 - oy;                                        // the lane's image column; the tile's first row in the image
    const bool icol = i >= 0 && i < ow;
    const unsigned D = (unsigned)sw * (unsigned)sh;                                   // (at most 2^26)
    const bool wide = D > 0xffffffffu / 255u;                                         // (uniform per pane)
    // acc[k][c] = sum_y wy(j_k, y) sum_x wx(i, x) v(x, y, c) for the lane's column i and its rows j_k = j0 + ty + 4 k: 32 bits where 255 D < 2^32, else hi : lo
    unsigned acc[4][CH], hi[4][CH];
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int c = 0; c < CH; c++) acc[k][c] = hi[k][c] = 0;
    if (i_lo < i_hi && j_lo < j_hi) {                                                 // (uniform)
        const int xs0 = (i_lo * sw) / ow, xs1 = (i_hi * sw - 1) / ow, ys0 = (j_lo * sh) / oh, ys1 = (j_hi * sh - 1) / oh;   // (products below 2^26)
        const int xa = icol ? (i * sw) / ow : 0, xb = icol ? ((i + 1) * sw - 1) / ow : -1;
        int ya[4], yb[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int j = j0 + ty + 4 * k;
            const bool row = icol && j >= 0 && j < oh;
            ya[k] = row ? (j * sh) / oh : 0; yb[k] = row ? ((j + 1) * sh - 1) / oh : -1;
        }
        for (int yc = ys0; yc <= ys1; yc += PREVIEW_ROWS) {                           // (uniform)
            const int nr = min(PREVIEW_ROWS, ys1 - yc + 1);
            for (int xc = xs0; xc <= xs1; xc += SEGX) {                               // (uniform)
                const int nx = min(SEGX, xs1 - xc + 1), nb = CH * nx, b0 = CH * (J.sx + xc);
                const unsigned char *const row0 = J.src + (size_t)(J.sy + yc) * (size_t)J.spitch + b0;       // the chunk's first byte
                // the chunk's bytes: lane t, the t-th aligned dword of every row, all loads issued before the first is stored.  Row r's misalignment is
                // that of row 0 plus r times the pitch's.
                const int mis0 = (int)(reinterpret_cast<uintptr_t>(row0) & 3), pm = J.spitch & 3;
                const bool edges = b0 < 4 || b0 + nb + 4 > J.srow;                     // some dword may stick out of the frame's row (uniform)
                unsigned v[PREVIEW_ROWS];
#pragma unroll
                for (int r = 0; r < PREVIEW_ROWS; r++) {
                    const int o = b0 - ((mis0 + r * pm) & 3) + 4 * tid;
                    v[r] = 0;
                    if (r < nr && o < b0 + nb && (!edges || (o >= 0 && o + 4 <= J.srow))) v[r] = *reinterpret_cast<const unsigned *>(row0 + (size_t)r * (size_t)J.spitch + (o - b0));
                }
#pragma unroll
                for (int r = 0; r < PREVIEW_ROWS; r++) s_src[r][tid] = v[r];
                // a dword that sticks out of the frame's row (a lane at the row's first or last bytes only): byte by byte
                if (edges) {
#pragma unroll 1
                    for (int r = 0; r < nr; r++) {
                        const unsigned char *p = row0 + (size_t)r * (size_t)J.spitch;
                        const int o = b0 - ((mis0 + r * pm) & 3) + 4 * tid;
                        if (o < b0 + nb && (o < 0 || o + 4 > J.srow)) {
                            unsigned w = 0;
                            for (int b = 0; b < 4; b++) if (o + b >= 0 && o + b < J.srow) w |= (unsigned)p[o + b - b0] << (8 * b);
                            s_src[r][tid] = w;
                        }
                    }
                }
                __syncthreads();
                // the horizontal sums of the lane's column over this chunk's columns, four source rows a lane
#pragma unroll 1
                for (int r = ty; r < nr; r += 4) {
                    if (!icol) continue;
                    const int mis = (mis0 + r * pm) & 3;
                    const int lo = max(xa, xc), hx = min(xb, xc + nx - 1);
                    const unsigned char *sb = reinterpret_cast<const unsigned char *>(s_src[r]) + mis + CH * (lo - xc);
                    unsigned sum[CH];
#pragma unroll
                    for (int c = 0; c < CH; c++) sum[c] = xc == xs0 ? 0u : s_h[r][tx * CH + c];           // (the lane's own words)
#pragma unroll 1
                    for (int x = lo; x <= hx; x++, sb += CH) {
                        const unsigned w = (unsigned)preview_weight(i, x, sw, ow);
#pragma unroll
                        for (int c = 0; c < CH; c++) sum[c] += w * sb[c];
                    }
#pragma unroll
                    for (int c = 0; c < CH; c++) s_h[r][tx * CH + c] = sum[c];
                }
                __syncthreads();
            }
            // the vertical sums over this chunk's rows
#pragma unroll
            for (int k = 0; k < 4; k++) {
#pragma unroll 1
                for (int y = max(ya[k], yc); y <= min(yb[k], yc + nr - 1); y++) {
                    const unsigned w = (unsigned)preview_weight(j0 + ty + 4 * k, y, sh, oh);
#pragma unroll
                    for (int c = 0; c < CH; c++) {
                        const unsigned long long t = (unsigned long long)w * s_h[y - yc][tx * CH + c] + acc[k][c];       // (below 2^47)
                        acc[k][c] = (unsigned)t;
                        if (wide) hi[k][c] += (unsigned)(t >> 32);
                    }
                }
            }
            __syncthreads();
        }
    }
    const int pc = tx0 + tx;
    if (pc >= J.pw) return;
    const unsigned M = 0xffffffffu / D;                                               // one division a lane for the narrow sums' quotients
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int pr = ty0 + ty + 4 * k, j = pr - oy;
        if (pr >= J.ph) continue;
        const bool image = icol && j >= 0 && j < oh;
        if (!image && J.keep) continue;
        unsigned val = J.fill;
        if (image) {
            val = 0;
#pragma unroll
            for (int c = 0; c < CH; c++) {
                unsigned q;
                if (wide) q = (unsigned)((((unsigned long long)hi[k][c] << 32 | acc[k][c]) + (D >> 1)) / D);
                else {                                                                // (sum + D / 2) / D without the sum's overflow: the quotient estimated from
                    q = __umulhi(acc[k][c], M);                                       // below with M <= 2^32 / D, then corrected: exact
                    unsigned r = acc[k][c] - q * D;
                    while (r >= D) { q++; r -= D; }
                    q += r + (D >> 1) >= D ? 1u : 0u;
                }
                val |= q << (8 * c);
            }
        }
        unsigned char *p = J.dst + (size_t)(J.py + pr) * (size_t)J.dpitch + (size_t)CH * (size_t)(J.px + pc);
        if (CH == 2) *reinterpret_cast<unsigned short *>(p) = (unsigned short)val;     // (the U V plane and its pitch are 2-byte aligned)
        else
#pragma unroll
            for (int c = 0; c < CH; c++) p[c] = (unsigned char)(val >> (8 * c));
    }
}

// ---- host side
extern "C" int ffgpu_preview_spec_check(const ffgpu_preview_spec *spec) { return ffgpu_preview_spec_check_host("preview_spec_check", spec); }
extern "C" int ffgpu_preview_rect(int src_w, int src_h, int dst_w, int dst_h, const ffgpu_preview_pane *pane, const ffgpu_preview_spec *spec, int nv12, int out[8])
{
    return ffgpu_preview_rect_host("preview_rect", src_w, src_h, dst_w, dst_h, pane, spec, nv12, out);
}
extern "C" int ffgpu_preview_grid(int npanes, int cols, int dst_w, int dst_h, int gap, int nv12, ffgpu_preview_pane *out)
{
    return ffgpu_preview_grid_host("preview_grid", npanes, cols, dst_w, dst_h, gap, nv12, out);
}
extern "C" int ffgpu_preview_tile(int out[3])
{
    if (!out) { ffgpu_set_error("preview_tile: NULL out"); return -1; }
    out[0] = PREVIEW_TW; out[1] = PREVIEW_TH; out[2] = PREVIEW_ARG_JOBS;
    return 0;
}

// the planes of one kind, PREVIEW_ARG_JOBS per launch, in order on the stream
template <int CH>
static int preview_launch(const std::vector<PreviewJob> &jobs, hipStream_t s)
{
    for (size_t i0 = 0; i0 < jobs.size(); i0 += PREVIEW_ARG_JOBS) {
        const int n = (int)std::min((size_t)PREVIEW_ARG_JOBS, jobs.size() - i0);
        PreviewArgs a;
        memset(&a, 0, sizeof a);
        memcpy(a.j, jobs.data() + i0, sizeof(PreviewJob) * (size_t)n);
        hipLaunchKernelGGL(k_preview<CH>, dim3(ffgpu_preview_tiles(a.j, n), (unsigned)n), dim3(256), 0, s, a);
        LAUNCH_OK("preview");
    }
    return 0;
}

template <class Frame>
static int preview_dev(const char *what, const Frame *srcs, const Frame *dsts, const ffgpu_preview_pane *panes, int npanes, const ffgpu_preview_spec *spec, void *stream)
{
    if (ffgpu_no_device(what)) return -1;
    std::vector<PreviewJob> jobs[2];
    if (ffgpu_preview_args_check(what, srcs, dsts, panes, npanes, spec, jobs)) return -1;
    if (std::is_same<Frame, ffgpu_nv12_frame>::value) return preview_launch<1>(jobs[0], (hipStream_t)stream) || preview_launch<2>(jobs[1], (hipStream_t)stream) ? -1 : 0;
    return preview_launch<3>(jobs[0], (hipStream_t)stream);
}

extern "C" int ffgpu_preview_bgr_dev(const ffgpu_bgr_frame *srcs, const ffgpu_bgr_frame *dsts, const ffgpu_preview_pane *panes, int npanes, const ffgpu_preview_spec *spec, void *stream)
{
    return preview_dev("preview_bgr_dev", srcs, dsts, panes, npanes, spec, stream);
}
extern "C" int ffgpu_preview_nv12_dev(const ffgpu_nv12_frame *srcs, const ffgpu_nv12_frame *dsts, const ffgpu_preview_pane *panes, int npanes, const ffgpu_preview_spec *spec, void *stream)
{
    return preview_dev("preview_nv12_dev", srcs, dsts, panes, npanes, spec, stream);
}
