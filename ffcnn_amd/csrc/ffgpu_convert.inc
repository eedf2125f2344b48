// ffgpu_convert.inc -- convert surfaces: I420, YV12, NV12, NV21, YUY2, UYVY, P010, RGB, BGR, RGBA, BGRA and GRAY8 frames into BGR and NV12 frames
// (ffgpu_convert_check, ffgpu_convert_tile, ffgpu_convert_bgr_dev / _nv12_dev).  The contract is in include/ffcnn_hip.h; the host side (a surface's
// check, the argument checks and the jobs of a call) is ffgpu_convert_host.hpp.
//
// k_convert<SRC, DST>: one template, instantiated per source class (CONVERT_*: packed RGB, gray, planar 4:2:0, pair-plane 4:2:0, 16-bit pair-plane
// 4:2:0, packed 4:2:2) and destination (BGR, NV12).  The fourth kernel of the tree that reads whole frames and the first that streams them: a lane
// owns a BLOCK of 4 destination pixels by 2 rows anchored at the frame's origin -- so the block's two chroma samples per plane are read or produced
// once, by the lane that owns them --, a wave 256 consecutive pixels of a row pair, a workgroup a tile of 256 x 8 pixels of one job, and it is the
// only writer of those bytes.  A block moves in three steps: its RAW dwords loaded (cv_load), decoded into samples and converted (registers only),
// the destination's raw dwords stored (cv_store).  The two forms of the contract differ in the first and the last step alone, so they give the same
// bytes by construction:
//   ALIGNED  (the job's every address and pitch is a multiple of 4: the host's choice, uniform per workgroup; whole blocks only)  a block's bytes
//            start at a multiple of 4 in every plane, so they are loaded as whole dwords -- a dword of Y per row, a dword of pair-plane chroma or two
//            16-bit values of planar chroma, 3 or 4 dwords of packed RGB per row, 2 of YUY2, 2 of P010 luma --, all of them issued before the first
//            result is stored, and stored as whole dwords past the caches (non-temporal): 3 of BGR per row, or one of Y per row and one of U V.
//   GENERAL  everything else, the ragged last block of a row and the odd last row of an aligned job included: the same raw dwords gathered byte by
//            byte (aligned 16-bit values where the plane holds pairs or 16-bit samples), bytes outside the frame zero and never stored.
// There is no LDS staging of unaligned rows (DESIGN 5.34).  Integer arithmetic: __mul24 products, min / max clamps (v_med3_i32), byte shuffles through
// v_perm_b32.  No atomics, no scratch.
struct ConvertArgs { ConvertJob j[CONVERT_ARG_JOBS]; };
static_assert(sizeof(ConvertArgs) <= 4096 - 256, "the table travels as a kernel argument (4 KB at most, the hidden arguments included)");
static_assert(CONVERT_TW == 256 && CONVERT_TH == 8 && WAVE == 64, "k_convert: a lane owns columns 4 (tid & 63) .. + 3 and rows 2 (tid >> 6), + 1 of the tile");
__constant__ int c_rgb2yuv[4][10] = FFGPU_RGB2YUV_MATRICES;
typedef const FFG unsigned char *cv_src;
typedef FFG unsigned char *cv_dst;

// byte k of the result is byte sel[k] of { hi : lo } (0..3: lo, 4..7: hi, 0x0c: zero)
__device__ __forceinline__ unsigned cv_perm(unsigned hi, unsigned lo, unsigned sel) { return __builtin_amdgcn_perm(hi, lo, sel); }
__device__ __forceinline__ int cv_byte(unsigned v, int k) { return (int)(v >> (8 * k) & 255u); }

// K raw dwords at p.  FAST: whole (p is a multiple of 4 and the 4 K bytes lie inside the row).  Else the first n UNITS of them -- bytes, or 16-bit
// values at even addresses (U16) -- one by one and the rest zero: no load reaches behind unit n - 1.
template <int K, bool FAST, bool U16 = false>
__device__ __forceinline__ void cv_load(cv_src p, int n, unsigned *d)
{
#pragma unroll
    for (int k = 0; k < K; k++) d[k] = FAST ? *reinterpret_cast<const FFG unsigned *>(p + 4 * k) : 0u;
    if constexpr (!FAST) {
        if constexpr (U16) {
#pragma unroll
            for (int u = 0; u < 2 * K; u++) if (u < n) d[u >> 1] |= (unsigned)*reinterpret_cast<const FFG unsigned short *>(p + 2 * u) << (16 * (u & 1));
        } else {
#pragma unroll
            for (int u = 0; u < 4 * K; u++) if (u < n) d[u >> 2] |= (unsigned)p[u] << (8 * (u & 3));
        }
    }
}
// the same for a destination: whole dwords past the caches, or the first n units of them
template <int K, bool FAST, bool U16 = false>
__device__ __forceinline__ void cv_store(cv_dst p, int n, const unsigned *d)
{
    if constexpr (FAST) {
#pragma unroll
        for (int k = 0; k < K; k++) __builtin_nontemporal_store(d[k], reinterpret_cast<FFG unsigned *>(p + 4 * k));
    } else if constexpr (U16) {
#pragma unroll
        for (int u = 0; u < 2 * K; u++) if (u < n) *reinterpret_cast<FFG unsigned short *>(p + 2 * u) = (unsigned short)(d[u >> 1] >> (16 * (u & 1)));
    } else {
#pragma unroll
        for (int u = 0; u < 4 * K; u++) if (u < n) p[u] = (unsigned char)(d[u >> 2] >> (8 * (u & 3)));
    }
}

// A block's raw dwords: a[r] of plane 0's row y0 + r (r < ny; the rest zero), c of the chroma row y0 >> 1 (4:2:0): planar c[0] = U U, c[1] = V V;
// pair plane c[0] = U V U V; 16-bit pair plane c[0] = U V, c[1] = U V.  Every load lies inside columns x0 .. x0 + nx - 1 (their chroma samples
// x0 / 2 .. x0 / 2 + ncx - 1, their 4:2:2 groups likewise) of rows y0 .. y0 + ny - 1: inside the surface.
struct CvRaw { unsigned a[2][4], c[2]; };
template <int SRC, bool FAST>
__device__ __forceinline__ void cv_load_block(const ConvertJob &J, int x0, int y0, int nx, int ny, CvRaw &R)
{
    const int ncx = (nx + 1) >> 1;
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const cv_src p = (cv_src)J.s[0] + (size_t)(y0 + r) * (size_t)J.sp[0];
        const int m = r < ny ? 1 : 0;                                                 // (an odd last row: no unit of row y0 + 1 is loaded)
        R.a[r][0] = R.a[r][1] = R.a[r][2] = R.a[r][3] = 0;
        if constexpr (SRC == CONVERT_RGB) {
            if (J.sel & CONVERT_BPP4) cv_load<4, FAST>(p + 4 * x0, m * 4 * nx, R.a[r]);
            else cv_load<3, FAST>(p + 3 * x0, m * 3 * nx, R.a[r]);
        } else if constexpr (SRC == CONVERT_PAIR16) cv_load<2, FAST, true>(p + 2 * x0, m * nx, R.a[r]);
        else if constexpr (SRC == CONVERT_PACKED422) cv_load<2, FAST>(p + 2 * x0, m * 4 * ncx, R.a[r]);
        else cv_load<1, FAST>(p + x0, m * nx, R.a[r]);
    }
    R.c[0] = R.c[1] = 0;
    const size_t cy = (size_t)(y0 >> 1);
    if constexpr (SRC == CONVERT_PLANAR) {
#pragma unroll
        for (int n = 0; n < 2; n++) {
            const cv_src p = (cv_src)J.s[1 + n] + cy * (size_t)J.sp[1 + n] + (x0 >> 1);
            if constexpr (FAST) R.c[n] = *reinterpret_cast<const FFG unsigned short *>(p);    // (x0 / 2 is even)
            else cv_load<1, false>(p, ncx, &R.c[n]);
        }
    } else if constexpr (SRC == CONVERT_PAIR) cv_load<1, FAST, true>((cv_src)J.s[1] + cy * (size_t)J.sp[1] + x0, ncx, R.c);
    else if constexpr (SRC == CONVERT_PAIR16) cv_load<2, FAST, true>((cv_src)J.s[1] + cy * (size_t)J.sp[1] + 2 * x0, 2 * ncx, R.c);
}

// A block's samples: RGB sources px[r][i] = B | G << 8 | R << 16; every other class y[r] = four Y bytes and u[r], v[r] = the two chroma samples of
// row r's pixels in bytes 0 and 1 (4:2:0: both rows the same).
struct CvBlock { unsigned px[2][4], y[2], u[2], v[2]; };
__device__ __forceinline__ unsigned cv_r10(unsigned s) { return min(((s >> 6) + 2u) >> 2, 255u); }      // the reduction of a P010 sample
template <int SRC>
__device__ __forceinline__ void cv_decode(const ConvertJob &J, const CvRaw &R, CvBlock &B)
{
    const bool swap = (J.sel & CONVERT_SWAP) != 0;
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const unsigned *a = R.a[r];
        B.y[r] = a[0]; B.u[r] = R.c[0]; B.v[r] = R.c[1];                             // (gray, planar)
        if constexpr (SRC == CONVERT_RGB) {
            const unsigned order = swap ? 0x0c000102u : 0x0c020100u;                  // R G B (A) or B G R (A) to B G R 0
            const bool bpp4 = (J.sel & CONVERT_BPP4) != 0;
            B.px[r][0] = cv_perm(0, a[0], order);
            B.px[r][1] = cv_perm(0, bpp4 ? a[1] : cv_perm(a[1], a[0], 0x0c050403u), order);
            B.px[r][2] = cv_perm(0, bpp4 ? a[2] : cv_perm(a[2], a[1], 0x0c040302u), order);
            B.px[r][3] = cv_perm(0, bpp4 ? a[3] : a[2] >> 8, order);
        } else if constexpr (SRC == CONVERT_PAIR) {
            B.u[r] = cv_perm(0, R.c[0], swap ? 0x0c0c0301u : 0x0c0c0200u); B.v[r] = cv_perm(0, R.c[0], swap ? 0x0c0c0200u : 0x0c0c0301u);
        } else if constexpr (SRC == CONVERT_PAIR16) {
            B.y[r] = cv_r10(a[0] & 0xffffu) | cv_r10(a[0] >> 16) << 8 | cv_r10(a[1] & 0xffffu) << 16 | cv_r10(a[1] >> 16) << 24;
            B.u[r] = cv_r10(R.c[0] & 0xffffu) | cv_r10(R.c[1] & 0xffffu) << 8; B.v[r] = cv_r10(R.c[0] >> 16) | cv_r10(R.c[1] >> 16) << 8;
        } else if constexpr (SRC == CONVERT_PACKED422) {                              // Y0 U Y1 V | Y2 U Y3 V, or U Y0 V Y1 | U Y2 V Y3
            B.y[r] = cv_perm(a[1], a[0], swap ? 0x07050301u : 0x06040200u);
            B.u[r] = cv_perm(a[1], a[0], swap ? 0x0c0c0400u : 0x0c0c0501u); B.v[r] = cv_perm(a[1], a[0], swap ? 0x0c0c0602u : 0x0c0c0703u);
        }
    }
}

// the block's BGR bytes: three raw dwords a row
template <int SRC>
__device__ __forceinline__ void cv_to_bgr(const ConvertJob &J, const CvBlock &B, unsigned (&o)[2][3])
{
    const YuvMat m = yuv_mat(J.fmt);
#pragma unroll
    for (int r = 0; r < 2; r++) {
        unsigned px[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if constexpr (SRC == CONVERT_RGB) px[i] = B.px[r][i];
            else if constexpr (SRC == CONVERT_GRAY) px[i] = (unsigned)cv_byte(B.y[r], i) * 0x010101u;
            else px[i] = nv12_to_bgr(cv_byte(B.y[r], i), cv_byte(B.u[r], i >> 1), cv_byte(B.v[r], i >> 1), m);
        }
        o[r][0] = cv_perm(px[1], px[0], 0x04020100u); o[r][1] = cv_perm(px[2], px[1], 0x05040201u); o[r][2] = cv_perm(px[3], px[2], 0x06050402u);
    }
}

// the block's NV12 bytes: a raw dword of Y a row and one of U V U V.  nx, ny: the block's pixels inside the frame (an RGB source's means)
template <int SRC>
__device__ __forceinline__ void cv_to_nv12(const ConvertJob &J, const CvBlock &B, int nx, int ny, unsigned (&oy)[2], unsigned &ouv)
{
    if constexpr (SRC == CONVERT_RGB) {
        const int *m = c_rgb2yuv[(J.fmt - 1) & 3];                                    // (every product below fits 24 signed bits: at most 183 x 255)
        const int yoff = m[0], yr = m[1], yg = m[2], yb = m[3], ur = m[4], ug = m[5], ub = m[6], vr = m[7], vg = m[8], vb = m[9];
        int sb[2] = { 0, 0 }, sg[2] = { 0, 0 }, sr[2] = { 0, 0 };                     // (pixels outside the frame are zero: they add nothing)
#pragma unroll
        for (int r = 0; r < 2; r++) {
            oy[r] = 0;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int b = cv_byte(B.px[r][i], 0), g = cv_byte(B.px[r][i], 1), rr = cv_byte(B.px[r][i], 2);
                oy[r] |= (unsigned)clamp255(((__mul24(yr, rr) + __mul24(yg, g) + __mul24(yb, b) + 128) >> 8) + yoff) << (8 * i);
                sb[i >> 1] += b; sg[i >> 1] += g; sr[i >> 1] += rr;
            }
        }
        ouv = 0;
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int sh = (nx - 2 * k >= 2 ? 1 : 0) + (ny == 2 ? 1 : 0), half = (1 << sh) >> 1;      // n = 1 << sh pixels: 1, 2 or 4
            const int b = (sb[k] + half) >> sh, g = (sg[k] + half) >> sh, rr = (sr[k] + half) >> sh;
            const int u = clamp255(((__mul24(ur, rr) + __mul24(ug, g) + __mul24(ub, b) + 128) >> 8) + 128);
            const int v = clamp255(((__mul24(vr, rr) + __mul24(vg, g) + __mul24(vb, b) + 128) >> 8) + 128);
            ouv |= ((unsigned)u | (unsigned)v << 8) << (16 * k);
        }
    } else {
        oy[0] = B.y[0]; oy[1] = B.y[1];
        unsigned u = B.u[0], v = B.v[0];
        if constexpr (SRC == CONVERT_PACKED422) {
            auto mean = [](unsigned c0, unsigned c1) {                               // of the two rows' samples, rounded up, per sample
                return (unsigned)((cv_byte(c0, 0) + cv_byte(c1, 0) + 1) >> 1) | (unsigned)((cv_byte(c0, 1) + cv_byte(c1, 1) + 1) >> 1) << 8;
            };
            if (ny == 2) { u = mean(u, B.u[1]); v = mean(v, B.v[1]); }
        }
        ouv = SRC == CONVERT_GRAY ? 0x80808080u : cv_perm(v, u, 0x05010400u);        // U0 V0 U1 V1
    }
}

// grid (tiles of the launch's largest job, jobs of this launch), 256 lanes
template <int SRC, int DST>
__global__ void __launch_bounds__(256) k_convert(ConvertArgs a)
{
    const ConvertJob J = a.j[blockIdx.y];                                             // (a copy: uniform loads from the kernel argument)
    const int ntx = (J.w + CONVERT_TW - 1) / CONVERT_TW, nty = (J.h + CONVERT_TH - 1) / CONVERT_TH;
    if ((int)blockIdx.x >= ntx * nty) return;                                         // a smaller job than the launch's largest (uniform)
    const int tid = threadIdx.x;
    const int x0 = (int)(blockIdx.x % ntx) * CONVERT_TW + 4 * (tid & 63), y0 = (int)(blockIdx.x / ntx) * CONVERT_TH + 2 * (tid >> 6);
    if (x0 >= J.w || y0 >= J.h) return;
    const int nx = min(4, J.w - x0), ny = min(2, J.h - y0), ncx = (nx + 1) >> 1;      // the block's pixels and chroma samples inside the frame
    const bool fast = J.aligned && nx == 4 && ny == 2;
    CvRaw R;
    if (fast) cv_load_block<SRC, true>(J, x0, y0, nx, ny, R);
    else cv_load_block<SRC, false>(J, x0, y0, nx, ny, R);
    CvBlock B;
    cv_decode<SRC>(J, R, B);
    if constexpr (DST == 0) {
        unsigned o[2][3];
        cv_to_bgr<SRC>(J, B, o);
        const cv_dst p = (cv_dst)J.d[0] + (size_t)y0 * (size_t)J.dp[0] + 3 * x0;      // rows y0 .. y0 + ny - 1, bytes 3 x0 .. 3 (x0 + nx) - 1 of them
        if (fast) { cv_store<3, true>(p, 0, o[0]); cv_store<3, true>(p + J.dp[0], 0, o[1]); }
        else {
            cv_store<3, false>(p, 3 * nx, o[0]);
            if (ny == 2) cv_store<3, false>(p + J.dp[0], 3 * nx, o[1]);
        }
    } else {
        unsigned oy[2], ouv;
        cv_to_nv12<SRC>(J, B, nx, ny, oy, ouv);
        const cv_dst p = (cv_dst)J.d[0] + (size_t)y0 * (size_t)J.dp[0] + x0;
        const cv_dst q = (cv_dst)J.d[1] + (size_t)(y0 >> 1) * (size_t)J.dp[1] + x0;   // pairs x0 / 2 .. x0 / 2 + ncx - 1 of chroma row y0 / 2: this block's alone
        if (fast) { cv_store<1, true>(p, 0, &oy[0]); cv_store<1, true>(p + J.dp[0], 0, &oy[1]); cv_store<1, true>(q, 0, &ouv); }
        else {
            cv_store<1, false>(p, nx, &oy[0]);
            if (ny == 2) cv_store<1, false>(p + J.dp[0], nx, &oy[1]);
            cv_store<1, false, true>(q, ncx, &ouv);
        }
    }
}

// ---- host side
extern "C" int ffgpu_convert_check(const ffgpu_surface *src, int dst_nv12, int dst_w, int dst_h)
{
    return ffgpu_convert_check_host(dst_nv12 ? "convert_check (nv12)" : "convert_check (bgr)", src, dst_w, dst_h);
}
extern "C" int ffgpu_convert_tile(int out[3])
{
    if (!out) { ffgpu_set_error("convert_tile: NULL out"); return -1; }
    out[0] = CONVERT_TW; out[1] = CONVERT_TH; out[2] = CONVERT_ARG_JOBS;
    return 0;
}

// the jobs of one source class, CONVERT_ARG_JOBS per launch, in order on the stream
template <int SRC, int DST>
static int convert_launch(const std::vector<ConvertJob> &jobs, hipStream_t s)
{
    return launch_jobs<ConvertArgs, CONVERT_ARG_JOBS>("convert", jobs, ffgpu_convert_tiles, [](ConvertArgs &) {}, k_convert<SRC, DST>, s);
}

template <int DST, class Frame>
static int convert_dev(const char *what, const ffgpu_surface *srcs, const Frame *dsts, int njobs, void *stream)
{
    if (ffgpu_no_device(what)) return -1;
    std::vector<ConvertJob> jobs[CONVERT_NSRC];
    if (ffgpu_convert_args_check(what, srcs, dsts, njobs, jobs)) return -1;
    const hipStream_t s = (hipStream_t)stream;
    return convert_launch<CONVERT_RGB, DST>(jobs[CONVERT_RGB], s) || convert_launch<CONVERT_GRAY, DST>(jobs[CONVERT_GRAY], s) ||
           convert_launch<CONVERT_PLANAR, DST>(jobs[CONVERT_PLANAR], s) || convert_launch<CONVERT_PAIR, DST>(jobs[CONVERT_PAIR], s) ||
           convert_launch<CONVERT_PAIR16, DST>(jobs[CONVERT_PAIR16], s) || convert_launch<CONVERT_PACKED422, DST>(jobs[CONVERT_PACKED422], s) ? -1 : 0;
}

extern "C" int ffgpu_convert_bgr_dev(const ffgpu_surface *srcs, const ffgpu_bgr_frame *dsts, int njobs, void *stream)
{
    return convert_dev<0>("convert_bgr_dev", srcs, dsts, njobs, stream);
}
extern "C" int ffgpu_convert_nv12_dev(const ffgpu_surface *srcs, const ffgpu_nv12_frame *dsts, int njobs, void *stream)
{
    return convert_dev<1>("convert_nv12_dev", srcs, dsts, njobs, stream);
}
