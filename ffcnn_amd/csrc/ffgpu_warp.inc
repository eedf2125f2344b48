// ffgpu_warp.inc -- warp surfaces: frames dewarped, rotated and rectified through a coarse mesh of source positions (ffgpu_warp_bgr_dev / _nv12_dev,
// ffgpu_warp_spec_check, ffgpu_warp_mesh_size, ffgpu_warp_mesh_orient, ffgpu_warp_mesh_homography, ffgpu_warp_mesh_lens, ffgpu_warp_point,
// ffgpu_warp_tile).  The contract is in include/ffcnn_hip.h; the host side (the builders, the checks and the planes of a call) is ffgpu_warp_host.hpp.
//
// k_warp<CH>: one template for the three kinds of plane -- BGR (3 interleaved channels), the Y plane (1) and the U V plane (2, at half the size, its
// positions taken from the mesh at luma pixel (2 i, 2 j) and halved).  The third kernel of the tree that reads whole frames and the first whose reads
// are a gather.  A workgroup owns a tile of 64 x 16 destination samples of one job and is the only writer of those bytes; a lane owns one column and
// FOUR CONSECUTIVE rows of it.  Those four rows lie in one cell of the mesh (cells are 8 or more, the group starts at a multiple of 4, and on the U V
// plane of 8 in luma rows), so the lane loads its cell's four points once, interpolates along the cell's top and bottom edge once, and steps down
// its rows by adding the difference: the contract's sum S in exact 64-bit integers, four multiplications a coordinate and lane.
// Two forms of the read, the same bytes from both; BGR planes choose per workgroup (uniform), the Y and the U V plane are always read directly (their
// tiles' boxes are a third the bytes and the staging's barriers cost more than they save: measured, DESIGN 5.33):
//   STAGED  the tile's taps lie inside the bounding box of the mesh points of the cells the tile touches, plus one sample (the interpolation stays
//           inside their hull, and rounding a value between two integers stays between them).  Where that box, clipped to the plane, fits
//           WARP_LDS_BYTES, the workgroup loads it once: a wave a row, a lane an ALIGNED dword of it -- whole where the dword lies inside the plane's
//           row, byte by byte where it sticks out of it, as motion_load does -- and samples from LDS: the two neighbouring samples of a tap row come
//           out of two or three aligned LDS dwords by v_alignbyte.
//   DIRECT  every lane loads its taps' bytes from global memory: the fallback for footprints over the budget (a minifying mesh, wild points).
// A tap's address is always that of the CLAMPED coordinate, so every load lies inside the source plane whatever the mesh holds; under FILL the loaded
// value is then replaced by the fill's where the tap was outside.  No atomics, no scratch.  Measured: DESIGN 5.33.
struct WarpArgs { WarpJob j[WARP_ARG_JOBS]; unsigned fill; int nearest, clamp, pad_; };
static_assert(sizeof(WarpArgs) <= 4096 - 256, "the table travels as a kernel argument (4 KB at most, the hidden arguments included)");
static_assert(WARP_TW == 64 && WARP_TH == 16 && WAVE == 64, "k_warp: a lane owns column tid & 63 and rows 4 (tid >> 6) .. + 3");
static_assert((WARP_TW * 2 / 8 + 1) * (WARP_TH * 2 / 8 + 1) <= 256, "k_warp: a lane a mesh point of the tile's cells, the U V plane's 17 x 5 at cells of 8 included");
typedef const FFG unsigned char *warp_src;

// Where a workgroup's taps come from: the staged box [bx0, ..] x [by0, ..] in LDS (row r at dword r stride, its bytes behind the misalignment of the
// row's first byte in global memory), or the plane in global memory.
struct WarpTaps {
    const unsigned *lds;          // NULL: direct
    warp_src src;
    int spitch, sw, sh;
    int bx0, by0, stride, mis0, pm;
};

// the samples (xa, y) and (xb, y), xb == xa or xa + 1, both inside the plane (and inside the box where one is staged): channel c in bits 8 c .. 8 c + 7
template <int CH>
__device__ __forceinline__ void warp_fetch(const WarpTaps &t, int y, int xa, int xb, unsigned &pa, unsigned &pb)
{
    constexpr unsigned MASK = CH == 3 ? 0xffffffu : CH == 2 ? 0xffffu : 0xffu;
    if (t.lds) {
        const int r = y - t.by0, o = ((t.mis0 + r * t.pm) & 3) + CH * (xa - t.bx0);
        const unsigned *w = t.lds + r * t.stride + (o >> 2);
        const unsigned lo = __builtin_amdgcn_alignbyte(w[1], w[0], (unsigned)o & 3u);            // bytes o .. o + 3 (the dwords behind a row's last byte: padding, unused)
        pa = lo & MASK;
        pb = CH == 3 ? lo >> 24 | (__builtin_amdgcn_alignbyte(w[2], w[1], (unsigned)o & 3u) & 0xffffu) << 8 : (lo >> (8 * CH)) & MASK;
        pb = xb == xa ? pa : pb;
        return;
    }
    const warp_src p = t.src + (size_t)y * (size_t)t.spitch;
    pa = pb = 0;
#pragma unroll
    for (int c = 0; c < CH; c++) { pa |= (unsigned)p[CH * xa + c] << (8 * c); pb |= (unsigned)p[CH * xb + c] << (8 * c); }
}

// one destination sample from its position (x5, y5) in 1 / 32 source samples: channel c in bits 8 c .. 8 c + 7
template <int CH>
__device__ __forceinline__ unsigned warp_sample(const WarpTaps &t, int x5, int y5, bool nearest, bool clamp, unsigned fill)
{
    const int sw = t.sw, sh = t.sh;
    if (nearest) {
        const int x = (x5 + 16) >> 5, y = (y5 + 16) >> 5, xc = min(max(x, 0), sw - 1), yc = min(max(y, 0), sh - 1);
        unsigned v, unused;
        warp_fetch<CH>(t, yc, xc, xc, v, unused);
        return clamp || (x == xc && y == yc) ? v : fill;
    }
    const int x0 = x5 >> 5, fx = x5 & 31, y0 = y5 >> 5, fy = y5 & 31;
    const int xa = min(max(x0, 0), sw - 1), xb = min(max(x0 + 1, 0), sw - 1), ya = min(max(y0, 0), sh - 1), yb = min(max(y0 + 1, 0), sh - 1);
    const bool ixa = clamp || xa == x0, ixb = clamp || xb == x0 + 1, iya = clamp || ya == y0, iyb = clamp || yb == y0 + 1;
    unsigned p00, p10, p01, p11;
    warp_fetch<CH>(t, ya, xa, xb, p00, p10);
    warp_fetch<CH>(t, yb, xa, xb, p01, p11);
    p00 = ixa && iya ? p00 : fill; p10 = ixb && iya ? p10 : fill; p01 = ixa && iyb ? p01 : fill; p11 = ixb && iyb ? p11 : fill;
    unsigned out = 0;
#pragma unroll
    for (int c = 0; c < CH; c++) {
        const int v00 = (int)(p00 >> (8 * c) & 255u), v10 = (int)(p10 >> (8 * c) & 255u), v01 = (int)(p01 >> (8 * c) & 255u), v11 = (int)(p11 >> (8 * c) & 255u);
        out |= (unsigned)(((32 - fy) * ((32 - fx) * v00 + fx * v10) + fy * ((32 - fx) * v01 + fx * v11) + 512) >> 10) << (8 * c);
    }
    return out;
}

// the first and the last tap coordinate of positions between the mesh values lo and hi (1 / 256 luma pixel), clamped to 0 .. n - 1
__device__ __forceinline__ void warp_span(int lo, int hi, int half, int n, int &t0, int &t1)
{
    const int a = (int)(((long long)lo + (4 << half)) >> (3 + half)) >> 5, b = ((int)(((long long)hi + (4 << half)) >> (3 + half)) >> 5) + 1;    // (NEAREST's tap lies between them)
    t0 = min(max(a, 0), n - 1); t1 = min(max(b, 0), n - 1);
}

// grid (tiles of the launch's largest job, jobs of this launch), 256 lanes.  Every load lies inside the sw x sh samples of the source plane and the
// mh x mw points of the mesh, every store inside the dw x dh samples of the destination plane.
template <int CH>
__global__ void __launch_bounds__(256) k_warp(WarpArgs a)
{
    const WarpJob J = a.j[blockIdx.y];                                                // (a copy: uniform loads from the kernel argument)
    const int ntx = (J.dw + WARP_TW - 1) / WARP_TW, nty = (J.dh + WARP_TH - 1) / WARP_TH;
    if ((int)blockIdx.x >= ntx * nty) return;                                         // a smaller job than the launch's largest (uniform)
    const int tid = threadIdx.x;
    const int tx0 = (int)(blockIdx.x % ntx) * WARP_TW, ty0 = (int)(blockIdx.x / ntx) * WARP_TH;
    const int i = tx0 + (tid & 63), j0 = ty0 + 4 * (tid >> 6);
    const int s = J.shift & 0xff, half = J.shift >> 8, c = 1 << s;
    const FFG long long *const mesh = (const FFG long long *)J.xy;                    // (a point is 8 aligned bytes: x low, y high)

    // BGR only (WARP_STAGED_CH; measured, DESIGN 5.33: the one- and two-channel planes are faster read directly).  The bounding box of the mesh points of
    // the cells the tile touches: a lane a point, a wave's minima and maxima by shuffles, the four waves' through LDS
    WarpTaps t;
    t.lds = nullptr; t.src = (warp_src)J.src; t.spitch = J.spitch; t.sw = J.sw; t.sh = J.sh; t.bx0 = t.by0 = t.stride = t.mis0 = t.pm = 0;
    if constexpr (CH == WARP_STAGED_CH) {
        __shared__ int s_red[4][4];
        __shared__ unsigned s_src[WARP_LDS_BYTES / 4 + 2];                              // (+ 2: warp_fetch reads up to two dwords behind a row's last byte)
        const int ci0 = (tx0 << half) >> s, npx = ((min(tx0 + WARP_TW, J.dw) - 1) << half >> s) + 2 - ci0;
        const int cj0 = (ty0 << half) >> s, npy = ((min(ty0 + WARP_TH, J.dh) - 1) << half >> s) + 2 - cj0;
        int mnx = 0x7fffffff, mxx = -0x7fffffff - 1, mny = 0x7fffffff, mxy = -0x7fffffff - 1;
        if (tid < npx * npy) {
            const int py = tid / npx, px = tid - py * npx;
            const long long q = mesh[(size_t)(cj0 + py) * (size_t)J.mw + (size_t)(ci0 + px)];
            mnx = mxx = (int)q; mny = mxy = (int)(q >> 32);
        }
#pragma unroll
        for (int o = 32; o; o >>= 1) {
            mnx = min(mnx, __shfl_xor(mnx, o)); mxx = max(mxx, __shfl_xor(mxx, o)); mny = min(mny, __shfl_xor(mny, o)); mxy = max(mxy, __shfl_xor(mxy, o));
        }
        if ((tid & 63) == 0) { s_red[tid >> 6][0] = mnx; s_red[tid >> 6][1] = mxx; s_red[tid >> 6][2] = mny; s_red[tid >> 6][3] = mxy; }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < 4; w++) { mnx = min(mnx, s_red[w][0]); mxx = max(mxx, s_red[w][1]); mny = min(mny, s_red[w][2]); mxy = max(mxy, s_red[w][3]); }
        int bx0, bx1, by0, by1;
        warp_span(mnx, mxx, half, J.sw, bx0, bx1);
        warp_span(mny, mxy, half, J.sh, by0, by1);
        const int nb = CH * (bx1 - bx0 + 1), nr = by1 - by0 + 1, stride = (nb + 6) >> 2;      // a row of LDS: its bytes behind a misalignment of up to 3
        if (nr * stride <= WARP_LDS_BYTES / 4) {                                       // (uniform; at most 8192 x 6146)
            const int b0 = CH * bx0, rowbytes = CH * J.sw;
            const warp_src row0 = t.src + (size_t)by0 * (size_t)J.spitch + (size_t)b0;
            const int mis0 = (int)(reinterpret_cast<uintptr_t>(row0) & 3), pm = J.spitch & 3;
            for (int r = tid >> 6; r < nr; r += 4) {                                   // a wave a row (uniform in the wave)
                const int mis = (mis0 + r * pm) & 3, nd = (mis + nb + 3) >> 2;            // (nd <= stride)
                const warp_src rp = row0 + (size_t)r * (size_t)J.spitch;
                for (int q = tid & 63; q < nd; q += 64) {
                    const int fo = 4 * q - mis, ro = b0 + fo;                          // the dword's first byte from rp (4-byte aligned), and in the plane's row
                    unsigned w = 0;
                    if (ro >= 0 && ro + 4 <= rowbytes) w = *reinterpret_cast<const FFG unsigned *>(rp + fo);
                    else
                        for (int b = 0; b < 4; b++) if (ro + b >= 0 && ro + b < rowbytes) w |= (unsigned)rp[fo + b] << (8 * b);
                    s_src[r * stride + q] = w;
                }
            }
            t.lds = s_src; t.bx0 = bx0; t.by0 = by0; t.stride = stride; t.mis0 = mis0; t.pm = pm;
            __syncthreads();
        }
    }
    if (i >= J.dw || j0 >= J.dh) return;
    const int li = i << half, lj = j0 << half;                                        // the luma pixel whose mesh position the sample takes
    const int ca = li & (c - 1), cb = lj & (c - 1);                                   // (cb + (3 << half) < c: the lane's rows stay in this cell)
    const FFG long long *const m = mesh + ((size_t)(lj >> s) * (size_t)J.mw + (size_t)(li >> s));
    const long long q00 = m[0], q10 = m[1], q01 = m[J.mw], q11 = m[J.mw + 1];
    const int2 p00 = { (int)q00, (int)(q00 >> 32) }, p10 = { (int)q10, (int)(q10 >> 32) }, p01 = { (int)q01, (int)(q01 >> 32) }, p11 = { (int)q11, (int)(q11 >> 32) };
    // along the cell's top and bottom edge (below 2^38), then S(b) = (c - b) top + b bottom = c top + b (bottom - top), a step of 1 << half rows down
    const long long tx = (long long)(c - ca) * p00.x + (long long)ca * p10.x, ty = (long long)(c - ca) * p00.y + (long long)ca * p10.y;
    const long long dx = (long long)(c - ca) * p01.x + (long long)ca * p11.x - tx, dy = (long long)(c - ca) * p01.y + (long long)ca * p11.y - ty;
    long long Sx = tx * c + dx * cb + (1LL << (2 * s - 1)), Sy = ty * c + dy * cb + (1LL << (2 * s - 1));    // (the rounding term of X8 included)
    FFG unsigned char *p = (FFG unsigned char *)J.dst + (size_t)j0 * (size_t)J.dpitch + (size_t)(CH * i);
    const bool nearest = a.nearest != 0, clamp = a.clamp != 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (j0 + k < J.dh) {
            const long long X8 = Sx >> (2 * s), Y8 = Sy >> (2 * s);                   // (arithmetic shifts)
            const int x5 = (int)((X8 + (4 << half)) >> (3 + half)), y5 = (int)((Y8 + (4 << half)) >> (3 + half));
            const unsigned v = warp_sample<CH>(t, x5, y5, nearest, clamp, a.fill);
            if (CH == 2) *reinterpret_cast<FFG unsigned short *>(p) = (unsigned short)v;    // (the U V plane and its pitch are 2-byte aligned)
            else
#pragma unroll
                for (int ch = 0; ch < CH; ch++) p[ch] = (unsigned char)(v >> (8 * ch));
        }
        Sx += dx << half; Sy += dy << half; p += J.dpitch;
    }
}

// ---- host side
extern "C" int ffgpu_warp_spec_check(const ffgpu_warp_spec *spec) { return ffgpu_warp_spec_check_host("warp_spec_check", spec); }
extern "C" int ffgpu_warp_mesh_size(int dst_w, int dst_h, int cell, int out[2]) { return ffgpu_warp_mesh_size_host("warp_mesh_size", dst_w, dst_h, cell, out); }
extern "C" int ffgpu_warp_mesh_orient(int src_w, int src_h, int orient, int cell, int out_dst_wh[2], int *xy)
{
    return ffgpu_warp_mesh_orient_host("warp_mesh_orient", src_w, src_h, orient, cell, out_dst_wh, xy);
}
extern "C" int ffgpu_warp_mesh_homography(int dst_w, int dst_h, int cell, const double h[9], int *xy)
{
    return ffgpu_warp_mesh_homography_host("warp_mesh_homography", dst_w, dst_h, cell, h, xy);
}
extern "C" int ffgpu_warp_mesh_lens(int dst_w, int dst_h, int cell, const ffgpu_warp_lens *lens, int *xy)
{
    return ffgpu_warp_mesh_lens_host("warp_mesh_lens", dst_w, dst_h, cell, lens, xy);
}
extern "C" int ffgpu_warp_point(const ffgpu_warp_mesh *mesh_on_host, int dst_w, int dst_h, int i, int j, int out[2])
{
    return ffgpu_warp_point_host("warp_point", mesh_on_host, dst_w, dst_h, i, j, out);
}
extern "C" int ffgpu_warp_tile(int out[4])
{
    if (!out) { ffgpu_set_error("warp_tile: NULL out"); return -1; }
    out[0] = WARP_TW; out[1] = WARP_TH; out[2] = WARP_LDS_BYTES; out[3] = WARP_ARG_JOBS;
    return 0;
}

// the planes of one kind, WARP_ARG_JOBS per launch, in order on the stream
template <int CH>
static int warp_launch(const std::vector<WarpJob> &jobs, const ffgpu_warp_spec *spec, unsigned fill, hipStream_t s)
{
    for (size_t i0 = 0; i0 < jobs.size(); i0 += WARP_ARG_JOBS) {
        const int n = (int)std::min((size_t)WARP_ARG_JOBS, jobs.size() - i0);
        WarpArgs a;
        memset(&a, 0, sizeof a);
        memcpy(a.j, jobs.data() + i0, sizeof(WarpJob) * (size_t)n);
        a.fill = fill; a.nearest = spec->filter == FFGPU_WARP_NEAREST; a.clamp = spec->border == FFGPU_WARP_CLAMP;
        hipLaunchKernelGGL(k_warp<CH>, dim3(ffgpu_warp_tiles(a.j, n), (unsigned)n), dim3(256), 0, s, a);
        LAUNCH_OK("warp");
    }
    return 0;
}

template <class Frame>
static int warp_dev(const char *what, const Frame *srcs, const Frame *dsts, const ffgpu_warp_mesh *meshes, int njobs, const ffgpu_warp_spec *spec, void *stream)
{
    if (ffgpu_no_device(what)) return -1;
    std::vector<WarpJob> jobs[2];
    if (ffgpu_warp_args_check(what, srcs, dsts, meshes, njobs, spec, jobs)) return -1;
    if (std::is_same<Frame, ffgpu_nv12_frame>::value)
        return warp_launch<1>(jobs[0], spec, spec->fill[0], (hipStream_t)stream) ||
               warp_launch<2>(jobs[1], spec, (unsigned)spec->fill[1] | (unsigned)spec->fill[2] << 8, (hipStream_t)stream) ? -1 : 0;
    return warp_launch<3>(jobs[0], spec, ffgpu_pack_colour(spec->fill), (hipStream_t)stream);
}

extern "C" int ffgpu_warp_bgr_dev(const ffgpu_bgr_frame *srcs, const ffgpu_bgr_frame *dsts, const ffgpu_warp_mesh *meshes, int njobs, const ffgpu_warp_spec *spec, void *stream)
{
    return warp_dev("warp_bgr_dev", srcs, dsts, meshes, njobs, spec, stream);
}
extern "C" int ffgpu_warp_nv12_dev(const ffgpu_nv12_frame *srcs, const ffgpu_nv12_frame *dsts, const ffgpu_warp_mesh *meshes, int njobs, const ffgpu_warp_spec *spec, void *stream)
{
    return warp_dev("warp_nv12_dev", srcs, dsts, meshes, njobs, spec, stream);
}
