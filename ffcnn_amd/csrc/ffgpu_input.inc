// ffgpu_input.inc -- the staging kernels: batched net_input (ffcnn.c:259-289) on the device.  u8 BGR or NV12 frames -> planar RGB fp32,
// nearest resize into the top-left sw x sh corner, zeros elsewhere; the output is the frame-major batch input (N x 3 x H x W) the ordinary
// graph consumes.  Also the per-frame descriptor table's upload, and the NV12 -> BGR conversion k_front (ffgpu_front.inc) shares.
struct InputP { float mean[3], norm[3]; };

// any W: one pixel per thread, every frame of the same geometry (ffgpu_exec_forward_bgr_dev when k_input4 cannot take the batch)
__global__ void k_input_bgr(const unsigned char *bgr, float *out, int N, int w, int h, int W, int H,
                            int sw, int sh, int s1, int s2, InputP p)
{
    const long total = (long)N * H * W;
    const long pitch = (long)((w * 3 + 3) & ~3);
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int x = (int)(idx % W);
        const long t = idx / W;
        const int y = (int)(t % H);
        const int n = (int)(t / H);
        float r = 0.f, g = 0.f, b = 0.f;
        if (x < sw && y < sh) {
            const unsigned char *px = bgr + (long)n * pitch * h + (long)((long)y * s1 / s2) * pitch + (long)((long)x * s1 / s2) * 3;
            r = ((float)px[2] - p.mean[0]) * p.norm[0];
            g = ((float)px[1] - p.mean[1]) * p.norm[1];
            b = ((float)px[0] - p.mean[2]) * p.norm[2];
        }
        float *o = out + (long)n * 3 * H * W + (long)y * W + x;
        o[0] = r; o[(long)H * W] = g; o[2L * H * W] = b;
    }
}

// NV12 -> B G R (bytes 0 1 2 of the result) of one pixel, include/ffcnn_hip.h's integer formula: every product fits 24 signed bits, >> is
// arithmetic, the clamp comes last.  m = { yoff, cy, crv, cgu, cgv, cbu } of the frame's matrix.
__constant__ int c_yuv_mat[4][6] = FFGPU_YUV_MATRICES;
struct YuvMat { int yoff, cy, crv, cgu, cgv, cbu; };
__device__ __forceinline__ YuvMat yuv_mat(int fmt)
{
    const int *m = c_yuv_mat[(fmt - 1) & 3];
    return YuvMat{ m[0], m[1], m[2], m[3], m[4], m[5] };
}
__device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }
__device__ __forceinline__ unsigned nv12_to_bgr(int Y, int U, int V, const YuvMat &m)
{
    // (every factor and every product fits 24 signed bits: __mul24 is exact and a full-rate v_mul_i32_i24 / v_mad_i32_i24, a plain int product is not)
    const int c = __mul24(m.cy, Y - m.yoff) + 128, d = U - 128, e = V - 128;
    const int r = clamp255((c + __mul24(m.crv, e)) >> 8), g = clamp255((c - __mul24(m.cgu, d) - __mul24(m.cgv, e)) >> 8), b = clamp255((c + __mul24(m.cbu, d)) >> 8);
    return (unsigned)b | ((unsigned)g << 8) | ((unsigned)r << 16);
}

// What k_input4 is instantiated with: where a frame's descriptor comes from -- desc(n), read once per thread -- and how the four source pixels
// of output pixels x0 .. x0 + 3 of row y are fetched -- load4, each pixel packed B | G << 8 | R << 16 (columns past sw - 1 repeat that column;
// the caller zeroes them).  Both pixel formats read a thread's bytes as whole dwords when the frame is not resized and its rows are dword
// aligned, and pixel by pixel otherwise.
struct BgrPixels {
    static __device__ __forceinline__ void load4(const FrameDesc &fd, int x0, int y, unsigned px[4])
    {
        const unsigned char *row = fd.bgr + (long)((long)y * fd.s1 / fd.s2) * fd.pitch;
        if (fd.s1 == fd.s2 && x0 + 3 < fd.sw && ((reinterpret_cast<uintptr_t>(fd.bgr) | (unsigned)fd.pitch) & 3) == 0) {   // 12 contiguous bytes (3 x0 % 4 == 0)
            const unsigned *q = reinterpret_cast<const unsigned *>(row + 3 * x0);
            const unsigned d0 = q[0], d1 = q[1], d2 = q[2];
            px[0] = d0 & 0xffffffu; px[1] = (d0 >> 24) | ((d1 & 0xffffu) << 8); px[2] = (d1 >> 16) | ((d2 & 0xffu) << 16); px[3] = d2 >> 8;
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int x = min(x0 + i, fd.sw - 1);
                const unsigned char *s = row + (long)((long)x * fd.s1 / fd.s2) * 3;
                px[i] = (unsigned)s[0] | ((unsigned)s[1] << 8) | ((unsigned)s[2] << 16);
            }
        }
    }
};
// the pixel is made from the Y plane's byte and the chroma pair of its 2 x 2 block (nearest chroma); converting only the sampled pixel is
// converting the whole image first, because net_input samples nearest-neighbour.  The byte path reads a byte and an aligned 16-bit pair.
struct Nv12Pixels {
    static __device__ __forceinline__ void load4(const FrameDesc &fd, int x0, int y, unsigned px[4])
    {
        const YuvMat m = yuv_mat(fd.fmt);
        const long ys = (long)y * fd.s1 / fd.s2;
        const unsigned char *yrow = fd.bgr + ys * fd.pitch, *crow = fd.uv + (ys >> 1) * fd.pitch_uv;
        if (fd.s1 == fd.s2 && x0 + 3 < fd.sw && ((reinterpret_cast<uintptr_t>(fd.bgr) | (unsigned)fd.pitch) & 3) == 0) {   // (sw == w)
            const unsigned yy = *reinterpret_cast<const unsigned *>(yrow + x0);
            unsigned cc;                                               // the two chroma pairs of pixels x0, x0 + 1 | x0 + 2, x0 + 3: bytes x0 .. x0 + 3 of the row
            if (((reinterpret_cast<uintptr_t>(fd.uv) | (unsigned)fd.pitch_uv) & 3) == 0) cc = *reinterpret_cast<const unsigned *>(crow + x0);
            else cc = (unsigned)*reinterpret_cast<const unsigned short *>(crow + x0) | ((unsigned)*reinterpret_cast<const unsigned short *>(crow + x0 + 2) << 16);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const unsigned pr = cc >> (16 * (i >> 1));
                px[i] = nv12_to_bgr((int)((yy >> (8 * i)) & 0xffu), (int)(pr & 0xffu), (int)((pr >> 8) & 0xffu), m);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int x = min(x0 + i, fd.sw - 1);
                const long xs = (long)x * fd.s1 / fd.s2;
                const unsigned pr = *reinterpret_cast<const unsigned short *>(crow + (xs & ~1L));      // U V of the pixel's 2 x 2 block: 2-byte aligned
                px[i] = nv12_to_bgr((int)yrow[xs], (int)(pr & 0xffu), (int)(pr >> 8), m);
            }
        }
    }
};
// ffgpu_exec_forward_bgr_dev: every frame the same geometry, `frame` bytes apart -- the descriptor travels by value as the kernel's argument
struct UniformBgr : BgrPixels {
    FrameDesc fd; long frame;
    __device__ __forceinline__ FrameDesc desc(unsigned n) const { FrameDesc d = fd; d.bgr += (long)n * frame; return d; }
};
// the frame-table entry points: every frame its own descriptor, any size, pitch and byte alignment
template <class Pixels> struct TableOf : Pixels {
    const FrameDesc *tab;
    __device__ __forceinline__ FrameDesc desc(unsigned n) const { return tab[n]; }
};

// A thread owns 4 consecutive output pixels of one row (one 32-bit division per thread, blockIdx.y = frame) and writes one 16-byte store per
// colour plane where W % 4 == 0.  Same arithmetic per pixel as k_input_bgr ((byte - mean) * norm, two roundings).
template <class Src>
__global__ void __launch_bounds__(256) k_input4(Src src, float *out, int W, int H, InputP p)
{
    typedef float f4 __attribute__((ext_vector_type(4)));
    const unsigned wq = ((unsigned)W + 3) >> 2, t = blockIdx.x * 256 + threadIdx.x;
    if (t >= wq * (unsigned)H) return;
    const int y = (int)(t / wq), x0 = (int)(t - (unsigned)y * wq) * 4, n = blockIdx.y;
    const FrameDesc fd = src.desc(n);
    f4 r = { 0.f, 0.f, 0.f, 0.f }, g = r, b = r;
    if (y < fd.sh && x0 < fd.sw) {
        unsigned px[4];
        Src::load4(fd, x0, y, px);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const bool in = x0 + i < fd.sw;
            r[i] = in ? ((float)((px[i] >> 16) & 0xffu) - p.mean[0]) * p.norm[0] : 0.f;
            g[i] = in ? ((float)((px[i] >> 8) & 0xffu) - p.mean[1]) * p.norm[1] : 0.f;
            b[i] = in ? ((float)(px[i] & 0xffu) - p.mean[2]) * p.norm[2] : 0.f;
        }
    }
    float *o = out + (long)n * 3 * H * W + (long)y * W + x0;
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

// the per-frame table of ffgpu_exec_forward_bgr_frames_dev / _nv12_frames_dev: FRAMES_CHUNK descriptors travel by value as the kernel's argument (no
// pinned staging, no host sync: the caller's array is free on return), one thread per descriptor: 64 x 56 = 3 588 bytes of arguments with the count, one
// launch for a batch of 64
#define FRAMES_CHUNK 64
struct FramesChunk { FrameDesc d[FRAMES_CHUNK]; int n; };
static_assert(sizeof(FramesChunk) + sizeof(FrameDesc *) <= 4096 - 256, "k_set_frames: the chunk travels as a kernel argument (4 KB at most, the hidden arguments included)");
__global__ void k_set_frames(FrameDesc *tab, FramesChunk c)
{
    if (threadIdx.x < (unsigned)c.n) tab[threadIdx.x] = c.d[threadIdx.x];
}

int ffgpu_launch_set_frames(FrameDesc *d_tab, const FrameDesc *h_desc, int n, hipStream_t s)
{
    for (int i0 = 0; i0 < n; i0 += FRAMES_CHUNK) {
        FramesChunk c;
        memset(&c, 0, sizeof c);
        c.n = std::min(FRAMES_CHUNK, n - i0);
        memcpy(c.d, h_desc + i0, sizeof(FrameDesc) * c.n);
        hipLaunchKernelGGL(k_set_frames, dim3(1), dim3(FRAMES_CHUNK), 0, s, d_tab + i0, c);
        LAUNCH_OK("set_frames");
    }
    return 0;
}

// (the caller has checked N <= 65535 and (W + 3) / 4 * H < 2^31)
template <class Src>
static int launch_input4(const Src &src, float *out, int N, int W, int H, const float mean[3], const float norm[3], const char *what, hipStream_t s)
{
    InputP p;
    for (int i = 0; i < 3; i++) { p.mean[i] = mean[i]; p.norm[i] = norm[i]; }
    hipLaunchKernelGGL(k_input4<Src>, dim3((unsigned)(((long)((W + 3) / 4) * H + 255) / 256), (unsigned)N), dim3(256), 0, s, src, out, W, H, p);
    LAUNCH_OK(what);
    return 0;
}

int ffgpu_launch_input_bgr(const unsigned char *bgr, float *out, int N, int w, int h, int W, int H,
                           int sw, int sh, int s1, int s2, const float mean[3], const float norm[3], hipStream_t s)
{
    if (W % 4 == 0 && N <= 65535 && (long)W * H < (1L << 31)) {
        UniformBgr src;
        memset(&src, 0, sizeof src);
        src.fd.bgr = bgr; src.fd.w = w; src.fd.h = h; src.fd.pitch = (w * 3 + 3) & ~3; src.fd.sw = sw; src.fd.sh = sh; src.fd.s1 = s1; src.fd.s2 = s2;
        src.frame = (long)src.fd.pitch * h;
        return launch_input4(src, out, N, W, H, mean, norm, "input_bgr4", s);
    }
    InputP p;
    for (int i = 0; i < 3; i++) { p.mean[i] = mean[i]; p.norm[i] = norm[i]; }
    hipLaunchKernelGGL(k_input_bgr, dim3(grid_for((long)N * H * W, 256)), dim3(256), 0, s, bgr, out, N, w, h, W, H, sw, sh, s1, s2, p);
    LAUNCH_OK("input_bgr");
    return 0;
}

int ffgpu_launch_input_frames(const FrameDesc *d_tab, bool nv12, float *out, int N, int W, int H, const float mean[3], const float norm[3], hipStream_t s)
{
    const char *const what = nv12 ? "input_nv12_frames" : "input_frames";
    if (N > 65535 || (long)((W + 3) / 4) * H >= (1L << 31)) { ffgpu_set_error("%s: %d frames of %d x %d is too large", what, N, W, H); return -1; }
    if (nv12) { TableOf<Nv12Pixels> src; src.tab = d_tab; return launch_input4(src, out, N, W, H, mean, norm, what, s); }
    TableOf<BgrPixels> src; src.tab = d_tab;
    return launch_input4(src, out, N, W, H, mean, norm, what, s);
}
