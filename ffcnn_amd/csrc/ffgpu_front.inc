// ffgpu_front.inc -- the net's first FOUR layers as one streaming kernel: dense 3x3 stride-2 convolution from 3 channels
// to 8 (layer 0: convolution_generic + im2row, conv-v6.c:9-42) feeding the first 8-channel inverted-residual block
// (1x1 8 -> 8, depthwise 3x3, 1x1 8 -> OC: conv-v6.c:46-91 / 96-229 / 46-91) without the 8-channel 160x160 tensor ever
// reaching memory.  With several batches in flight both k_conv_first and k_irb_thin ran at the speed of their HBM traffic
// (78.6 MB in, 52.4 out; 52.4 in, 26.2 out per 64 frames): fused, 78.6 MB come in and 26.2 go out.
//
// Structure = k_irb_thin's (a wave owns a band of output rows of a frame, lane -> 4 columns, an expanded row is folded
// into the three depthwise sums it touches the moment it exists) with the block's input row produced in registers: for
// output row r of layer 0 the lane holds the three input rows 2r-1, 2r, 2r+1 of its eight columns per channel (the last
// one is carried into the next step, the two new ones are in flight during the block's arithmetic), the column to the
// left comes from the neighbour lane by DPP, and the 27 x 8 taps are read from LDS as output-channel PAIRS, so all
// arithmetic is packed and the reference's accumulation orders (ci, ky, kx; ci; w0..w8; c) are kept per output.
struct FrontP {
    const float *in; float *out;
    const float *const *in_ind;      // optional device slot holding the input pointer (ConvDesc::in_ind)
    const ExecParams *prm;           // U8 form: the executor's parameter block (u8 BGR source, pitch, mean / norm of this forward)
    const float *f0;                 // layer 0 filter rows [8][32] (27 taps, scale' at 28, bias' at 29)
    const float *w1, *wd, *w2;       // the block's filter rows: w1 [8][12], wd [8][16], w2 [OC][12]
    long in_cs, in_ns;               // input strides (frame-major batch input or CNHW)
    int W, H, N;                     // geometry of the 8-channel plane = output plane (W % 4 == 0, W / 4 <= 64); input is 2W x 2H
    int band, nbands, ntasks;
    float act0, act1, actd, act2;    // slopes: act(x) = max(x, slope x)
};

// U8 (round 3): the batch arrives as u8 BGR images of the net's own geometry (net_input without resize, ffcnn.c:259-289) and the
// kernel converts while it loads: a lane's eight columns of a row are 24 contiguous bytes (one 16-byte + one 8-byte load instead of
// six 16-byte loads), plane 0 / 1 / 2 = (R - mean[0]) * norm[0], (G - mean[1]) * norm[1], (B - mean[2]) * norm[2] with the
// reference's two roundings.  The raw dwords stay in flight during the block's arithmetic exactly like the fp32 rows and are
// converted where the next step consumes them; the 78.6 MB fp32 batch of k_input_bgr4 is never written or read.
// NC = output columns per lane.  4: a 160-pixel row occupies 40 of a wave's 64 lanes.  3 (round 5): 54 lanes -- a quarter fewer vector instructions per row
// (every instruction is a wave's), 75 registers less.  A width that is not a multiple of 3 lets the LAST lane slide left to end with the row (it overlaps its
// neighbour by `sl` columns, computed twice, stored twice with the same values): no column outside the row is ever loaded, computed or stored; what changes is
// which of the neighbour's registers the two lanes at the seam take as their left / right column (wave-uniform `sl`).
// RS (U8 as well): the frames of ffgpu_exec_forward_bgr_frames_dev -- every frame its own u8 BGR source of any size, pitch and byte alignment,
// letterboxed into the plane as net_input does (ffcnn.c:267-289).  The frame is wave-uniform (n = task / nbands), so its descriptor (the
// parameter block's frames_tab[n]) comes in with scalar loads.  Per task a lane computes the source byte offsets of its 2 NC input columns
// (x s1 / s2, 64-bit products as k_input_bgr4), per row the wave maps y to y s1 / s2; a pixel is two aligned dwords (the one holding its first
// byte and the one holding its last: neither reaches past the frame's own bytes' dwords) and a byte align.  Columns x >= sw and rows
// y >= sh are 0.0f, as the staged path writes them.  A frame of the net's own size whose rows are dword aligned takes the U8 form's
// contiguous-dword loads instead (wave-uniform branch).  Everything behind the conversion is the U8 form's code.
__device__ __forceinline__ unsigned front_muldiv(unsigned x, unsigned s1, unsigned s2)
{
    const unsigned long long t = (unsigned long long)x * s1;
    return (t >> 32) ? (unsigned)(t / s2) : (unsigned)t / s2;
}
// (byte - mean) * norm with the reference's two roundings, as two plain VALU instructions: the resizing form's conversion is never paired into
// packed fp32 instructions (tools/isa_lint.py: no new packed forms)
__device__ __forceinline__ float front_cvt(unsigned byte, float m, float s)
{
    float t, v;
    asm("v_sub_f32 %0, %1, %2" : "=v"(t) : "v"((float)byte), "v"(m));
    asm("v_mul_f32 %0, %1, %2" : "=v"(v) : "v"(t), "v"(s));
    return v;
}

// NV (RS as well): the frames of ffgpu_exec_forward_nv12_frames_dev.  The same gather with a pixel made of its Y byte (one byte load) and the U V pair
// of its 2 x 2 block (one aligned 16-bit load: the chroma plane is 2-byte aligned, its pitch even): 12 raw dwords per lane and row in flight, as in RS.
// A lane's column offsets serve both planes (x' in the Y row, x' & ~1 in the chroma row); per row the wave maps y -> y' = y s1 / s2 and the chroma row
// y' >> 1.  The matrix is the frame's, hence the wave's: six scalar values.  Integer conversion (nv12_to_bgr) where cvt_row converts, then front_cvt.
template <int OC, bool U8, int NC = 4, bool RS = false, bool NV = false>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) k_front(FrontP p)
{
    static_assert(NC == 4 || NC == 3, "columns per lane");
    static_assert(!RS || (U8 && NC == 3), "the resizing form reads u8 frames, three columns per lane");
    static_assert(!NV || RS, "the NV12 form is a resizing form");
    constexpr int IC = 8, EC = 8, CP = EC / 2, RL1 = 12, RL2 = 12, OCP = (OC + 3) & ~3;
    // LDS tables: t0 [27 taps][4 oc pairs][2] + scale' pairs [4][2] + bias' pairs [4][2] of layer 0; then the block's
    // tables exactly as in k_irb_thin (t1 | td | t2 | sb2)
    constexpr int T0 = 27 * 8 + 16, T1 = (IC + 2) * 2, TD = 24, T2 = 2 * OCP;
    __shared__ __attribute__((aligned(16))) float tw[T0 + CP * (T1 + TD + T2) + 2 * OCP];
    float *t0 = tw, *t1 = tw + T0, *td = t1 + CP * T1, *t2 = td + CP * TD, *tsb = t2 + CP * T2;
    for (int i = threadIdx.x; i < T0; i += 256) {
        const int tap = i >> 3, o = i & 7;                           // [tap][oc] = [tap][pair][2]; taps 27 / 28: scale', bias'
        t0[i] = p.f0[o * 32 + (tap < 27 ? tap : tap + 1)];
    }
    for (int i = threadIdx.x; i < CP * T1; i += 256) {
        const int cp = i / T1, j = (i % T1) >> 1, c = 2 * cp + (i & 1);
        t1[i] = p.w1[c * RL1 + (j < IC ? j : 8 + (j - IC))];
    }
    for (int i = threadIdx.x; i < CP * TD; i += 256) {
        const int cp = i / TD, j = (i % TD) >> 1, c = 2 * cp + (i & 1);
        td[i] = j < 9 ? p.wd[c * 16 + j] : (j < 11 ? p.wd[c * 16 + 3 + j] : 0.f);
    }
    for (int i = threadIdx.x; i < CP * T2; i += 256) {
        const int cp = i / T2, h = (i % T2) / OCP, k = i % OCP;
        t2[i] = k < OC ? p.w2[k * RL2 + 2 * cp + h] : 0.f;
    }
    for (int i = threadIdx.x; i < 2 * OCP; i += 256) { const int k = i % OCP; tsb[i] = k < OC ? p.w2[k * RL2 + RL2 - 4 + i / OCP] : 0.f; }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int task = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // wave-uniform, and known to be
    if (task >= p.ntasks) return;
    const int n = task / p.nbands, band_i = task - n * p.nbands;
    const int lpr = (p.W + NC - 1) / NC;
    const bool on = lane < lpr, last_col = lane == lpr - 1, seam_l = lane == lpr - 2;
    const int sl = lpr * NC - p.W;                                   // wave-uniform: columns the last lane slides left (0 for NC = 4: W % 4 == 0)
    const int IW = 2 * p.W, IH = 2 * p.H;
    const unsigned HW = (unsigned)p.W * p.H, cs = (unsigned)p.N * HW;
    const unsigned lo = on ? (unsigned)min(lane * NC, p.W - NC) : 0, li = 2 * lo;      // idle lanes work on column 0; nothing of theirs is stored
    // (both inputs are named through the parameter block: global address space, not flat -- see ffgpu_kernels.hip)
    const gfp ip = U8 ? nullptr : to_global(p.in_ind ? *p.in_ind : p.in) + (long)n * p.in_ns;
    const FFG unsigned char *bp = U8 && !RS ? (const FFG unsigned char *)p.prm->bgr + (long)n * p.prm->bgr_frame + ((3u * li) & ~3u) : nullptr;     // this lane's 6 NC bytes of a row, from the dword they start in
    const unsigned bsh = (3u * li) & 3u;                             // ... and where in that dword (NC = 3: 18 bytes per lane start at 0 or 2)
    const unsigned bpitch = U8 && !RS ? (unsigned)p.prm->bgr_pitch : 0u;
    // RS: the frame's source, the rows that hold pixels (ihv: min(IH, sh), none when sw == 0), the lane's column offsets / which of them hold pixels
    const FFG unsigned char *fsrc = nullptr;
    unsigned long fpitch = 0, fpitch_uv = 0;
    const FFG unsigned char *fuv = nullptr;
    YuvMat ym = { 0, 0, 0, 0, 0, 0 };
    unsigned fs1 = 1, fs2 = 1, cmask = 0, coff[2 * NC];
    int ihv = IH;
    bool ffast = false;
    if (RS) {
        const FrameDesc *fd = p.prm->frames_tab + n;                // (the values are the wave's: said so, they live in scalar registers)
        const uintptr_t a = reinterpret_cast<uintptr_t>(fd->bgr);
        const unsigned alo = __builtin_amdgcn_readfirstlane((unsigned)a), ahi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
        fsrc = (const FFG unsigned char *)(((uintptr_t)ahi << 32) | alo);
        fpitch = (unsigned)__builtin_amdgcn_readfirstlane(fd->pitch);
        fs1 = (unsigned)__builtin_amdgcn_readfirstlane(fd->s1); fs2 = (unsigned)__builtin_amdgcn_readfirstlane(fd->s2);
        const int sw = __builtin_amdgcn_readfirstlane(fd->sw), sh = __builtin_amdgcn_readfirstlane(fd->sh);
        const int fw = __builtin_amdgcn_readfirstlane(fd->w), fh = __builtin_amdgcn_readfirstlane(fd->h);
        ihv = sw > 0 ? min(IH, sh) : 0;
        ffast = !NV && fw == IW && fh == IH && ((alo | (unsigned)fpitch) & 3u) == 0;      // (then s1 == s2, sw = IW, sh = IH)
        if constexpr (NV) {
            const uintptr_t c = reinterpret_cast<uintptr_t>(fd->uv);
            const unsigned clo = __builtin_amdgcn_readfirstlane((unsigned)c), chi = __builtin_amdgcn_readfirstlane((unsigned)(c >> 32));
            fuv = (const FFG unsigned char *)(((uintptr_t)chi << 32) | clo);
            fpitch_uv = (unsigned)__builtin_amdgcn_readfirstlane(fd->pitch_uv);
            const YuvMat m = yuv_mat(__builtin_amdgcn_readfirstlane(fd->fmt));
            ym = YuvMat{ __builtin_amdgcn_readfirstlane(m.yoff), __builtin_amdgcn_readfirstlane(m.cy), __builtin_amdgcn_readfirstlane(m.crv),
                         __builtin_amdgcn_readfirstlane(m.cgu), __builtin_amdgcn_readfirstlane(m.cgv), __builtin_amdgcn_readfirstlane(m.cbu) };
        }
#pragma unroll
        for (int i = 0; i < 2 * NC; i++) {
            const unsigned x = li + i;
            const bool in = (int)x < sw;
            coff[i] = in ? (NV ? 1u : 3u) * front_muldiv(x, fs1, fs2) : 0u;         // (a column outside the frame reads pixel 0 of the row; its value is 0)
            cmask |= in ? 1u << i : 0u;
        }
    }
    float cm[3] = { 0.f, 0.f, 0.f }, cn[3] = { 1.f, 1.f, 1.f };
    if (U8) {
#pragma unroll
        for (int k = 0; k < 3; k++) { cm[k] = p.prm->mean[k]; cn[k] = p.prm->norm[k]; }
    }
    float *op = p.out + (long)n * HW;
    const int y0 = band_i * p.band, y1 = min(y0 + p.band, p.H);
    const v2f_t z2 = { 0.f, 0.f };
    const v4f z4 = { 0.f, 0.f, 0.f, 0.f };

    // input row `row` of the lane's eight columns, three channels (zero outside the image: layer 0 pads with zeros)
    typedef unsigned u4_t __attribute__((ext_vector_type(4)));
    typedef unsigned u2_t __attribute__((ext_vector_type(2)));
    // the lane's 24 bytes start at 24 * lane in a row whose pitch is a multiple of 4: DWORD aligned, no more -- the loads say so
    // (gfx9 global loads of 8 / 16 bytes need only dword alignment; the types must not promise the compiler more than that)
    typedef u4_t u4a4_t __attribute__((aligned(4)));
    typedef u2_t u2a4_t __attribute__((aligned(4)));
    struct RowB { v4f a[3], b[3]; u4_t q0; u2_t q1; };              // the lane's 2 NC input columns of three channels (a: 0-3, b: 4-..); U8: the raw dwords (NC = 3: q1.x only)
    struct RowG { v4f a[3], b[3]; u4_t q0; u2_t q1; unsigned g[4 * NC]; unsigned sh; };   // RS: two dwords per pixel (g[2 i], g[2 i + 1]) and the row's byte misalignment, or g[0..5] as q0 / q1
    typedef std::conditional_t<RS, RowG, RowB> Row;

#define ROWC(R, ci, i) ((i) < 4 ? (R).a[ci][(i) & 3] : (R).b[ci][((i) - 4) & 3])       /* column i (a compile-time index after unrolling) */
    // U8: the raw bytes of row `row` (nothing for a row outside the image) ...
    auto load_irow_rs = [&](int row, Row &R) __attribute__((always_inline)) {
        if constexpr (RS) {
            if (row < 0 || row >= ihv) return;                        // wave-uniform; cvt_row makes the zeros
            if constexpr (NV) {
                const unsigned ys = front_muldiv((unsigned)row, fs1, fs2);                                  // uniform, as the two row bases are
                const FFG unsigned char *yr = fsrc + (unsigned long)ys * fpitch, *cr = fuv + (unsigned long)(ys >> 1) * fpitch_uv;
#pragma unroll
                for (int i = 0; i < 2 * NC; i++) {
                    R.g[2 * i] = yr[coff[i]];
                    R.g[2 * i + 1] = *(const FFG unsigned short *)(cr + (coff[i] & ~1u));
                }
                R.sh = 0u;
                return;
            }
            unsigned v[4 * NC], r3 = 0;                               // (both branches write every element: no store the compiler could merge into one through a selected address)
            if (ffast) {
                const FFG unsigned char *src = fsrc + (unsigned long)row * fpitch + ((3u * li) & ~3u);
                const u4_t a = *(const FFG u4a4_t *)src;
                v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
                if (NC == 4) { const u2_t b = *(const FFG u2a4_t *)(src + 16); v[4] = b.x; v[5] = b.y; }
                else { v[4] = *(const FFG unsigned *)(src + 16); v[5] = 0u; }
#pragma unroll
                for (int k = 6; k < 4 * NC; k++) v[k] = 0u;
            } else {
                const FFG unsigned char *rb = fsrc + (unsigned long)front_muldiv((unsigned)row, fs1, fs2) * fpitch;     // uniform
                r3 = (unsigned)reinterpret_cast<uintptr_t>(rb) & 3u;
                const FFG unsigned *ra = (const FFG unsigned *)(rb - r3);
#pragma unroll
                for (int i = 0; i < 2 * NC; i++) {
                    const unsigned o = r3 + coff[i];
                    v[2 * i] = ra[o >> 2];                            // the dword holding the pixel's first byte ...
                    v[2 * i + 1] = ra[(o + 2) >> 2];                  // ... and the one holding its last (the same one when o % 4 < 2)
                }
            }
#pragma unroll
            for (int k = 0; k < 4 * NC; k++) R.g[k] = v[k];
            R.sh = r3;
        }
    };
    auto load_irow_u8 = [&](int row, Row &R) __attribute__((always_inline)) {
        if constexpr (RS) { load_irow_rs(row, R); return; }
        if (row < 0 || row >= IH) return;                             // wave-uniform; cvt_row makes the zeros
        const FFG unsigned char *src = bp + (unsigned)row * bpitch;
        R.q0 = *(const FFG u4a4_t *)src;
        if (NC == 4) R.q1 = *(const FFG u2a4_t *)(src + 16);
        else { R.q1.x = *(const FFG unsigned *)(src + 16); R.q1.y = 0u; }
    };
    // ... and their conversion into the three planes' eight columns, where the row is consumed
    auto cvt_row = [&](int row, Row &R) __attribute__((always_inline)) {
        if (row < 0 || row >= (RS ? ihv : IH)) {
#pragma unroll
            for (int ci = 0; ci < 3; ci++) { R.a[ci] = z4; R.b[ci] = z4; }
            return;
        }
        if constexpr (RS) if (NV || !ffast) {
#pragma unroll
            for (int i = 0; i < 2 * NC; i++) {
                unsigned px;                                                                                            // B G R in bytes 0 1 2
                if constexpr (NV) px = nv12_to_bgr((int)R.g[2 * i], (int)(R.g[2 * i + 1] & 0xffu), (int)(R.g[2 * i + 1] >> 8), ym);
                else px = __builtin_amdgcn_alignbyte(R.g[2 * i + 1], R.g[2 * i], (R.sh + coff[i]) & 3u);
                const bool in = (cmask >> i) & 1u;
#pragma unroll
                for (int ci = 0; ci < 3; ci++) {
                    const float v = in ? front_cvt((px >> (8 * (2 - ci))) & 0xffu, cm[ci], cn[ci]) : 0.f;
                    if (i < 4) R.a[ci][i & 3] = v; else R.b[ci][(i - 4) & 3] = v;
                }
            }
            return;
        }
        unsigned d[6] = { R.q0.x, R.q0.y, R.q0.z, R.q0.w, R.q1.x, R.q1.y };
        if constexpr (RS) { d[0] = R.g[0]; d[1] = R.g[1]; d[2] = R.g[2]; d[3] = R.g[3]; d[4] = R.g[4]; d[5] = R.g[5]; }
        if (NC == 3) {                                                // the lane's 18 bytes start 0 or 2 bytes into the first dword
#pragma unroll
            for (int i = 0; i < 5; i++) d[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], bsh);
        }
#pragma unroll
        for (int i = 0; i < 2 * NC; i++)
#pragma unroll
            for (int ci = 0; ci < 3; ci++) {
                const int k = 3 * i + 2 - ci;                         // plane 0 = R (byte 2 of the pixel), 1 = G, 2 = B
                float v;
                if constexpr (RS) v = front_cvt((d[k >> 2] >> (8 * (k & 3))) & 0xffu, cm[ci], cn[ci]);
                else v = ((float)((d[k >> 2] >> (8 * (k & 3))) & 0xffu) - cm[ci]) * cn[ci];
                if (i < 4) R.a[ci][i] = v; else R.b[ci][i - 4] = v;
            }
    };
    auto load_irow = [&](int row, Row &R) __attribute__((always_inline)) {
        if (U8) { load_irow_u8(row, R); return; }
        if (row < 0 || row >= IH) {                                   // wave-uniform
#pragma unroll
            for (int ci = 0; ci < 3; ci++) { R.a[ci] = z4; R.b[ci] = z4; }
            return;
        }
        const unsigned ro = (unsigned)row * IW + li;
        typedef float v4a4 __attribute__((ext_vector_type(4), aligned(4)));      // (6 floats per lane start 8-byte aligned at most: dword alignment is all the loads need)
        typedef float v2a4 __attribute__((ext_vector_type(2), aligned(4)));
#pragma unroll
        for (int ci = 0; ci < 3; ci++) {
            const gfp src = ip + ci * p.in_cs;                        // uniform
            if (NC == 4) { R.a[ci] = gld<v4f>(src + ro); R.b[ci] = gld<v4f>(src + (ro + 4)); }
            else { R.a[ci] = (v4f)gld<v4a4>(src + ro); const v2f_t b = (v2f_t)gld<v2a4>(src + (ro + 4)); R.b[ci] = (v4f){ b.x, b.y, 0.f, 0.f }; }
        }
    };

    struct W1T { v4f q[T1 / 4]; };
    struct WDT { v4f q[TD / 4]; v4f w2[T2 / 4]; };
    auto ld1 = [&](int cp) { W1T r;
#pragma unroll
        for (int j = 0; j < T1 / 4; j++) r.q[j] = *reinterpret_cast<const v4f *>(t1 + cp * T1 + 4 * j);
        return r; };
    auto ldd = [&](int cp) { WDT r;
#pragma unroll
        for (int j = 0; j < TD / 4; j++) r.q[j] = *reinterpret_cast<const v4f *>(td + cp * TD + 4 * j);
#pragma unroll
        for (int j = 0; j < T2 / 4; j++) r.w2[j] = *reinterpret_cast<const v4f *>(t2 + cp * T2 + 4 * j);
        return r; };

    v2f_t A[2][CP][NC];               // the block's depthwise sums under way (see k_irb_thin)
    Row R[3];                         // input rows 2r-1 (carried), 2r, 2r+1 of the step's layer-0 row r: R[0], R[1], R[2] at even steps,
                                      // R[2], R[1], R[0] at odd ones -- the carried row changes role, not registers
#pragma unroll
    for (int c = 0; c < CP; c++)
#pragma unroll
        for (int j = 0; j < NC; j++) A[0][c][j] = A[1][c][j] = z2;
    {
        const int r = y0 - 1;
        if (r >= 0) { load_irow(2 * r - 1, R[0]); load_irow(2 * r, R[1]); load_irow(2 * r + 1, R[2]); }
        else        { load_irow(-1, R[0]); load_irow(-1, R[1]); load_irow(2 * r + 1, R[2]); }      // only row -1 matters (as the carried row of step 0)
        if (U8) cvt_row(r >= 0 ? 2 * r - 1 : -1, R[0]);              // the carried row of the first step; the two others are converted by that step
    }

    auto step = [&](int r, auto PAR) {
        constexpr int P = decltype(PAR)::value;
        asm volatile("" ::: "memory");                             // the tables are re-read every row
        const bool rin = r >= 0 && r < p.H, fin = r > y0;          // wave-uniform
        Row &C = R[P ? 2 : 0], &N0 = R[1], &N1 = R[P ? 0 : 2];
        if (U8) {                                                     // rows 2r, 2r+1 arrived as bytes (the prologue's r = -1 step: rows -1 -> zeros, -1)
            cvt_row(r >= 0 ? 2 * r : -1, N0);
            cvt_row(2 * r + 1, N1);
        }
        // ---- layer 0, output row r: x[pair][pixel] = act0(scale' * sum + bias'), channels (2 pair, 2 pair + 1)
        v2f_t x[4][NC];
        if (rin) {
#pragma unroll
            for (int pr = 0; pr < 4; pr++)
#pragma unroll
                for (int j = 0; j < NC; j++) x[pr][j] = z2;
#pragma unroll
            for (int ci = 0; ci < 3; ci++) {
#pragma unroll
                for (int ky = 0; ky < 3; ky++) {
                    const Row &R = ky == 0 ? C : (ky == 1 ? N0 : N1);
                    float win[2 * NC + 1];                            // input columns 2 lo - 1 .. 2 lo + 2 NC - 1
#pragma unroll
                    for (int i = 0; i < 2 * NC; i++) win[1 + i] = ROWC(R, ci, i);
                    win[0] = dpp_shr1(ROWC(R, ci, 2 * NC - 1));
                    if (NC == 3 && sl) {                              // the slid last lane's left column is its neighbour's column 2 NC - 1 - 2 sl = 3 / 1
                        const float alt = dpp_shr1(sl == 2 ? R.a[ci].y : R.a[ci].w);
                        win[0] = last_col ? alt : win[0];
                    }
#pragma unroll
                    for (int kx = 0; kx < 3; kx++) {
                        const float *tp = t0 + ((ci * 3 + ky) * 3 + kx) * 8;
                        const v4f ta = *reinterpret_cast<const v4f *>(tp), tb = *reinterpret_cast<const v4f *>(tp + 4);
                        const v2f_t t[4] = { { ta.x, ta.y }, { ta.z, ta.w }, { tb.x, tb.y }, { tb.z, tb.w } };
#pragma unroll
                        for (int j = 0; j < NC; j++)
#pragma unroll
                            for (int pr = 0; pr < 4; pr++) x[pr][j] += t[pr] * win[2 * j + kx];
                    }
                }
                if constexpr (NC == 4) {
                    asm volatile("" : "+v"(x[0][0]), "+v"(x[0][1]), "+v"(x[0][2]), "+v"(x[0][3]), "+v"(x[1][0]), "+v"(x[1][1]), "+v"(x[1][2]), "+v"(x[1][3]));
                    asm volatile("" : "+v"(x[2][0]), "+v"(x[2][1]), "+v"(x[2][2]), "+v"(x[2][3]), "+v"(x[3][0]), "+v"(x[3][1]), "+v"(x[3][2]), "+v"(x[3][3]));
                } else {
                    asm volatile("" : "+v"(x[0][0]), "+v"(x[0][1]), "+v"(x[0][2]), "+v"(x[1][0]), "+v"(x[1][1]), "+v"(x[1][2]));
                    asm volatile("" : "+v"(x[2][0]), "+v"(x[2][1]), "+v"(x[2][2]), "+v"(x[3][0]), "+v"(x[3][1]), "+v"(x[3][2]));
                }
            }
            const v4f sa = *reinterpret_cast<const v4f *>(t0 + 216), sb = *reinterpret_cast<const v4f *>(t0 + 220),
                      ba = *reinterpret_cast<const v4f *>(t0 + 224), bb = *reinterpret_cast<const v4f *>(t0 + 228);
            const v2f_t sc[4] = { { sa.x, sa.y }, { sa.z, sa.w }, { sb.x, sb.y }, { sb.z, sb.w } };
            const v2f_t bi[4] = { { ba.x, ba.y }, { ba.z, ba.w }, { bb.x, bb.y }, { bb.z, bb.w } };
#pragma unroll
            for (int pr = 0; pr < 4; pr++)
#pragma unroll
                for (int j = 0; j < NC; j++) {
                    const v2f_t t = x[pr][j] * sc[pr] + bi[pr], u = t * p.act0;
                    x[pr][j] = (v2f_t){ act_max(t.x, u.x, act_floor(p.act0)), act_max(t.y, u.y, act_floor(p.act0)) };
                }
        }
        // the next step's rows: 2r+1 becomes the carried one, 2r+2 and 2r+3 are fetched during the block's arithmetic
        if (r < y1 && r + 1 >= 0 && r + 1 < p.H) { load_irow(2 * r + 2, N0); load_irow(2 * r + 3, C); }   // N1 is the next step's carried row
        __builtin_amdgcn_sched_barrier(0);
        // ---- the block: expanded row r finishes output row r - 1, continues r, starts r + 1
        v2f_t o[OCP / 2][NC];
#pragma unroll
        for (int k = 0; k < OCP / 2; k++)
#pragma unroll
            for (int j = 0; j < NC; j++) o[k][j] = z2;
#pragma unroll
        for (int cp = 0; cp < CP; cp++) {
            const W1T c1 = ld1(cp);                                 // (no read-ahead of the tables here: the registers are needed)
            __builtin_amdgcn_sched_barrier(0);
            auto w1p = [&](int j) { return (j & 1) ? (v2f_t){ c1.q[j >> 1].z, c1.q[j >> 1].w } : (v2f_t){ c1.q[j >> 1].x, c1.q[j >> 1].y }; };
            v2f_t win[NC + 2];
            if (rin) {
#pragma unroll
                for (int j = 0; j < NC; j++) {
                    v2f_t a = w1p(0) * x[0][j].x;
#pragma unroll
                    for (int ci = 1; ci < IC; ci++) a += w1p(ci) * ((ci & 1) ? x[ci >> 1][j].y : x[ci >> 1][j].x);
                    a = a * w1p(IC) + w1p(IC + 1);
                    const v2f_t u = a * p.act1;
                    win[1 + j] = (v2f_t){ act_max(a.x, u.x, act_floor(p.act1)), act_max(a.y, u.y, act_floor(p.act1)) };
                }
            } else {
#pragma unroll
                for (int j = 0; j < NC; j++) win[1 + j] = z2;
            }
            __builtin_amdgcn_sched_barrier(0);
            const WDT cd = ldd(cp);
            auto wdp = [&](int j) { return (j & 1) ? (v2f_t){ cd.q[j >> 1].z, cd.q[j >> 1].w } : (v2f_t){ cd.q[j >> 1].x, cd.q[j >> 1].y }; };
            win[0] = (v2f_t){ dpp_shr1(win[NC].x), dpp_shr1(win[NC].y) };
            v2f_t sr = { dpp_shl1(win[1].x), dpp_shl1(win[1].y) };
            if (NC == 3 && sl) {                                      // the seam: the slid last lane takes its neighbour's column NC - 1 - sl as left column, the neighbour the last lane's column sl as right one
                const v2f_t lsrc = sl == 2 ? win[1] : win[2], rsrc = sl == 2 ? win[3] : win[2];      // columns NC - 1 - sl and sl (sl = 1, 2)
                const v2f_t la = { dpp_shr1(lsrc.x), dpp_shr1(lsrc.y) };
                const v2f_t ra = { dpp_shl1(rsrc.x), dpp_shl1(rsrc.y) };
                win[0] = (v2f_t){ last_col ? la.x : win[0].x, last_col ? la.y : win[0].y };
                sr = (v2f_t){ seam_l ? ra.x : sr.x, seam_l ? ra.y : sr.y };
            }
            win[NC + 1] = (v2f_t){ last_col ? 0.f : sr.x, last_col ? 0.f : sr.y };
            __builtin_amdgcn_sched_barrier(0);
            if (fin) {
#pragma unroll
                for (int j = 0; j < NC; j++) {
                    v2f_t d = A[P][cp][j];
                    d += wdp(6) * win[j]; d += wdp(7) * win[j + 1]; d += wdp(8) * win[j + 2];
                    d = d * wdp(9) + wdp(10);
                    const v2f_t u = d * p.actd;
                    d = (v2f_t){ act_max(d.x, u.x, act_floor(p.actd)), act_max(d.y, u.y, act_floor(p.actd)) };
#pragma unroll
                    for (int k = 0; k < OCP / 2; k++) {
                        const v4f &wa = cd.w2[k >> 1], &wb = cd.w2[(OCP / 2 + k) >> 1];
                        const v2f_t w2a = (k & 1) ? (v2f_t){ wa.z, wa.w } : (v2f_t){ wa.x, wa.y };
                        const v2f_t w2b = ((OCP / 2 + k) & 1) ? (v2f_t){ wb.z, wb.w } : (v2f_t){ wb.x, wb.y };
                        o[k][j] += w2a * d.x;
                        o[k][j] += w2b * d.y;
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < NC; j++) {
                v2f_t m = A[P ^ 1][cp][j];
                m += wdp(3) * win[j]; m += wdp(4) * win[j + 1]; m += wdp(5) * win[j + 2];
                A[P ^ 1][cp][j] = m;
                v2f_t s = wdp(0) * win[j];
                s += wdp(1) * win[j + 1]; s += wdp(2) * win[j + 2];
                A[P][cp][j] = s;
            }
#pragma unroll
            for (int j = 0; j < NC; j++) asm volatile("" : "+v"(A[0][cp][j]), "+v"(A[1][cp][j]));
            if (fin) {
#pragma unroll
                for (int k = 0; k < OCP / 2; k++)
#pragma unroll
                    for (int j = 0; j < NC; j++) asm volatile("" : "+v"(o[k][j]));
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (fin && on) {
            v4f sb[2 * OCP / 4];
#pragma unroll
            for (int j = 0; j < 2 * OCP / 4; j++) sb[j] = *reinterpret_cast<const v4f *>(tsb + 4 * j);
#pragma unroll
            for (int k = 0; k < OC / 2; k++) {
                const v4f &sq = sb[k >> 1], &bq = sb[(OCP / 2 + k) >> 1];
                const v2f_t sc = (k & 1) ? (v2f_t){ sq.z, sq.w } : (v2f_t){ sq.x, sq.y };
                const v2f_t bi = ((OCP / 2 + k) & 1) ? (v2f_t){ bq.z, bq.w } : (v2f_t){ bq.x, bq.y };
                v2f_t v[NC];
#pragma unroll
                for (int j = 0; j < NC; j++) {
                    const v2f_t t = o[k][j] * sc + bi, u = t * p.act2;
                    v[j] = (v2f_t){ act_max(t.x, u.x, act_floor(p.act2)), act_max(t.y, u.y, act_floor(p.act2)) };
                }
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    float *dst = op + ((2 * k + h) * cs + (unsigned)(r - 1) * p.W + lo);
                    if constexpr (NC == 4) *reinterpret_cast<v4f *>(dst) = (v4f){ v[0][h], v[1][h], v[2][h], v[3][h] };
                    else { typedef float v3a4 __attribute__((ext_vector_type(3), aligned(4))); *reinterpret_cast<v3a4 *>(dst) = (v3a4){ v[0][h], v[1][h], v[2][h] }; }
                }
            }
        }
    };
    int r = y0 - 1;
    for (; r < y1; r += 2) {
        step(r, std::integral_constant<int, 0>());
        step(r + 1, std::integral_constant<int, 1>());
    }
    if (r == y1) step(r, std::integral_constant<int, 0>());
}
