// ffgpu_conv_igemm.inc -- dense (groups == 1) K x K convolution as an IMPLICIT GEMM on v_mfma_f32_32x32x2_f32.
//
// The reference's conv-v2.c lowers every convolution to im2col + GEMM: im2col writes a [K][oh*ow] column buffer
// (K = fs*fs*ic, conv-v2.c:7-33), the filter rows are repacked densely (conv-v2.c:63-74) and a naive GEMM
// out[c][n] = sum_h col[h][n] * W[c][h] follows (conv-v2.c:77-87).  Here the column buffer is never materialised: the
// K x pixels operand tile is GATHERED from the input tensor straight into LDS in the MFMA operand layout, with the zero
// padding applied on the way (the reference skips out-of-range taps, conv-v0.c:16-21: adding their zero products is the
// same sum).  K runs in the reference's order (input channel, tap row, tap column), so each output is the same k-ordered
// fp32 fmaf chain as the reference's loop.  Any filter size, stride, padding; any input strides (CNHW tensors or the
// frame-major batch input, also through the executor's parameter block); output CNHW.  Grouped convolutions (conv-v0.c:46-51)
// with at least 8 channels per group run as one launch per group on the group's channel / filter / output slices.
//
// Same skeleton as ffgpu_pw_gemm32.inc (workgroup of 4 waves, wave tile 64 channels x 64 pixels = 2 x 2 accumulator
// tiles, chunks of 16 k, two LDS buffers, operands of the next pair of k-steps prefetched into registers), with
//   WM = 2: workgroup tile 128 channels x 128 pixels (2 x 2 waves)       -- layers with more than 64 filters
//   WM = 1: workgroup tile  64 channels x 256 pixels (1 x 4 waves)       -- fewer filters: no matrix rows wasted on padding
// The gather: a thread owns ONE pixel of the tile for the whole K loop (its frame / row / column are decoded once) and, per
// chunk, 16 * TN / 256 rows k of it.  k is wave-uniform, so (ci, ky, kx) and the tap's offset ci * cs + ky * iw + kx are
// scalar arithmetic; per element the lane adds that offset to its pixel's base address, tests the two coordinates against the
// plane and loads 4 bytes -- unconditionally, from a clamped address, zeroed afterwards (a load under a lane predicate is
// waited for on the spot by hipcc).  Consecutive lanes are consecutive pixels of an output row: coalesced for stride 1.
// Round 3 -- the 3x3 / stride 1 / pad 1 form (VEC, what every darknet backbone is made of; needs ow % 4 == 0): the scalar gather
// above issues one 4-byte load, one 4-byte LDS write and ~7 address / predicate instructions per operand element, and that -- not
// the matrix pipe -- bounds the kernel (0.13-0.34 of the fp32 matrix peak).  Here a thread owns a QUAD of four consecutive output
// pixels of one row and, per chunk, whole (input channel, tap row) pairs: the quad's four input columns arrive as ONE aligned
// 16-byte load, the column to their left and right as two 4-byte loads, and the three tap columns kx = 0, 1, 2 leave as three
// 16-byte LDS writes -- 3 loads and 3 writes for 12 operand elements instead of 12 and 12.  K runs in chunks of 24 (= 8 pairs x 3
// taps) in the same (ci, ky, kx) order, so every output still is the reference's k-ordered fmaf chain.
struct IgemmP {
    const float *in; const float *const *in_ind; float *out; const float *residual; const float *wpack;
    long P;                      // output pixels per channel = N * oh * ow
    long ntn;                    // pixel tiles
    long in_cs, in_ns;           // input strides in floats (channel, frame)
    long in_off;                 // first input channel of this group, in floats (added behind the parameter-block indirection)
    int  N, iw, ih, ic, ow, oh, oc, fs, stride, pad;
    int  K, nchunks, ntm, img;   // K = fs * fs * ic; img = floats per channel tile in the packed image
    int  act, res_act, per_xcd;
    unsigned m_ff, m_f;          // ceil(2^32 / (fs * fs)), ceil(2^32 / fs) for k -> (ci, ky, kx) (exact: k * fs * fs < 2^32); 0 when the divisor is 1
    long Pp; int owp;            // VEC: the tile's pixel space has every output row padded to owp = ALIGN(ow, 4) columns (Pp = N oh owp):
                                 // quads never straddle rows, whatever the width (13 x 13, 26 x 26 planes of a 416-pixel darknet input)
    int  nsplit;                 // split-K (round 3): workgroup (tile, s) walks chunks [s nchunks / nsplit, (s + 1) nchunks / nsplit) and, for
    float *part;                 // nsplit > 1, leaves its raw sums in part[group][s][oc][P]; k_conv_igemm_reduce adds them in split order
    // grouped layers (conv-v0.c:46-51: group g = input channels / filters / outputs [g n / G, (g + 1) n / G)): ALL groups in one grid (round 5; a
    // launch per group left a 16-group layer at 16 launches of a sixteenth of the chip each).  Per-group strides in floats; oc, ic, K above are per group
    int  groups;
    long g_in, g_out, g_w;       // in: gic * in_cs; out / residual: goc * P; packed image: img * ntm
};

constexpr int IG_KC = 16, IG_KC3 = 24, IG_KC3N = 12;   // k per chunk: scalar gather; quad gather (8 pairs x 3 taps); quad gather of the 64-channel tile (4 pairs: 31 KB of LDS, three workgroups per CU)

// packed image per channel tile mt (TM = 64 WM channels), per chunk c: [s = 0..7][wm = 0..WM-1][lane][rr = 0..1] =
// W[TM mt + 32 (2 wm + rr) + (lane & 31)][16 c + 2 s + (lane >> 5)] (zero beyond oc / K), then [TM][2] scale', bias'
struct IgemmPackP { const float *filt; float *pk; int K, k4, oc, nchunks, ntm, WM, kc; };
__global__ void k_conv_igemm_pack(IgemmPackP p)
{
    const int TM = 64 * p.WM, cf = (p.kc / 2) * p.WM * 128, img = p.nchunks * cf + 2 * TM, total = img * p.ntm, rl = p.k4 + 4;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int mt = i / img, j = i - mt * img;
        float v = 0.f;
        if (j < p.nchunks * cf) {
            const int c = j / cf, r = j - c * cf;
            const int rr = r & 1, l = (r >> 1) & 63, wm = (r >> 7) % p.WM, s = (r >> 7) / p.WM;
            const int o = TM * mt + 32 * (2 * wm + rr) + (l & 31), k = p.kc * c + 2 * s + (l >> 5);
            if (o < p.oc && k < p.K) v = p.filt[(long)o * rl + k];
        } else {
            const int q = j - p.nchunks * cf, o = TM * mt + (q >> 1);
            if (o < p.oc) v = p.filt[(long)o * rl + p.k4 + (q & 1)];
        }
        p.pk[i] = v;
    }
}

// HALF (WM == 1 only): layers with at most 32 filters -- the upper 32 rows of the 64-row tile would be padding: their MFMAs, operand
// reads and epilogue rows are left out
template <int WM, bool VEC, bool HALF = false>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) k_conv_igemm(IgemmP p)
{
    constexpr int NR = HALF ? 1 : 2;                  // 32-row blocks per wave
    constexpr int IG_KC = VEC ? (WM == 1 ? IG_KC3N : IG_KC3) : ::IG_KC;     // k per chunk
    constexpr int WN = 4 / WM, TM = 64 * WM, TN = 64 * WN;
    constexpr int BROW = TN + 4;                      // pixel-operand row pitch in floats (+16 bytes: the half-waves of a read hit different banks)
    constexpr int ACH = (IG_KC / 2) * WM * 128, BCH = IG_KC * BROW;
    constexpr int NA = (ACH / 4 + 255) / 256;         // 16-byte weight loads per thread and chunk (1 - 3; the last one may be partial)
    constexpr bool NA_RAGGED = (ACH / 4) % 256 != 0;
    constexpr int NE = VEC ? 1 : IG_KC * TN / 256;    // gathered elements per thread and chunk (8 or 16)
    constexpr int NT = (IG_KC / 3) * (TN / 4) / 256;  // VEC: (channel, tap row) pairs per thread and chunk (1 or 2)
    constexpr int KSTEP = 256 / TN;                   // k rows covered by one pass of the workgroup (2 or 1)
    typedef float v2f __attribute__((ext_vector_type(2)));
    typedef float v4 __attribute__((ext_vector_type(4)));
    typedef float v16 __attribute__((ext_vector_type(16)));
    __shared__ __attribute__((aligned(16))) float smem[2 * ACH + 2 * BCH + 2 * TM];
    float (*sA)[ACH] = reinterpret_cast<float (*)[ACH]>(smem);
    float (*sB)[BCH] = reinterpret_cast<float (*)[BCH]>(smem + 2 * ACH);
    float *sSB = smem + 2 * ACH + 2 * BCH;

    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = WM == 2 ? wid >> 1 : 0, wn = WM == 2 ? wid & 1 : wid;
    const long total = (long)p.ntm * p.ntn * p.nsplit;                                 // per group
    const long tile_g = (long)(blockIdx.x & 7) * p.per_xcd + (blockIdx.x >> 3);        // XCD-aware order (see ffgpu_pw_gemm32.inc)
    if ((int)(blockIdx.x >> 3) >= p.per_xcd || tile_g >= total * p.groups) return;
    const int grp = (int)(tile_g / total);
    const long tile_s = tile_g - (long)grp * total;
    float *const g_outp = p.out + (long)grp * p.g_out;
    const float *const g_res = p.residual ? p.residual + (long)grp * p.g_out : nullptr;
    const long tile = tile_s / p.nsplit;
    const int ks = (int)(tile_s - tile * p.nsplit);                                    // this workgroup's part of K
    const int cb = (int)((long)ks * p.nchunks / p.nsplit), ce = (int)((long)(ks + 1) * p.nchunks / p.nsplit);
    const int mt = (int)(tile % p.ntm);
    const long p0 = (tile / p.ntm) * TN;
    const float *wimg = p.wpack + (size_t)grp * p.g_w + (size_t)mt * p.img;
    for (int i = tid; i < 2 * TM; i += 256) sSB[i] = wimg[p.nchunks * ACH + i];
    const gfp in0 = to_global(p.in_ind ? *p.in_ind : p.in) + p.in_off + (long)grp * p.g_in;        // (global, not flat: see ffgpu_kernels.hip)

    // this thread's pixel of the tile: frame n, output row / column -> base address of tap (0, 0) and its coordinates
    const int pxl = tid % TN, krow0 = __builtin_amdgcn_readfirstlane(tid / TN);
    const long pg = p0 + pxl;
    const bool pvalid = pg < p.P;
    const unsigned pgu = (unsigned)(pvalid ? pg : 0);                                 // P < 2^31 (launcher)
    const unsigned n = pgu / (unsigned)(p.oh * p.ow), rem = pgu - n * (unsigned)(p.oh * p.ow);      // once per thread
    const unsigned oy = rem / (unsigned)p.ow, ox = rem - oy * (unsigned)p.ow;
    const int iy0 = (int)oy * p.stride - p.pad, ix0 = (int)ox * p.stride - p.pad;
    const gfp pbase = in0 + (long)n * p.in_ns + (long)iy0 * p.iw + ix0;             // may point before the plane: only dereferenced when in range
    const int ff = p.fs * p.fs;

    v4 ra[NA];
    float rb[NE];
    // VEC: this thread's quad (four consecutive pixels of one output row in the row-padded pixel space) and the
    // (ci, ky) pairs m = 8 c + mrow0 + MSTEP j of every chunk c.  A quad that reaches past the row's end (width not a multiple
    // of 4) loads the row's LAST four columns instead and shifts them into place (qsh): no access outside the row.
    constexpr int NQ = TN / 4, MSTEP = 256 / NQ;      // quads per tile (32 / 64), pairs covered by one pass of the workgroup (8 / 4)
    const int qd = tid % NQ, mrow0 = tid / NQ;        // (per lane: with 32 quads per tile the two halves of a wave take different pairs)
    v4 rc[VEC ? NT : 1]; float rl[VEC ? NT : 1], rr[VEC ? NT : 1];
    gfp qbase = in0; int qy0 = 0, qx0 = 0, qsh = 0; bool qvalid = false;
    const bool ragged_w = VEC && p.owp != p.ow;                                          // uniform
    if (VEC) {
        const long qg = p0 + 4 * qd;
        qvalid = qg < p.Pp;
        const unsigned qgu = (unsigned)(qvalid ? qg : 0);
        const unsigned qn = qgu / (unsigned)(p.oh * p.owp), qrem = qgu - qn * (unsigned)(p.oh * p.owp);
        const unsigned qoy = qrem / (unsigned)p.owp, qox = qrem - qoy * (unsigned)p.owp;
        qy0 = (int)qoy - 1; qx0 = (int)qox;                                             // input row of tap row 0; input column of the quad's first pixel
        const int qa = min(qx0, p.iw - 4);                                              // first column actually loaded
        qsh = qx0 - qa;                                                                 // 0, or 1..3 for the row's last, partial quad
        qbase = in0 + (long)qn * p.in_ns + qa;
    }
    auto gload = [&](int c) {
#pragma unroll
        for (int j = 0; j < NA; j++)
            if (!NA_RAGGED || j + 1 < NA || tid + 256 * j < ACH / 4) ra[j] = reinterpret_cast<const v4 *>(wimg + (size_t)c * ACH)[tid + 256 * j];
        if (VEC) {
#pragma unroll
            for (int j = 0; j < NT; j++) {
                const int m = (IG_KC / 3) * c + mrow0 + MSTEP * j;                      // (ci, ky) = (m / 3, m % 3)
                const unsigned ci = __umulhi((unsigned)m, 0x55555556u), ky = (unsigned)m - 3u * ci;
                const int iy = qy0 + (int)ky;
                const bool ok = qvalid && 3 * m < p.K && (unsigned)iy < (unsigned)p.ih;
                const gfp rowc = ok ? qbase + (long)ci * p.in_cs + (long)iy * p.iw : in0;          // unconditional loads from a valid address
                typedef v4 v4a4 __attribute__((aligned(4)));                                      // (ragged widths: a row starts at any dword)
                v4 t = gld<v4a4>(rowc);
                const bool okl = ok && qx0 > 0 && qsh == 0, okr = ok && qx0 + 4 < p.iw;   // (a shifted quad finds its left neighbour in t, and has none to the right)
                const float vl = *(okl ? rowc - 1 : rowc), vr = *(okr ? rowc + 4 : rowc);
                if (!ok) t = (v4){ 0.f, 0.f, 0.f, 0.f };
                float L = okl ? vl : 0.f;
                if (ragged_w) {
                    if (qsh) L = qsh == 1 ? t.x : (qsh == 2 ? t.y : t.z);
                    if (qsh == 1) t = (v4){ t.y, t.z, t.w, 0.f }; else if (qsh == 2) t = (v4){ t.z, t.w, 0.f, 0.f }; else if (qsh == 3) t = (v4){ t.w, 0.f, 0.f, 0.f };
                }
                rc[j] = t;
                rl[j] = L; rr[j] = okr ? vr : 0.f;
            }
            return;
        }
#pragma unroll
        for (int j = 0; j < NE; j++) {
            const int k = IG_KC * c + krow0 + KSTEP * j;                                // wave-uniform
            const unsigned ci = p.m_ff ? __umulhi((unsigned)k, p.m_ff) : (unsigned)k, t = (unsigned)k - ci * (unsigned)ff;
            const unsigned ky = p.m_f ? __umulhi(t, p.m_f) : t, kx = t - ky * (unsigned)p.fs;
            const long koff = (long)ci * p.in_cs + (long)ky * p.iw + kx;                // scalar
            const bool ok = pvalid && k < p.K && (unsigned)(iy0 + (int)ky) < (unsigned)p.ih && (unsigned)(ix0 + (int)kx) < (unsigned)p.iw;
            const gfp src = ok ? pbase + koff : in0;                                 // unconditional load from a valid address
            const float v = *src;
            rb[j] = ok ? v : 0.f;
        }
    };
    auto lstore = [&](auto BUF) {
        constexpr int buf = decltype(BUF)::value;
#pragma unroll
        for (int j = 0; j < NA; j++)
            if (!NA_RAGGED || j + 1 < NA || tid + 256 * j < ACH / 4) reinterpret_cast<v4 *>(sA[buf])[tid + 256 * j] = ra[j];
        if (VEC) {
#pragma unroll
            for (int j = 0; j < NT; j++) {
                float *dst = &sB[buf][3 * (mrow0 + MSTEP * j) * BROW + 4 * qd];          // rows k = 3 m', 3 m' + 1, 3 m' + 2 of the chunk
                *reinterpret_cast<v4 *>(dst) = (v4){ rl[j], rc[j].x, rc[j].y, rc[j].z };                 // kx = 0: columns x - 1 .. x + 2
                *reinterpret_cast<v4 *>(dst + BROW) = rc[j];                                             // kx = 1
                *reinterpret_cast<v4 *>(dst + 2 * BROW) = (v4){ rc[j].y, rc[j].z, rc[j].w, rr[j] };      // kx = 2
            }
            return;
        }
#pragma unroll
        for (int j = 0; j < NE; j++) sB[buf][(krow0 + KSTEP * j) * BROW + pxl] = rb[j];
    };

    v16 acc[2][2];
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[r][j][e] = 0.f;

    gload(cb);
    lstore(std::integral_constant<int, 0>{});
    __syncthreads();
    const int aoff = (wm * 64 + lane) * 2;                            // + s * WM * 128
    const int boff = (lane >> 5) * BROW + wn * 64 + 2 * (lane & 31);  // + 2 s * BROW: pixels 2n, 2n + 1 feed accumulator tiles 0, 1
    auto chunk = [&](int c, auto BUF) {
        constexpr int buf = decltype(BUF)::value;
        const bool more = c + 1 < ce;
        if (more) gload(c + 1);                                       // in flight during this chunk's MFMAs
        const float *A = sA[buf] + aoff, *B = sB[buf] + boff;
        v2f fa[2][2], fb[2][2];
        auto lread = [&](int q, int s2) {
#pragma unroll
            for (int h = 0; h < 2; h++) {
                fa[q][h] = *reinterpret_cast<const v2f *>(A + (2 * s2 + h) * (WM * 128));
                fb[q][h] = *reinterpret_cast<const v2f *>(B + 2 * (2 * s2 + h) * BROW);
            }
        };
        lread(0, 0);
#pragma unroll
        for (int s2 = 0; s2 < IG_KC / 4; s2++) {
            if (s2 + 1 < IG_KC / 4) lread((s2 + 1) & 1, s2 + 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int h = 0; h < 2; h++)
#pragma unroll
                for (int r = 0; r < NR; r++)
#pragma unroll
                    for (int j = 0; j < 2; j++)
                        acc[r][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[s2 & 1][h][r], fb[s2 & 1][h][j], acc[r][j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (more) lstore(std::integral_constant<int, buf ^ 1>{});
        __syncthreads();
    };
    for (int c = cb; c < ce; c += 2) {
        chunk(c, std::integral_constant<int, 0>{});
        if (c + 1 < ce) chunk(c + 1, std::integral_constant<int, 1>{});
    }

    // epilogue: C/D map of 32x32: col = lane & 31 (pixel pair 2 col, 2 col + 1 across the two tiles), row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
    const float slope = p.act == 2 ? 0.1f : (p.act == 1 ? 0.f : 1.f), rslope = p.res_act == 2 ? 0.1f : (p.res_act == 1 ? 0.f : 1.f);
    long px = p0 + wn * 64 + 2 * (lane & 31);
    if (px >= (VEC ? p.Pp : p.P)) return;
    bool two = px + 1 < p.P;
    if (VEC && p.owp != p.ow) {                                       // padded pixel space -> the real one (the pair 2c, 2c + 1 lies in one row)
        const unsigned rowi = (unsigned)px / (unsigned)p.owp, x = (unsigned)px - rowi * (unsigned)p.owp;
        if ((int)x >= p.ow) return;
        two = (int)x + 1 < p.ow;
        px = (long)rowi * p.ow + x;
    }
    const bool pair = two && !(p.P & 1) && !(p.ow & 1);               // 8-byte store: both pixels exist and every pair starts 8-byte aligned
    auto act1 = [&](float t, int a, float sl) { return a == 3 ? 1.0f / (1.0f + (float)exp((double)-t)) : act_max(t, sl * t, act_floor(sl)); };
    if (p.nsplit > 1) {                                               // raw partial sums; scale', bias', activation and residual follow in the reduction
        float *part = p.part + ((size_t)grp * p.nsplit + ks) * p.oc * p.P;
#pragma unroll
        for (int r = 0; r < NR; r++)
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const int o = TM * mt + 32 * (2 * wm + r) + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
                if (o >= p.oc) continue;
                const long off = (long)o * p.P + px;
                if (pair) *reinterpret_cast<v2f *>(part + off) = (v2f){ acc[r][0][e], acc[r][1][e] };
                else { part[off] = acc[r][0][e]; if (two) part[off + 1] = acc[r][1][e]; }
            }
        return;
    }
#pragma unroll
    for (int r = 0; r < NR; r++)
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const int ol = 32 * (2 * wm + r) + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5), o = TM * mt + ol;
            if (o >= p.oc) continue;
            const float sc = sSB[2 * ol], bi = sSB[2 * ol + 1];
            float v0 = act1(fmaf(acc[r][0][e], sc, bi), p.act, slope), v1 = act1(fmaf(acc[r][1][e], sc, bi), p.act, slope);
            const long off = (long)o * p.P + px;
            if (g_res) {
                v0 = act1(v0 + g_res[off], p.res_act, rslope);
                if (two) v1 = act1(v1 + g_res[off + 1], p.res_act, rslope);
            }
            if (pair) *reinterpret_cast<v2f *>(g_outp + off) = (v2f){ v0, v1 };
            else { g_outp[off] = v0; if (two) g_outp[off + 1] = v1; }
        }
}

// split-K reduction: out[o][px] = act(scale' * (part[0] + part[1] + ...)[o][px] + bias') (+ residual) -- the splits added in order
// (deterministic; the sum is no longer ONE k-ordered fmaf chain but nsplit of them: same tolerance class, stated in the tests)
struct IgemmRedP { const float *part; const float *filt; const float *residual; float *out; long P; int oc, goc, nsplit, rl, k4, act, res_act; };
__global__ void __launch_bounds__(256) k_conv_igemm_reduce(IgemmRedP p)
{
    // (all groups at once: output channel o = goc g + ol of the contiguous oc x P tensor; part[g][s][ol][px])
    const long total = (long)p.oc * p.P, gsz = (long)p.goc * p.P;
    const float slope = p.act == 2 ? 0.1f : (p.act == 1 ? 0.f : 1.f), rslope = p.res_act == 2 ? 0.1f : (p.res_act == 1 ? 0.f : 1.f);
    auto act1 = [&](float t, int a, float sl) { return a == 3 ? 1.0f / (1.0f + (float)exp((double)-t)) : act_max(t, sl * t, act_floor(sl)); };
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int o = (int)(i / p.P), g = o / p.goc;
        const float *part = p.part + (size_t)g * p.nsplit * gsz + (i - (long)g * gsz);
        float v = part[0];
        for (int s = 1; s < p.nsplit; s++) v += part[(size_t)s * gsz];
        v = act1(fmaf(v, p.filt[(long)o * p.rl + p.k4], p.filt[(long)o * p.rl + p.k4 + 1]), p.act, slope);
        if (p.residual) v = act1(v + p.residual[i], p.res_act, rslope);
        p.out[i] = v;
    }
}
