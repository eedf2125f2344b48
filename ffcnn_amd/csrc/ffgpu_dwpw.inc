// ffgpu_dwpw.inc -- depthwise K x K (stride 1, "same" padding) followed by a pointwise 1 x 1 convolution in ONE kernel:
// the detection heads' pairs of yolo-fastest (layers 116+117, 118+119 on 10x10 planes; 125+126, 127+128 on 20x20), i.e.
// two consecutive groupconv calls of the reference (conv-v6.c:291-465 resp. conv-v0.c:7-31 for the depthwise -- the CORRECT
// 5x5, not conv-v6.c's row omission -- and conv-v6.c:46-91 for the pointwise).  The depthwise result never leaves the CU:
// it is written to LDS in the MFMA B-operand layout and consumed by v_mfma_f32_16x16x4_f32 (exact fp32, k-ordered).
//
//   workgroup (4 waves) = one tile of TW x TH <= 128 pixels of one frame, all C channels in, all OC channels out
//   LDS: the pointwise weights as A fragments (plan-time packed image, copied once: C / 4 x NRT x 64 floats), the taps +
//        scale' / bias' of every depthwise channel, one halo tile of KC = 8 channels, two B tiles [8][TP]
//   per chunk of 8 channels:  halo tile (zero padded, prefetched into registers one chunk ahead) -> LDS | barrier |
//        depthwise: an item = (channel, tile row, x segment), taps summed in the reference's order w0..w(K*K-1),
//        scale' / bias' / activation, result -> B tile | barrier | 2 k-steps of MFMAs: wave w owns pixel tiles w, w + 4
//        and all NRT channel tiles (the next chunk's depthwise overlaps other waves' MFMAs: B tiles are double-buffered)
//   epilogue: C/D map of 16x16 (col = lane & 15 = pixel, row = 4 (lane >> 4) + i = channel), scale' / bias' / activation
// Accumulation order per output = the reference's (depthwise: tap row, tap column; pointwise: input channel ascending).
struct DwPwP {
    const float *in; float *out;
    const float *wd;             // depthwise filter rows [C][k4d + 4]
    const float *wpack;          // pointwise weights as A fragments (k_dwpw_pack)
    int N, W, H, C, OC;
    int TW, TH, TP, TPS;         // tile, pixels per tile, B-tile row pitch in floats (>= 16 NCT, padded)
    int ntx, nty;                // tiles per plane
    int HW_, HH_;                // halo tile width / height = TW + FS - 1, TH + FS - 1
    int NRT, NCT, nchunks;       // channel tiles of 16 (<= 8), pixel tiles of 16 (<= 8), chunks of 8 channels
    int XS, SEG;                 // x segments per tile row and their length
    int rld;                     // depthwise filter row length
    float slope_d, slope_p;      // activations as max(x, slope x)
};

// A-fragment image of the pointwise layer: [k-step = 0 .. 2 nchunks)[channel tile r < NRT][lane] = W[16 r + (lane & 15)][4 ks + (lane >> 4)]
// (zero beyond OC / C), then [16 NRT][2] scale', bias'
struct DwPwPackP { const float *filt; float *pk; int C, OC, NRT, nchunks; };
__global__ void k_dwpw_pack(DwPwPackP p)
{
    const int ks2 = 2 * p.nchunks, frag = ks2 * p.NRT * 64, total = frag + p.NRT * 32, k4 = (p.C + 3) & ~3, rl = k4 + 4;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        float v = 0.f;
        if (i < frag) {
            const int l = i & 63, r = (i >> 6) % p.NRT, ks = (i >> 6) / p.NRT;
            const int o = 16 * r + (l & 15), ci = 4 * ks + (l >> 4);
            if (o < p.OC && ci < p.C) v = p.filt[(long)o * rl + ci];
        } else {
            const int q = i - frag, o = q >> 1;
            if (o < p.OC) v = p.filt[(long)o * rl + k4 + (q & 1)];
        }
        p.pk[i] = v;
    }
}

template <int FS, int SG>          // SG: compile-time bound of the segment length (4 or 8)
__global__ void __launch_bounds__(256) k_dwpw(DwPwP p)
{
    constexpr int KC = 8, FF = FS * FS, R = FS / 2, TAPW = FF + 3;   // taps, scale', bias' (+1: odd pitch, conflict-free broadcast rows)
    typedef float v4 __attribute__((ext_vector_type(4)));
    extern __shared__ __attribute__((aligned(16))) float dp_s[];
    const int ksteps = 2 * p.nchunks;
    const int aimg = ksteps * p.NRT * 64 + p.NRT * 32;               // A fragments, then [NRT * 16][2] scale', bias'
    float *sA = dp_s;
    float *sTap = sA + ((aimg + 3) & ~3);                            // [nchunks * 8][TAPW]
    float *sIn = sTap + ((p.nchunks * KC * TAPW + 3) & ~3);          // [8][HH_ * HW_]
    const int halo = p.HW_ * p.HH_;
    float *sB = sIn + ((KC * halo + 3) & ~3);                        // [2][8][TPS]

    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tiles = p.ntx * p.nty;
    const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
    const int ty0 = (t / p.ntx) * p.TH, tx0 = (t % p.ntx) * p.TW;
    const long plane = (long)p.W * p.H, cs = (long)p.N * plane;

    // one-off: pointwise A fragments, depthwise taps
    for (int i = tid; i < aimg / 4; i += 256) reinterpret_cast<v4 *>(sA)[i] = reinterpret_cast<const v4 *>(p.wpack)[i];
    for (int i = tid; i < p.nchunks * KC * TAPW; i += 256) {
        const int c = i / TAPW, j = i - c * TAPW;
        float v = 0.f;
        if (c < p.C && j < FF + 2) v = p.wd[(long)c * p.rld + (j < FF ? j : p.rld - 4 + (j - FF))];
        sTap[i] = v;
    }

    // halo gather: element e of a chunk = (channel e / halo, position e % halo); NLD elements per thread
    constexpr int NLD = 8;                                           // 8 * 256 >= 8 * halo  <=>  halo <= 256 (launcher)
    const float *inb = p.in + (long)n * plane;
    auto decode = [&](int e, int &ch, int &off, bool &ok) {
        ch = e / halo;
        const int q = e - ch * halo, hy = q / p.HW_, hx = q - hy * p.HW_;
        const int y = ty0 + hy - R, x = tx0 + hx - R;
        ok = ch < KC && (unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W;
        off = ok ? y * p.W + x : 0;
    };
    int gch[NLD], gq[NLD], goff[NLD]; bool gok[NLD];
#pragma unroll
    for (int j = 0; j < NLD; j++) { int ch, off; bool ok; decode(tid + 256 * j, ch, off, ok); gch[j] = ch; goff[j] = off; gok[j] = ok; gq[j] = tid + 256 * j; }
    float rin[NLD];
    auto gload = [&](int c) {
#pragma unroll
        for (int j = 0; j < NLD; j++) {
            const int chg = KC * c + gch[j];
            const bool ok = gok[j] && chg < p.C;
            const float v = inb[ok ? (long)chg * cs + goff[j] : 0];   // unconditional load from a valid address
            rin[j] = ok ? v : 0.f;
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int j = 0; j < NLD; j++) if (gq[j] < KC * halo) sIn[gq[j]] = rin[j];
    };

    // depthwise items of this thread (fixed over the chunks): (channel, row, segment)
    const int items = KC * p.TH * p.XS;
    const bool has_item = tid < items;
    const int ich = tid / (p.TH * p.XS), irem = tid - ich * (p.TH * p.XS), iy = irem / p.XS, ix0 = (irem - iy * p.XS) * p.SEG;
    const int iseg = min(p.SEG, p.TW - ix0);

    v4 acc[8][2];
#pragma unroll
    for (int r = 0; r < 8; r++)
#pragma unroll
        for (int j = 0; j < 2; j++) acc[r][j] = (v4){ 0.f, 0.f, 0.f, 0.f };
    const int nct_w = (p.NCT - wid + 3) / 4;                          // pixel tiles of this wave: wid, wid + 4 (0, 1 or 2)

    gload(0);
    for (int c = 0; c < p.nchunks; c++) {
        lstore();
        __syncthreads();                                             // halo tile of chunk c (and, the first time, the tables) visible
        if (c + 1 < p.nchunks) gload(c + 1);
        float *B = sB + (c & 1) * KC * p.TPS;
        if (has_item && iseg > 0) {
            const float *tp = sTap + (KC * c + ich) * TAPW;
            const float *src = sIn + ich * halo + iy * p.HW_ + ix0;
            float o[SG];
#pragma unroll
            for (int j = 0; j < SG; j++) o[j] = 0.f;
#pragma unroll
            for (int ky = 0; ky < FS; ky++) {
                float row[SG + FS - 1];
#pragma unroll
                for (int j = 0; j < SG + FS - 1; j++) row[j] = j < p.SEG + FS - 1 ? src[ky * p.HW_ + j] : 0.f;
#pragma unroll
                for (int kx = 0; kx < FS; kx++) {
                    const float w = tp[ky * FS + kx];
#pragma unroll
                    for (int j = 0; j < SG; j++) o[j] = fmaf(row[j + kx], w, o[j]);
                }
            }
            const float sc = tp[FF], bi = tp[FF + 1];
#pragma unroll
            for (int j = 0; j < SG; j++)
                if (j < iseg) { const float v = fmaf(o[j], sc, bi); B[ich * p.TPS + iy * p.TW + ix0 + j] = act_max(v, p.slope_d * v, act_floor(p.slope_d)); }
        }
        __syncthreads();                                             // B tile of chunk c complete; everyone is done with the halo tile
        if (nct_w > 0) {
#pragma unroll
            for (int ks = 0; ks < 2; ks++) {
                const float *Bk = B + (4 * ks + (lane >> 4)) * p.TPS + (lane & 15);
                const float b0 = Bk[16 * wid], b1 = nct_w > 1 ? Bk[16 * (wid + 4)] : 0.f;
                const float *Ak = sA + (size_t)((2 * c + ks) * p.NRT) * 64 + lane;
#pragma unroll
                for (int r = 0; r < 8; r++) {
                    if (r < p.NRT) {
                        const float a = Ak[r * 64];
                        acc[r][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0, acc[r][0], 0, 0, 0);
                        if (nct_w > 1) acc[r][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1, acc[r][1], 0, 0, 0);
                    }
                }
            }
        }
    }

    // epilogue: pixel = 16 ct + (lane & 15) of the tile (row-major TW x TH), channel = 16 r + 4 (lane >> 4) + i
    const float *sb = sA + ksteps * p.NRT * 64;
    float *outb = p.out + (long)n * plane;
#pragma unroll
    for (int j = 0; j < 2; j++) {
        if (j >= nct_w) break;
        const int px = 16 * (wid + 4 * j) + (lane & 15);
        if (px >= p.TP) continue;
        const int py = px / p.TW, pxx = px - py * p.TW;
        const int y = ty0 + py, x = tx0 + pxx;
        if (y >= p.H || x >= p.W) continue;
        const long poff = (long)y * p.W + x;
#pragma unroll
        for (int r = 0; r < 8; r++) {
            if (r >= p.NRT) break;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int ol = 16 * r + 4 * (lane >> 4) + i;
                if (ol < p.OC) {
                    const float v = fmaf(acc[r][j][i], sb[2 * ol], sb[2 * ol + 1]);
                    outb[(long)ol * cs + poff] = act_max(v, p.slope_p * v, act_floor(p.slope_p));
                }
            }
        }
    }
}
