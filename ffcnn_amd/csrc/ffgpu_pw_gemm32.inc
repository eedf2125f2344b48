// ffgpu_pw_gemm32.inc -- pointwise convolution for COMPUTE-bound shapes (BASELINE config[2]: 256 -> 512 channels on
// 20x20 planes, batch 256: M = 512, K = 256, N = 102 400, 85 flop/B) as an LDS-tiled GEMM on v_mfma_f32_32x32x2_f32.
// Restates conv-v6.c:46-91 (Out[oc][p] = act(scale' * sum_ci W[oc][ci] In[ci][p] + bias')); exact fp32, k-ordered.
//
// Why 32x32x2 and LDS (the first round's kernel fed v_mfma_f32_16x16x4_f32 straight from global memory and stopped at
// 0.60 of the matrix peak): a 32x32x2 MFMA does twice the flops of a 16x16x4 per operand register, and with the operands
// staged in LDS the inner loop is LDS reads with immediate offsets + MFMAs -- no address arithmetic, no vector-memory waits.
//
//   workgroup = 4 waves as 4 (channels) x 1; workgroup tile 128 output channels x 128 pixels; a wave owns ONE 32-channel row
//   block and all four 32-pixel blocks (4 accumulator tiles of 32 x 32 = 64 accumulator VGPRs, ~100 in all: 4 waves per SIMD);
//   K walked in chunks of KC = 16 channels, two LDS buffers per operand, the next chunk's LDS-DMA (global_load_lds_dwordx4: no
//   staging registers, no ds_write pass) in flight during the current chunk's MFMAs, one barrier per chunk; the input operands of
//   the next pair of k-steps are read from LDS into registers while the 8 MFMAs of the current pair run.
//   A (weights): plan-time packed image in global memory that IS the LDS chunk image ([half chunk][wave][lane][4 k-steps]):
//     a chunk is one linear 8 KB copy, a lane's A operands of four k-steps are one ds_read_b128.
//   B (input):   chunk = KC channel rows x tile pixels, row-major, 512 contiguous bytes per channel row from global memory;
//     a lane reads 4 consecutive pixels of channel 2s + (lane >> 5) with ONE ds_read_b128, and component j feeds accumulator
//     tile j: MFMA column n <-> pixel 4 n + j, so a lane's 4 results of an output row are 4 consecutive pixels -> 16 stores of
//     16 bytes per wave and tile, no transpose anywhere.  (The first form of this kernel had waves 2 x 2 with 64 x 64 wave
//     tiles: pixels 2 n + j, 32 stores of 8 bytes; 220.5 against 218.3 us.)
//   C/D map of 32x32 (cdna_hip_programming.md section 3): col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).
// Tiles are walked in an XCD-aware order: consecutive workgroup ids land on different XCDs (round robin), so the id is
// remapped to give each XCD one contiguous range of tiles -- the M tiles of one pixel strip run on the same L2.
// The last, partial round of workgroups (3200 tiles on 1024 slots: 128 left over, one per CU on half the chip with one wave per
// SIMD) is cut finer: the pixel range it would cover is walked in NARROW tiles of 128 channels x 64 pixels (the same code with
// two pixel blocks per wave), twice as many workgroups with half the work per wave.
// Measured structure of the kernel's time and the variants that lost (pixels as matrix rows, tile turned through LDS for
// 16-byte row stores, staggered starts, wave priorities, 256 x 256 tiles on 16 waves, persistent workgroups with chained
// tiles, packed-math epilogue): DESIGN.md section 5.7.
typedef float v16f_pg __attribute__((ext_vector_type(16)));
typedef float v2f_pg __attribute__((ext_vector_type(2)));

struct PwG32P {
    const float *in; float *out; const float *residual; const float *wpack;
    long P;                      // pixels per channel (P % 4 == 0)
    long ntn;                    // pixel tiles
    int  ic, oc, nchunks;        // nchunks = ceil(ic / 16)
    int  ntm;                    // channel tiles of 32 wm
    int  img;                    // floats per channel tile in the packed image: nchunks * 512 WM + 64 WM
    int  wm;                     // waves (= 32-channel row blocks) per workgroup: 4 (128-channel tiles) or 8 (256-channel tiles)
    int  act, res_act;
    int  per_xcd;                // tiles per XCD range (ceil(total / 8))
    int  dbg;                    // tuning only (wrong results): 1 no global loads / LDS writes in the loop, 2 no barrier, 4 no LDS reads
};

constexpr int PWG_KC = 16;

// packed image: per channel tile mt (TM = 32 WM channels), per chunk c: [h2 = 0..1][wq = 0..WM-1][lane = 0..63][t = 0..3] =
// W[TM mt + 32 wq + (lane & 31)][16 c + 8 h2 + 2 t + (lane >> 5)]
// (zero beyond oc / ic): wave wq's A operands of k-steps 4 h2 .. 4 h2 + 3 are one ds_read_b128; then [TM][2] scale', bias'
struct PwG32PackP { const float *filt; float *pk; int ic, oc, k4, nchunks, ntm, wm; };
__global__ void k_pw_gemm32_pack(PwG32PackP p)
{
    const int ach = 512 * p.wm, tm = 32 * p.wm;
    const int img = p.nchunks * ach + 2 * tm, total = img * p.ntm, rl = p.k4 + 4;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int mt = i / img, j = i - mt * img;
        float v = 0.f;
        if (j < p.nchunks * ach) {
            const int c = j / ach, r = j - c * ach;
            const int t = r & 3, l = (r >> 2) & 63, wq = (r >> 8) % p.wm, h2 = (r >> 8) / p.wm;
            const int o = tm * mt + 32 * wq + (l & 31), k = PWG_KC * c + 8 * h2 + 2 * t + (l >> 5);
            if (o < p.oc && k < p.ic) v = p.filt[(long)o * rl + k];
        } else {
            const int q = j - p.nchunks * ach, o = tm * mt + (q >> 1);
            if (o < p.oc) v = p.filt[(long)o * rl + p.k4 + (q & 1)];
        }
        p.pk[i] = v;
    }
}

// what a padded row of the last, ragged input chunk is loaded from (every lane the same 16 bytes): channels beyond ic count as ZERO.  Their weights are zero
// in the image, but a re-read row of the input would give 0 x Inf = NaN where the reference has no term at all
// (tests/conv_kernels/test_gpu_kernels.py::test_non_finite_inputs[pw_gemm-*])
__device__ __attribute__((aligned(16))) const float pwg_zero_row[4] = { 0.f, 0.f, 0.f, 0.f };

__device__ __noinline__ float pwg_sigmoid(float t) { return 1.0f / (1.0f + (float)exp((double)-t)); }

// one tile of 128 channels x 32 PXB pixels: waves 4 (channels) x 1, a wave owns ONE 32-channel row block and PXB pixel blocks
// (PXB accumulators of 32 x 32).  PXB = 4: the main tile (128 pixels; a lane's results of an output row are 4 consecutive
// pixels: 16 stores of 16 bytes per wave and tile); PXB = 2: the narrow tile of the partial last round (64 pixels, 8-byte stores)
// WM = 8 (round 3; layers with at least 256 filters): 256 channels x 128 pixels on 8 waves.  The input chunk is shared by twice as
// many waves: ONE input piece per wave and chunk instead of two (three LDS-DMA instructions per wave and chunk instead of four --
// their issue, ~70 matrix-pipe cycles each, is what separates the kernel from its MFMA-only time), and every input tile is fetched
// oc / 256 times instead of oc / 128 times.
template <int PXB, int WM>
__device__ __forceinline__ void pwg_tile(const PwG32P &p, float *smem, int mt, long p0)
{
    constexpr int TN = 32 * PXB, PWG_TM = 32 * WM;                    // pixels / channels per tile
    constexpr int ACH = 512 * WM, BCH = PWG_KC * TN;                  // floats per chunk buffer (the LDS images are lane-linear: no padding)
    constexpr int NBP = BCH / 256;                                    // 1 KB input pieces per chunk (8 / 4)
    constexpr int BP = NBP >= WM ? NBP / WM : 1;                      // ... per wave (2 / 1; 8 waves on a narrow tile: waves 0-3 one each)
    constexpr bool BHALF = NBP < WM;
    typedef float v16 __attribute__((ext_vector_type(16)));
    typedef float v4 __attribute__((ext_vector_type(4)));
    typedef float v2 __attribute__((ext_vector_type(2)));
    typedef float vB __attribute__((ext_vector_type(PXB)));
    float (*sA)[ACH] = reinterpret_cast<float (*)[ACH]>(smem);
    float (*sB)[BCH] = reinterpret_cast<float (*)[BCH]>(smem + 2 * ACH);
    float *sSB = smem + 2 * ACH + 2 * PWG_KC * 128;

    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const float *wimg = p.wpack + (size_t)mt * p.img;
    sSB[tid] = wimg[p.nchunks * ACH + tid];                            // 2 TM floats = one per thread

    // LDS-DMA of one chunk: wave w brings pieces 2w, 2w + 1 of the weight chunk (1 KB each, linear) and BP pieces of the input
    // chunk (a piece = 256 floats of the [16][TN] image: 2 channel rows of 128 pixels, or 4 rows of 64).  The inner loop carries
    // as few vector instructions as possible: the input pointers advance by one 64-bit add per chunk, the weight pointer is uniform.
    const float *aptr = wimg;                                         // uniform
    const long bstep = (long)PWG_KC * p.P;
    const float *gb[BP];
    int gbk[BP];
    const bool kragged = (p.ic & (PWG_KC - 1)) != 0;                  // uniform
    const bool bload = !BHALF || wid < NBP;                           // wave-uniform
#pragma unroll
    for (int j = 0; j < BP; j++) {
        const int f = 256 * ((BHALF ? (wid < NBP ? wid : 0) : wid * BP) + j) + 4 * lane;      // this lane's first float inside the chunk image
        gbk[j] = f / TN;
        long px = p0 + f % TN;
        if (px > p.P - 4) px = p.P - 4;                               // ragged last tile: clamped (its results are not stored)
        gb[j] = p.in + px + (long)gbk[j] * p.P;
    }
    typedef __attribute__((address_space(3))) void *lds_t;
    typedef const __attribute__((address_space(1))) void *glb_t;
    auto glds = [&](int c, auto BUF) {
        constexpr int buf = decltype(BUF)::value;
#pragma unroll
        for (int h = 0; h < 2; h++)
            __builtin_amdgcn_global_load_lds((glb_t)(aptr + (wid * 2 + h) * 256 + lane * 4), (lds_t)(&sA[buf][(wid * 2 + h) * 256]), 16, 0, 0);
        aptr += ACH;
        const bool rag = kragged && c == p.nchunks - 1;               // channels beyond ic: the zero row
        if (bload) {
#pragma unroll
            for (int j = 0; j < BP; j++) {
                const float *src = rag && PWG_KC * c + gbk[j] >= p.ic ? pwg_zero_row : gb[j];
                __builtin_amdgcn_global_load_lds((glb_t)src, (lds_t)(&sB[buf][(wid * BP + j) * 256]), 16, 0, 0);
                gb[j] += bstep;
            }
        }
    };

    v16 acc[PXB];
#pragma unroll
    for (int j = 0; j < PXB; j++)
#pragma unroll
        for (int e = 0; e < 16; e++) acc[j][e] = 0.f;

    glds(0, std::integral_constant<int, 0>{});
    __syncthreads();
    const int aoff = (wid * 64 + lane) * 4;                           // + ACH / 2 h2: k-steps 4 h2 .. 4 h2 + 3 of this wave's row block
    const int boff = (lane >> 5) * TN + PXB * (lane & 31);            // + 2 s TN: pixels PXB n .. PXB n + PXB - 1 of channel 2 s + (lane >> 5)
    // one chunk: 8 k-steps from LDS buffer BUF, the next chunk's LDS-DMA in flight, one barrier
    auto chunk = [&](int c, auto BUF) {
        constexpr int buf = decltype(BUF)::value;
        if (c + 1 < p.nchunks && !(p.dbg & 1)) glds(c + 1, std::integral_constant<int, buf ^ 1>{});
        const float *A = sA[buf] + aoff, *B = sB[buf] + boff;
        // the input operands of the next PAIR of k-steps are read from LDS while the MFMAs of this pair run (register double
        // buffer; the scheduling barriers keep hipcc from sinking the reads back to their first use)
        v4 fa[2]; vB fb[2][2];
        auto lread = [&](int q, int s2) {
#pragma unroll
            for (int h = 0; h < 2; h++) fb[q][h] = *reinterpret_cast<const vB *>(B + 2 * (2 * s2 + h) * TN);
        };
        fa[0] = *reinterpret_cast<const v4 *>(A);
        lread(0, 0);
#pragma unroll
        for (int s2 = 0; s2 < PWG_KC / 4; s2++) {
            if (s2 == 0) fa[1] = *reinterpret_cast<const v4 *>(A + ACH / 2);
            if (s2 + 1 < PWG_KC / 4) lread((s2 + 1) & 1, s2 + 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int h = 0; h < 2; h++)
#pragma unroll
                for (int j = 0; j < PXB; j++)
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[s2 >> 1][2 * (s2 & 1) + h], fb[s2 & 1][h][j], acc[j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
    };
    for (int c = 0; c < p.nchunks; c += 2) {
        chunk(c, std::integral_constant<int, 0>{});
        if (c + 1 < p.nchunks) chunk(c + 1, std::integral_constant<int, 1>{});
    }

    if (p.dbg & 8) {                                                  // tuning only: no epilogue (one store keeps the MFMAs alive)
        float t = 0.f;
#pragma unroll
        for (int j = 0; j < PXB; j++)
#pragma unroll
            for (int e = 0; e < 16; e++) t += acc[j][e];
        if (t == 12345.678f) p.out[tid] = t;
        return;
    }
    // epilogue: scale' / bias' / activation (+ residual), PXB consecutive pixels per store.  An output row's address is
    // (uniform row base in SGPRs) + (32-bit lane offset): no per-row vector address arithmetic.
    const float slope = p.act == 2 ? 0.1f : (p.act == 1 ? 0.f : 1.f), rslope = p.res_act == 2 ? 0.1f : (p.res_act == 1 ? 0.f : 1.f);
    const int pxl = PXB * (lane & 31), lh = lane >> 5;
    if (p0 + pxl >= p.P) return;                                      // P % 4 == 0: a lane's pixels are in or out together
    const unsigned voff = ((unsigned)(4 * lh) * (unsigned)p.P + (unsigned)pxl) * 4u;     // bytes; P < 2^26 (launcher)
    const int olu = 32 * wid;                                         // first row of this wave inside the 128-row tile (uniform)
    auto epilogue = [&](auto FULL, auto RES, auto SIG) {
        constexpr bool full = decltype(FULL)::value, res = decltype(RES)::value, sig = decltype(SIG)::value;
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const int ou = olu + (e & 3) + 8 * (e >> 2);              // uniform part of the row; the lane adds 4 lh
            if (!full && PWG_TM * mt + ou + 4 * lh >= p.oc) continue;
            const v2 sb = *reinterpret_cast<const v2 *>(&sSB[2 * (ou + 4 * lh)]);
            vB v;
#pragma unroll
            for (int j = 0; j < PXB; j++) {
                const float t = fmaf(acc[j][e], sb.x, sb.y);
                v[j] = (sig && p.act == 3) ? pwg_sigmoid(t) : act_max(t, slope * t, act_floor(slope));
            }
            const size_t rowoff = ((size_t)(PWG_TM * mt + ou) * (size_t)p.P + (size_t)p0) * 4;      // uniform
            if (res) {
                const vB q = *reinterpret_cast<const vB *>(reinterpret_cast<const char *>(p.residual) + rowoff + voff);
#pragma unroll
                for (int j = 0; j < PXB; j++) {
                    const float t = v[j] + q[j];
                    v[j] = (sig && p.res_act == 3) ? pwg_sigmoid(t) : act_max(t, rslope * t, act_floor(rslope));
                }
            }
            *reinterpret_cast<vB *>(reinterpret_cast<char *>(p.out) + rowoff + voff) = v;
        }
    };
    using T = std::true_type; using F = std::false_type;
    const bool full = PWG_TM * (mt + 1) <= p.oc;
    if (p.act == 3 || p.res_act == 3) { if (p.residual) epilogue(F{}, T{}, T{}); else epilogue(F{}, F{}, T{}); }
    else if (p.residual) { if (full) epilogue(T{}, T{}, F{}); else epilogue(F{}, T{}, F{}); }
    else { if (full) epilogue(T{}, F{}, F{}); else epilogue(F{}, F{}, F{}); }
}

template <int WM>
__global__ void __launch_bounds__(64 * WM) __attribute__((amdgpu_waves_per_eu(4))) k_pw_gemm32(PwG32P p)
{
    // ONE __shared__ object (a second one makes hipcc wait vmcnt(0) before every LDS read while an LDS-DMA is in flight)
    __shared__ __attribute__((aligned(16))) float smem[2 * 512 * WM + 2 * PWG_KC * 128 + 64 * WM];
    // main tiles in an XCD-aware order: workgroup ids go round robin over the 8 XCDs; XCD x walks tiles [x * per_xcd, (x + 1) * per_xcd)
    if (blockIdx.x < (unsigned)(8 * p.per_xcd)) {
        const long total = (long)p.ntm * p.ntn;
        const long tile = (long)(blockIdx.x & 7) * p.per_xcd + (blockIdx.x >> 3);
        if (tile >= total) return;
        pwg_tile<4, WM>(p, smem, (int)(tile % p.ntm), (tile / p.ntm) * 128);
        return;
    }
    // narrow tiles over the pixels behind the main ones
    const long t = (long)blockIdx.x - 8L * p.per_xcd;
    pwg_tile<2, WM>(p, smem, (int)(t % p.ntm), p.ntn * 128 + (t / p.ntm) * 64);
}
