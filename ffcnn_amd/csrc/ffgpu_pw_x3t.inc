// ffgpu_pw_x3t.inc -- pointwise (1x1) convolution, fp32-equivalent results on the BF16 matrix cores, as a TILED, double-buffered GEMM (round 5).
//
// Restates conv-v6.c:46-91: Out[oc][p] = act(scale'[oc] * sum_ci W[oc][ci] * In[ci][p] + bias'[oc]); arithmetic = ffgpu_pw_x3.inc's ("X3": every
// fp32 operand is the exact sum of three bf16 parts, the six partial products with i + j <= 2 on the bf16 matrix cores, fp32 accumulation).
//
// Why a third pointwise kernel: k_pw_x3 / pw_x3s (k_conv_x3<.., 1>) split every input value once per WAVE and channel tile -- eight times for 512 output
// channels -- and sit at 0.38 of what the split form can reach on BASELINE config[2] (matrix cores busy ~40 %, 39 M vector instructions of re-splitting;
// VERDICT r04 item 3).  Here an input value is split ONCE per 256 output channels, by the workgroup, into LDS in operand layout:
//   * workgroup = 4 waves, tile = 256 output channels x 32 PXB pixels (PXB = 4: 128 pixels); wave w owns rows 64 w .. 64 w + 63 and all PXB
//     pixel blocks: 2 x PXB accumulators of v_mfma_f32_32x32x16_bf16 (128 registers at PXB = 4);
//   * K in chunks of 16 (one MFMA k-step), two LDS buffers per operand, ONE barrier per chunk, two workgroups per CU (74 KB of LDS each) that drift
//     out of phase: one's barrier wait is the other's matrix time;
//   * A (weights): plan-time image of the three parts that IS the LDS chunk image ([chunk][part][k-group][row][8 bf16], 24 KB per chunk), brought by
//     LDS-DMA (global_load_lds_dwordx4: no staging registers) one chunk ahead;
//   * B (input): per chunk every lane loads two of the 16 channel rows (16-byte loads; which pair rotates with the lane's pixel slot, see `rot`: 128 contiguous
//     bytes per row and 8 lanes) two chunks ahead, splits its 8 values one chunk ahead (44 vector instructions per wave and chunk, dealt out between that
//     chunk's 48 MFMAs) and writes the bf16 pairs into [part][k-group][pixel slot][8 bf16]; MFMA column n of pixel block j is pixel PXB n + j, so a lane's PXB
//     accumulators of a row are PXB consecutive pixels (16-byte stores, no transpose); both LDS read sides are lane-linear (slot = 32 j + n) and the split
//     stores hit 32 banks with 32 lanes: no bank conflicts on either side (round 6; SQ_LDS_BANK_CONFLICT = 0);
//   * per wave and chunk: 18 ds_read_b128 (2 x 3 A fragments, PXB x 3 B fragments) for 48 MFMAs of 32 cycles -- 1.5 KB of LDS reads per KB a
//     16x16x32 tiling would need twice;
//   * tiles are walked XCD by XCD (the channel tiles of one pixel range share an L2).
#ifndef XT_SPLIT_FIRST
#define XT_SPLIT_FIRST 0
#endif
#ifndef XT_TRACE              // lab builds: 1 = per-tile timeline of wave 0 (FFGPU_PWXT_TRACE=<file>, tools/pw_x3t_trace.py)
#define XT_TRACE 0
#endif
#ifndef XT_NT_LOAD            // lab builds: 1 = non-temporal input loads
#define XT_NT_LOAD 0
#endif
#ifndef XT_STAGGER            // lab builds: 1 = FFGPU_PWXT_DBG >> 8 = units of 8128 cycles the second resident workgroup of every CU (first round) sleeps before its first tile
#define XT_STAGGER 0
#endif
#ifndef XT_PRIO               // lab builds: 1 = the main loop runs at wave priority 2, the epilogue at 0 (the partner workgroup's MFMAs win the issue slot)
#define XT_PRIO 0
#endif
typedef unsigned u4_xt __attribute__((ext_vector_type(4)));
typedef __bf16 v8bf_xt __attribute__((ext_vector_type(8)));
typedef float v16f_xt __attribute__((ext_vector_type(16)));

constexpr int XT_KC = 16;                        // channels per chunk = one k-step of v_mfma_f32_32x32x16_bf16
constexpr int XT_BCH = 3 * 2 * 128 * 4;          // dwords of one input chunk at PXB = 4: [part][k-group][slot][4 dwords]
// RB = 32-row blocks per wave: 2 -> 256 output channels per workgroup tile (128 accumulator registers per wave, two workgroups per CU),
//                              1 -> 128 (64 accumulator registers, three workgroups per CU: more waves in different phases, twice the splits and LDS reads per flop)
constexpr int xt_tm(int rb) { return 128 * rb; }
constexpr int xt_ach(int rb) { return 3 * 2 * xt_tm(rb) * 4; }       // dwords of one weight chunk: [part][k-group][row][4 dwords]

struct PwX3tP {
    const float *in; float *out; const float *residual;
    const unsigned *wpack;       // per channel tile: nchunks x XT_ACH dwords, then [256][2] fp32 scale', bias'
    long P;                      // pixels per channel (P % 4 == 0)
    long ntn;                    // main pixel tiles of 128
    long img;                    // dwords per channel tile
    int  ic, oc, nchunks, ntm;
    int  act, res_act, per_xcd;
    int  nmain, tpw;             // main-tile workgroups and tiles per workgroup (1 unless FFGPU_PWXT_PERSIST): nmain tpw >= ntm ntn
    int  dbg;                    // tuning only (FFGPU_PWXT_DBG): 2 = no epilogue
    unsigned long long *dbg_t;   // XT_TRACE builds: 8 words per tile (start, first barrier, main loop done, epilogue issued, HW_ID, XCC_ID, tile, -)
    int  nt;                     // non-temporal output stores (launcher: outputs of 128 MB and more; FFGPU_PWXT_NT=0 / 1 forces)
};

// dword ((c * 3 + part) * 2 + kg) * 256 + row) * 4 + d of tile mt = parts of W[256 mt + row][16 c + 8 kg + 2 d + (0, 1)] as a bf16 pair
struct PwX3tPackP { const float *filt; unsigned *pk; int ic, oc, k4, nchunks, ntm, rb; };
__global__ void k_pw_x3t_pack(PwX3tPackP p)
{
    const int XT_TM = xt_tm(p.rb), XT_ACH = xt_ach(p.rb);
    const long img = (long)p.nchunks * XT_ACH + 2 * XT_TM, total = img * p.ntm;
    const int rl = p.k4 + 4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int mt = (int)(i / img);
        const long j = i - (long)mt * img;
        unsigned v = 0;
        if (j < (long)p.nchunks * XT_ACH) {
            const int d = (int)(j & 3), row = (int)((j >> 2) % XT_TM), kg = (int)((j >> 2) / XT_TM & 1), t = (int)((j >> 2) / XT_TM >> 1);
            const int part = t % 3, c = t / 3;
            const int o = XT_TM * mt + row, k = XT_KC * c + 8 * kg + 2 * d;
            const float w0 = (o < p.oc && k < p.ic) ? p.filt[(long)o * rl + k] : 0.f, w1 = (o < p.oc && k + 1 < p.ic) ? p.filt[(long)o * rl + k + 1] : 0.f;
            v = irbw_x3_part(w0, part) | (irbw_x3_part(w1, part) << 16);
        } else {
            const int t = (int)(j - (long)p.nchunks * XT_ACH), o = XT_TM * mt + (t >> 1);
            const float f = o < p.oc ? p.filt[(long)o * rl + p.k4 + (t & 1)] : 0.f;
            v = __float_as_uint(f);
        }
        p.pk[i] = v;
    }
}

template <int PXB, int RB>
__device__ __forceinline__ void xt_tile(const PwX3tP &p, unsigned *smem, int mt, long p0, int sbsel = 0)
{
    static_assert(PXB == 4 || PXB == 2, "pixel blocks per wave");
    constexpr int XT_TM = xt_tm(RB), XT_ACH = xt_ach(RB), NPC = XT_ACH / 1024;       // NPC: 4 KB pieces of a weight chunk (6 / 3)
    constexpr int TN = 32 * PXB;
    typedef float vB __attribute__((ext_vector_type(PXB)));
    typedef float v2 __attribute__((ext_vector_type(2)));
    unsigned (*sA)[XT_ACH] = reinterpret_cast<unsigned (*)[XT_ACH]>(smem);
    unsigned (*sB)[XT_BCH] = reinterpret_cast<unsigned (*)[XT_BCH]>(smem + 2 * XT_ACH);
    float *sSB = reinterpret_cast<float *>(smem + 2 * XT_ACH + 2 * XT_BCH) + sbsel * 2 * XT_TM;      // (two tables: a persistent workgroup's next tile fills the other one, no barrier between tiles)

    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 31, kg = lane >> 5;
#if XT_TRACE
    const long trow = ((p0 / 32) * p.ntm + mt) * 8;                   // (unique per tile: main tiles start at multiples of 128, narrow ones of 64)
#define XT_T(k) do { if (p.dbg_t && tid == 0) p.dbg_t[trow + (k)] = __builtin_amdgcn_s_memrealtime(); } while (0)
    if (p.dbg_t && tid == 0) { p.dbg_t[trow + 4] = __builtin_amdgcn_s_getreg(4 | (31 << 11)); p.dbg_t[trow + 5] = __builtin_amdgcn_s_getreg(20 | (31 << 11)); p.dbg_t[trow + 6] = (unsigned long long)blockIdx.x; }
#else
#define XT_T(k) do { } while (0)
#endif
    XT_T(0);
    const unsigned *wimg = p.wpack + (size_t)mt * p.img;
#pragma unroll
    for (int i = 0; i < 2 * XT_TM / 256; i++) sSB[tid + 256 * i] = __uint_as_float(wimg[(size_t)p.nchunks * XT_ACH + 256 * i + tid]);

    // Both operands are fetched through buffer resources (SGPR base + 32-bit lane offset in a VGPR + chunk offset in an SGPR): no per-chunk vector
    // address arithmetic, two address registers in all (flat 64-bit addresses cost ~20 registers and a dozen vector adds per chunk here)
    typedef __attribute__((address_space(3))) void *lds_t;
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned *>(wimg), 0, 0x7fffffff, 0x00020000);
    const unsigned alane = (unsigned)(wid * NPC * 256 + lane * 4) * 4u;    // wave w brings NPC 1 KB pieces of a chunk (bytes [1024 NPC w, ..)), lane-linear
    unsigned aoff = 0;                                                // uniform: byte offset of the next weight chunk
    auto glds = [&](auto BUF) {
        constexpr int buf = decltype(BUF)::value;
#pragma unroll
        for (int h = 0; h < NPC; h++)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_t)(&sA[buf][wid * NPC * 256 + h * 256]), 16, alane, aoff + h * 1024, 0, 0);
        aoff += XT_ACH * 4;
    };
    // this lane's two channel rows of a chunk: k = 16 c + 8 kg + 2 rot + (0, 1) (rot: below), pixels p0 + PXB n .. + PXB - 1 (a ragged last tile re-reads the
    // last PXB pixels; its results are not stored)
    long px = p0 + PXB * n;
    if (px > p.P - PXB) px = p.P - PXB;
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.in + p0), 0, 0x7fffffff, 0x00020000);    // (ic + 32) P < 2^29 floats: launcher
    const unsigned Pu = (unsigned)p.P, pxl = (unsigned)(px - p0);
    // Which two rows of a k-group a lane brings ROTATES with its pixel slot: dword rot = (wid + n / 8) & 3 of the slot's four.  The 32 lanes of a
    // ds_write_b32 group then hit 32 different banks (bank = 4 (n & 7) + rot of 32; with rot = wid for every lane the slots' stride of 4 dwords
    // made every split store 4-way conflicted: 7.4 M of 17.8 M LDS cycles per config[2] launch, VERDICT r05 item 2 (i)).  The image in LDS -- and
    // with it both read sides and the MFMA operand order -- is unchanged; a wave's row loads become eight 128-byte runs instead of two of 512.
    const int rot = (wid + (n >> 3)) & 3;
    const int krow = 8 * kg + 2 * rot;
    const unsigned boff[2] = { ((unsigned)krow * Pu + pxl) * 4u, ((unsigned)(krow + 1) * Pu + pxl) * 4u };      // bytes: rows of chunk 0; + 64 P per chunk (an SGPR)
    auto bld = [&](unsigned voff, unsigned soff) -> vB {
        constexpr int aux = XT_NT_LOAD ? 2 : 0;
        if constexpr (PXB == 4) return __builtin_bit_cast(vB, __builtin_amdgcn_raw_buffer_load_b128(rsB, voff, soff, aux));
        else return __builtin_bit_cast(vB, __builtin_amdgcn_raw_buffer_load_b64(rsB, voff, soff, aux));
    };
    // CLAMP (prologue and the last chunks): rows beyond ic re-read the last row -- bsplit(.., lastc) zeroes them
    auto bload = [&](int c, vB (&raw)[2], auto CLAMP) {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            if (decltype(CLAMP)::value) raw[h] = bld(((unsigned)min(XT_KC * c + krow + h, p.ic - 1) * Pu + pxl) * 4u, 0u);
            else raw[h] = bld(boff[h], (unsigned)(XT_KC * c) * Pu * 4u);
        }
    };
    // split the lane's 2 x PXB values into their three bf16 parts; dword (part, pixel q) = the pair (row k, row k + 1) -> slot 32 q + n, dword rot.
    // `lastc` >= 0 (the chunks around the ragged end): rows beyond ic count as zero (their weights are zero too: no 0 x Inf from a re-read row)
    auto bsplit1 = [&](const vB (&raw)[2], auto BUF, int lastc, int q) {
        constexpr int buf = decltype(BUF)::value;
        unsigned u[3][2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            float x = raw[h][q];
            if (lastc >= 0 && XT_KC * lastc + krow + h >= p.ic) x = 0.f;
            const float r = x3_resid(x);                                                       // exact (0 for +-Inf)
            const float r2 = x3_resid2(r);                                                       // exact, <= 8 significant bits
            u[0][h] = __float_as_uint(x); u[1][h] = __float_as_uint(r); u[2][h] = __float_as_uint(r2);
        }
#pragma unroll
        for (int pt = 0; pt < 3; pt++)
            sB[buf][((pt * 2 + kg) * TN + 32 * q + n) * 4 + rot] = __builtin_amdgcn_perm(u[pt][1], u[pt][0], 0x07060302u);
    };
    auto bsplit = [&](const vB (&raw)[2], auto BUF, int lastc) {
#pragma unroll
        for (int q = 0; q < PXB; q++) bsplit1(raw, BUF, lastc, q);
    };

    v16f_xt acc[RB][PXB];
#pragma unroll
    for (int r = 0; r < RB; r++)
#pragma unroll
        for (int j = 0; j < PXB; j++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[r][j][e] = 0.f;

    // six terms per (row block, pixel block, chunk), the small ones first: (w0 x2) (w1 x1) (w2 x0) | (w0 x1) (w1 x0) | (w0 x0)
    constexpr int WP[6] = { 0, 1, 2, 0, 1, 0 }, XP[6] = { 2, 1, 0, 1, 0, 0 };
    // One chunk of a wave = 12 (PXB = 2: 6) "quads" -- a term for two pixel blocks x RB row blocks -- in a FIXED order, every quad fenced
    // (sched_barrier): the fragment reads run one quad ahead of the MFMAs that use them, in the order of use -- the first MFMA of a chunk waits for 4 reads,
    // not for 12 (round 5's listing: all reads of a half in front of its first MFMA, `s_waitcnt lgkmcnt(3)`; the timeline's lone workgroup at 58 % of
    // the pipe) -- the second half's input fragments arrive under the first half's last three quads, in the registers of parts that are dead by then,
    // and the split of the next chunk's rows (`slice(q)`: 10 vector instructions + 3 LDS stores per pixel) is dealt out between later quads instead
    // of standing as one block of 44 + 12 behind the last MFMA.
    auto compute = [&](auto BUF, auto slice) {
        constexpr int buf = decltype(BUF)::value;
        auto ldA = [&](int r, int pt) { return *reinterpret_cast<const u4_xt *>(&sA[buf][((pt * 2 + kg) * XT_TM + 32 * RB * wid + 32 * r + n) * 4]); };
        auto ldB = [&](int j, int pt) { return *reinterpret_cast<const u4_xt *>(&sB[buf][((pt * 2 + kg) * TN + 32 * j + n) * 4]); };
        u4_xt fa[RB][3], fb[2][3], fc[2][3];                          // fc: the second pair of pixel blocks (PXB = 4)
#ifndef XT_QORDER             // lab builds: 1 = the MFMAs of a quad row block by row block (consecutive MFMAs share the WEIGHT fragment instead of the input fragment)
#define XT_QORDER 0
#endif
        auto quad = [&](int m, int jp, u4_xt (&f)[2][3]) {
#pragma unroll
            for (int i = 0; i < 2 * RB; i++) {
                const int jj = XT_QORDER ? i % 2 : i / RB, r = XT_QORDER ? i / 2 : i % RB;
                acc[r][jp + jj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8bf_xt, fa[r][WP[m]]), __builtin_bit_cast(v8bf_xt, f[jj][XP[m]]),
                                                                         acc[r][jp + jj], 0, 0, 0);
            }
        };
        auto rdq = [&](int m) {                                       // what quad m of the first half reads: weight part WP[m], input part XP[m] of blocks 0 / 1
#pragma unroll
            for (int r = 0; r < RB; r++) fa[r][WP[m]] = ldA(r, WP[m]);
#pragma unroll
            for (int jj = 0; jj < 2; jj++) fb[jj][XP[m]] = ldB(jj, XP[m]);
        };
        auto rdc = [&](int pt) {
#pragma unroll
            for (int jj = 0; jj < 2; jj++) fc[jj][pt] = ldB(2 + jj, pt);
        };
#define XT_FENCE() __builtin_amdgcn_sched_barrier(0)
        rdq(0); XT_FENCE();
        rdq(1); quad(0, 0, fb); XT_FENCE();
        rdq(2); quad(1, 0, fb); XT_FENCE();
        quad(2, 0, fb); XT_FENCE();
        if constexpr (PXB == 4) {
            quad(3, 0, fb); rdc(2); XT_FENCE();                       // (x2 of blocks 0 / 1 is dead since quad 0)
            quad(4, 0, fb); rdc(1); XT_FENCE();                       // (x1: since quad 3)
            quad(5, 0, fb); slice(0); XT_FENCE();
            quad(0, 2, fc); rdc(0); XT_FENCE();                       // (x0: since quad 5)
            quad(1, 2, fc); slice(1); XT_FENCE();
            quad(2, 2, fc); slice(2); XT_FENCE();
            quad(3, 2, fc); slice(3); XT_FENCE();
            quad(4, 2, fc); XT_FENCE();
            quad(5, 2, fc);
        } else {
            quad(3, 0, fb); slice(0); XT_FENCE();
            quad(4, 0, fb); slice(1); XT_FENCE();
            quad(5, 0, fb);
        }
#undef XT_FENCE
    };
    auto noslice = [](int) { };

    // pipeline: chunk c computes from buffers c & 1 while the weights of chunk c + 1 arrive by LDS-DMA, the input rows of chunk c + 1 (loaded
    // during chunk c - 1) are split into the other buffer and the rows of chunk c + 2 are in flight.  Chunks go in PAIRS (the image is padded with
    // zero weights to an even count): buffer index and the roles of the two raw-register sets are compile-time, the accumulators never meet a
    // parity branch.  Three copies of the pair: whole chunks (no clamp, no mask), the chunks around the ragged end, the last pair.
    using B0 = std::integral_constant<int, 0>; using B1 = std::integral_constant<int, 1>;
    using T = std::true_type; using F = std::false_type;
    const int npad = p.nchunks, nfull = p.ic / XT_KC;                 // uniform; npad is even (launcher)
    vB rawa[2], rawb[2];
    glds(B0{});
    __builtin_amdgcn_sched_barrier(0);                                // (the pieces first: see step())
    bload(0, rawa, T{});
    bload(1, rawb, T{});
    __builtin_amdgcn_sched_barrier(0);
    bsplit(rawa, B0{}, 0);
    // hipcc does not know that an LDS-DMA load writes LDS: the wait in front of every barrier is spelled out (ADVICE r05; ffgpu_conv_x3.inc had exactly this
    // slip).  vmcnt(2): everything but the two youngest loads -- rawb's plain rows, issued BEHIND the DMA pieces -- has landed; tools/isa_lint.py rule 3
    // checks in the listing that the two youngest vector-memory instructions in front of the barrier are indeed plain loads.
    __builtin_amdgcn_s_waitcnt(0x0f72);                               // vmcnt(2)
    __syncthreads();
    XT_T(1);
    // rcur: the rows of chunk c + 1 (split now); rnxt: receives the rows of chunk c + 2 (LOAD)
    auto step = [&](int c, auto BUF, vB (&rcur)[2], vB (&rnxt)[2], auto TAIL, auto LOAD) {
        constexpr int buf = decltype(BUF)::value;
        constexpr bool tail = decltype(TAIL)::value;
        glds(std::integral_constant<int, buf ^ 1>{});
        // the DMA pieces FIRST, the two plain row loads behind them, pinned: only then does vmcnt(2) in front of the barrier cover the pieces.  (Round 5's
        // listing had the row loads hoisted in front of five of the six pieces in the first step of every pair: hipcc -- which does know that an LDS-DMA
        // load writes LDS -- answered with vmcnt(0) there, i.e. every other chunk waited for the rows it had just asked for: a full memory latency.)
        __builtin_amdgcn_sched_barrier(0);
        if (decltype(LOAD)::value) bload(c + 2, rnxt, TAIL);
        __builtin_amdgcn_sched_barrier(0);                            // the loads stay in front of the chunk's MFMAs (the scheduler sinks them to the barrier otherwise)
#if XT_SPLIT_FIRST                                                 // lab builds only (tools/build_lab_lib.sh): split and LDS writes in front of the chunk's MFMAs
        bsplit(rcur, std::integral_constant<int, buf ^ 1>{}, tail ? c + 1 : -1);
        compute(BUF, noslice);
#else
        compute(BUF, [&](int q) { bsplit1(rcur, std::integral_constant<int, buf ^ 1>{}, tail ? c + 1 : -1, q); });
#endif
        if (decltype(LOAD)::value) __builtin_amdgcn_s_waitcnt(0x0f72);   // vmcnt(2): this step's DMA pieces are in LDS, the two row loads behind them stay in flight
        else __builtin_amdgcn_s_waitcnt(0x0f70);                         // vmcnt(0)
        __syncthreads();
    };
#if XT_PRIO
    __builtin_amdgcn_s_setprio(2);
#endif
    int c = 0;
    for (; c + 3 < nfull && c + 2 < npad; c += 2) { step(c, B0{}, rawb, rawa, F{}, T{}); step(c + 1, B1{}, rawa, rawb, F{}, T{}); }
    for (; c + 2 < npad; c += 2) { step(c, B0{}, rawb, rawa, T{}, T{}); step(c + 1, B1{}, rawa, rawb, T{}, T{}); }
    step(c, B0{}, rawb, rawa, T{}, F{});
    compute(B1{}, noslice);
    XT_T(2);
#if XT_PRIO
    __builtin_amdgcn_s_setprio(0);
#endif

    if (p.dbg & 2) {                                                  // tuning only: no epilogue (one store keeps the MFMAs alive)
        float t = 0.f;
#pragma unroll
        for (int r = 0; r < RB; r++)
#pragma unroll
            for (int j = 0; j < PXB; j++)
#pragma unroll
                for (int e = 0; e < 16; e++) t += acc[r][j][e];
        if (t == 12345.678f) p.out[tid] = t;
        return;
    }
    // epilogue: scale' / bias' / activation (+ residual); row = 64 wid + 32 r + (e & 3) + 8 (e >> 2) + 4 kg, pixels p0 + PXB n .. : PXB consecutive pixels per store
    const float slope = p.act == 2 ? 0.1f : (p.act == 1 ? 0.f : 1.f), rslope = p.res_act == 2 ? 0.1f : (p.res_act == 1 ? 0.f : 1.f);
    if (p0 + PXB * n >= p.P) return;                                  // P % 4 == 0: a lane's pixels are in or out together
    const unsigned voff = ((unsigned)(4 * kg) * Pu + (unsigned)(PXB * n)) * 4u;          // bytes; (ic + 32) P < 2^30 and oc P < 2^30 (launcher)
    // Round 6: the epilogue is ~5 us of every tile in which no MFMA runs (both workgroups of a CU are in phase), so its issue time counts.  (i) scale' / bias' of a
    // row block come with 8 ds_read_b128 up front (rows 8 g + 4 kg + 0 .. 3 are 32 consecutive bytes) -- round 5's listing had one ds_read_b64 per store with
    // `s_waitcnt lgkmcnt(0)` right behind it: 32 exposed LDS latencies per wave; (ii) max(t, slope t) as a bare v_max_f32: behind the opaque fma hipcc put a
    // canonicalising v_max_f32 v, v, v in front of every fmaxf (both operands come out of arithmetic: nothing to quiet).  18 -> 13 vector instructions per store.
    // (with the floor of act_floor as third operand: relu(NaN) = relu(-Inf) = 0 as in the reference; the floor is wave-uniform, one scalar operand)
    auto max_raw = [](float a, float b, float floor) { float d; asm("v_max3_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "s"(floor)); return d; };
    auto epilogue = [&](auto FULL, auto RES, auto SIG, auto NT) {
        constexpr bool full = decltype(FULL)::value, res = decltype(RES)::value, sig = decltype(SIG)::value, nt = decltype(NT)::value;
        auto act1 = [&](float t, int a, float sl) { return (sig && a == 3) ? pwg_sigmoid(t) : max_raw(t, sl * t, act_floor(sl)); };
#pragma unroll
        for (int r = 0; r < RB; r++) {
            typedef float v4 __attribute__((ext_vector_type(4)));
            v4 sbq[4][2];                                             // [g][half]: (scale', bias') of rows 8 g + 4 kg + (0, 1 | 2, 3) of this row block
#pragma unroll
            for (int g = 0; g < 4; g++)
#pragma unroll
                for (int hh = 0; hh < 2; hh++) sbq[g][hh] = *reinterpret_cast<const v4 *>(&sSB[2 * (32 * RB * wid + 32 * r + 8 * g + 4 * kg + 2 * hh)]);
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const int ou = 32 * RB * wid + 32 * r + (e & 3) + 8 * (e >> 2);               // uniform part of the row; the lane adds 4 kg
                if (!full && XT_TM * mt + ou + 4 * kg >= p.oc) continue;
                const v4 q4 = sbq[e >> 2][(e & 3) >> 1];
                const float sbx = (e & 1) ? q4[2] : q4[0], sby = (e & 1) ? q4[3] : q4[1];
                vB v;
                if constexpr (PXB == 4) {
                    const v4f_pw f = pw_fma4_apart(acc[r][0][e], acc[r][1][e], acc[r][2][e], acc[r][3][e], sbx, sby);    // (plain v_fma_f32: DESIGN 5.10)
#pragma unroll
                    for (int j = 0; j < PXB; j++) v[j] = act1(f[j], p.act, slope);
                } else {
#pragma unroll
                    for (int j = 0; j < PXB; j++) { float t = fmaf(acc[r][j][e], sbx, sby); asm volatile("" : "+v"(t)); v[j] = act1(t, p.act, slope); }
                }
                const size_t rowoff = ((size_t)(XT_TM * mt + ou) * (size_t)p.P + (size_t)p0) * 4;  // uniform
                if (res) {
                    const vB q = *reinterpret_cast<const vB *>(reinterpret_cast<const char *>(p.residual) + rowoff + voff);
#pragma unroll
                    for (int j = 0; j < PXB; j++) v[j] = act1(v[j] + q[j], p.res_act, rslope);
                }
                // nt = p.nt: an output far larger than the caches is streamed past them (config[2]'s 210 MB: 140 -> 131 us; the lines the partner workgroup's
                // loads need stay where they are; sc0 / sc1 on top change nothing, non-temporal INPUT loads cost the gain again).  A compile-time copy: under a
                // run-time test the two stores are merged and the hint is lost.
                // NOT buffer_store_dwordx4 with the row offset in an SGPR (2 us faster, measured): on gfx950 a vector instruction that overwrites one of the
                // store's data registers right behind it corrupts that dword on some lanes -- the "store of more than 8 bytes" wait state, which hipcc only
                // inserts for an IMMEDIATE soffset (profiles/r05_e_buffer_store_hazard.txt; tools/isa_lint.py rejects the pattern).
                if constexpr (nt) __builtin_nontemporal_store(v, reinterpret_cast<vB *>(reinterpret_cast<char *>(p.out) + rowoff + voff));
                else *reinterpret_cast<vB *>(reinterpret_cast<char *>(p.out) + rowoff + voff) = v;
            }
        }
    };
    const bool full = XT_TM * (mt + 1) <= p.oc;
    if (p.act == 3 || p.res_act == 3) { if (p.residual) epilogue(F{}, T{}, T{}, F{}); else epilogue(F{}, F{}, T{}, F{}); }
    else if (p.residual) { if (full) epilogue(T{}, T{}, F{}, F{}); else epilogue(F{}, T{}, F{}, F{}); }
    else if (p.nt) { if (full) epilogue(T{}, F{}, F{}, T{}); else epilogue(F{}, F{}, F{}, T{}); }          // (streamed stores: the plain form only)
    else { if (full) epilogue(T{}, F{}, F{}, F{}); else epilogue(F{}, F{}, F{}, F{}); }
    XT_T(3);
#undef XT_T
}

template <int RB>
__global__ void __launch_bounds__(256, RB == 2 ? 2 : 3) k_pw_x3t(PwX3tP p)
{
    // ONE __shared__ object (see ffgpu_pw_gemm32.inc): 2 weight chunks (24 / 12 KB each), 2 x 12 KB input chunks, scale' / bias'
    __shared__ __attribute__((aligned(16))) unsigned smem[2 * xt_ach(RB) + 2 * XT_BCH + 4 * xt_tm(RB)];
    // main tiles in an XCD-aware order: workgroup ids go round robin over the 8 XCDs; XCD x walks tiles [x per_xcd, (x + 1) per_xcd): the channel
    // tiles of one pixel range share an L2
    // (tpw > 1, FFGPU_PWXT_PERSIST: a workgroup walks tiles b, b + nmain, ... -- the next tile's first loads go out right behind this tile's stores instead
    //  of behind their acknowledgement and a workgroup launch; nmain % 8 == 0 keeps a workgroup's tiles on its XCD)
#if XT_STAGGER
    if ((p.dbg >> 8) && blockIdx.x < 512u && (((blockIdx.x >> 3) >> 5) & 1))
        for (int i = 0; i < (p.dbg >> 8); i++) __builtin_amdgcn_s_sleep(127);
#endif
    if (blockIdx.x < (unsigned)p.nmain) {
        const long total = (long)p.ntm * p.ntn;
        for (int i = 0; i < p.tpw; i++) {
            const unsigned m = blockIdx.x + (unsigned)i * (unsigned)p.nmain;
            const long tile = (long)(m & 7) * p.per_xcd + (m >> 3);
            if ((int)(m >> 3) >= p.per_xcd || tile >= total) return;
            xt_tile<4, RB>(p, smem, (int)(tile % p.ntm), (tile / p.ntm) * 128, i & 1);
        }
        return;
    }
    // narrow tiles (64 pixels) over the pixels behind the main ones: the partial last round of workgroups
    const long t = (long)blockIdx.x - (long)p.nmain;
    xt_tile<2, RB>(p, smem, (int)(t % p.ntm), p.ntn * 128 + (t / p.ntm) * 64);
}
