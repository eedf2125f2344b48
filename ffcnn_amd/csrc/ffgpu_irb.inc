// ffgpu_irb.inc -- fused "inverted residual block" of yolo-fastest on gfx950:
//
//     1x1 expand (ic -> ec, act1)  ->  depthwise 3x3 (stride 1|2, pad 1, actd)
//     -> 1x1 project (ec -> oc, act2)  [-> + residual, res_act]
//
// i.e. three consecutive groupconv calls of the reference (conv-v6.c:46-91, 96-287, 46-91)
// and the shortcut that follows (ffcnn.c:418-423), with the two expanded tensors (the
// largest activations of the net) kept in LDS instead of making four trips through HBM.
//
// Persistent workgroups (4 waves) walk output tiles of TH x TW pixels of NF frames:
//   phase 1  input tile + 1-px halo (ic channels)              global -> LDS  In[k4][NPin]
//   per chunk of ECH expanded channels:
//   phase 2  E = act1(s1 * W1c . In + b1), zero outside the image  MFMA -> LDS  E[ECH][NPin]
//   phase 3  B = actd(sd * dw3x3(E) + bd) built per lane straight in the MFMA B-operand
//            layout (16-byte + 8-byte LDS reads per tap row), acc += W2c . B   (MFMA)
//   epilogue out = act2(s2 * acc + b2) [+ residual]             16-byte stores, CNHW
// All matrix products run on v_mfma_f32_16x16x4_f32 (exact fp32).  The pixel <-> MFMA column
// mapping is the one of ffgpu_pw_mfma.inc: a lane owns 4 consecutive pixels of a row.
// Every per-layer constant (A fragments of both GEMMs, depthwise taps, scale'/bias') is packed
// once at plan time into the exact LDS image (k_irb_pack), so staging is one coalesced copy;
// single-chunk blocks stage it once per workgroup, multi-chunk blocks prefetch chunk c+1 into
// registers while chunk c computes.  When a tile has fewer than 4 pixel strips the channel
// loop of phase 3 is split across the idle waves (KS) and reduced through LDS.
#ifndef IRB_TRACE
#define IRB_TRACE 0      // make TRACE=1: in-kernel timeline (tools/irb_trace.py); costs registers, never in the product build
#endif
typedef float v4f_irb __attribute__((ext_vector_type(4)));
typedef float v2f_irb __attribute__((ext_vector_type(2)));

#define IRB_TAPP 12      // depthwise row in the packed image: 9 taps, scale', bias', pad

struct IrbP {
    const float *in; float *out; const float *residual;
    const float *pk;                 // packed constants (see irb_pack_layout)
    int N, H, W, OH, OW;             // input / output plane geometry
    int ic, ec, oc, stride;
    float act1, actd, act2, res_act; // activation slopes (see irb_act)
    int TH, TW, TWq;                 // output tile; TWq = ceil(TW / 4) quads per tile row
    int NF;                          // frames per workgroup
    int EH, EW;                      // input tile rows / padded row length (EW % 4 == 0)
    int NPin;                        // NF*EH*EW rounded up to 64
    int NPout;                       // NF*TH*TWq*4
    int tiles_x, tiles_y, ntiles;
    int k4, nchunks, ECH;            // ALIGN(ic,4); ceil(ec/ECH); 16 or 32
    int CH;                          // floats per chunk in the packed image (multiple of 4)
    int KS;                          // waves sharing one pixel strip in phase 3 (1, 2 or 4)
    int red_off;                     // float offset of the split-K scratch in LDS (0 = aliases In..E)
    int vec_store;                   // OW % 4 == 0 and tile origins 4-aligned -> 16-byte stores
    int resident;                    // every chunk's constants live in LDS for the whole kernel (no per-chunk streaming)
    int inv_nsi;                     // ceil(65536 / (NPin/64)): wave item -> (channel, strip) without a division
    unsigned long long *dbg_t;       // tuning only (FFGPU_IRB_TRACE): 8 timestamps per workgroup (100 MHz REFCLK)
    int dbg_skip;                    // tuning only (FFGPU_IRB_SKIP): 1 no input loads, 2 no expand, 4 no dw/project, 8 no stores
};

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains the vector-memory queue
// (s_waitcnt vmcnt(0)), which would stall every barrier on the prefetches this kernel keeps in flight
// (next chunk's constants, residual tile) and on the previous tile's stores.
__device__ __forceinline__ void irb_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// global access as (wave-uniform base, 32-bit BYTE offset per lane): lets the compiler use the scalar-base addressing
// form (one VGPR per address, no 64-bit lane arithmetic).  Offsets must stay below 2^32 bytes (checked at launch).
template <class T> __device__ __forceinline__ T irb_ld(const void *base, unsigned byte_off)
{ return *reinterpret_cast<const T *>(reinterpret_cast<const char *>(base) + byte_off); }
template <class T> __device__ __forceinline__ void irb_st(void *base, unsigned byte_off, T v)
{ *reinterpret_cast<T *>(reinterpret_cast<char *>(base) + byte_off) = v; }

// linear / relu / leaky(0.1) (utils.h:15-23) as ONE branch-free form: act(x) = max(x, slope * x) with
// slope 1, 0 or 0.1 -- two VALU ops and no wave-uniform branches in the inner loops
__device__ __forceinline__ float irb_act(float x, float slope) { return act_max(x, slope * x, act_floor(slope)); }

// ---- packed constants ------------------------------------------------------------------
// chunk c at pk + c*CH:  [W1 frags ks1*MT*64][W2 frags (ECH/4)*OT*64][Wd ECH*12][Sb1 ECH*2]
// after the chunks:      [Sb2 OT*16*2]
struct IrbPackP {
    const float *w1, *wd, *w2; float *pk;
    int ic, ec, oc, k4, ECH, MT, OT, nchunks, CH;
};

__global__ void k_irb_pack(IrbPackP p)
{
    const int total = p.nchunks * p.CH + p.OT * 32;
    const int rl1 = p.k4 + 4, rl2 = ((p.ec + 3) & ~3) + 4;
    const int ks1 = p.k4 >> 2;
    const int n1 = ks1 * p.MT * 64, n2 = (p.ECH / 4) * p.OT * 64, n3 = p.ECH * IRB_TAPP, n4 = p.ECH * 2;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        float v = 0.f;
        if (i >= p.nchunks * p.CH) {
            const int j = i - p.nchunks * p.CH, o = j >> 1;
            if (o < p.oc) v = p.w2[(long)o * rl2 + (rl2 - 4) + (j & 1)];
        } else {
            const int c = i / p.CH, ec0 = c * p.ECH;
            int j = i - c * p.CH;
            if (j < n1) {
                const int l = j & 63, t = (j >> 6) % p.MT, ks = (j >> 6) / p.MT;
                const int e = ec0 + 16 * t + (l & 15), ci = 4 * ks + (l >> 4);
                if (e < p.ec) v = p.w1[(long)e * rl1 + ci];                 // rows are zero padded up to k4
            } else if ((j -= n1) < n2) {
                const int l = j & 63, t = (j >> 6) % p.OT, ks = (j >> 6) / p.OT;
                const int o = 16 * t + (l & 15), e = ec0 + 4 * ks + (l >> 4);
                if (o < p.oc && e < p.ec) v = p.w2[(long)o * rl2 + e];
            } else if ((j -= n2) < n3) {
                const int e = ec0 + j / IRB_TAPP, k = j % IRB_TAPP;
                if (e < p.ec) v = k < 9 ? p.wd[(long)e * 16 + k] : (k < 11 ? p.wd[(long)e * 16 + 12 + (k - 9)] : 0.f);
            } else if ((j -= n3) < n4) {
                const int e = ec0 + (j >> 1);
                if (e < p.ec) v = p.w1[(long)e * rl1 + p.k4 + (j & 1)];
            }
        }
        p.pk[i] = v;
    }
}

// MT = ECH/16 expand tiles per chunk, OT = ceil(oc/16) output tiles, SPW = output strips per wave, S = stride,
// NW = waves per workgroup (8: two waves per SIMD hide each other's LDS / MFMA latencies)
template <int MT, int OT, int SPW, int S, int NW>
__global__ void __launch_bounds__(NW * 64, (NW == 8 && OT <= 2) ? 4 : 2) k_irb(IrbP p)   // <= 128 VGPRs: two 8-wave workgroups per CU
{
    constexpr int NT = NW * 64;
#if IRB_TRACE
#define IRB_T(k) do { if (p.dbg_t && threadIdx.x == 0) p.dbg_t[blockIdx.x * 16 + (k)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define IRB_T(k) do { } while (0)
#endif
    IRB_T(0);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave id in an SGPR
    const int kq = lane >> 4, jq = lane & 15;
    constexpr int ECH = MT * 16;
    const int ks1 = p.k4 >> 2;                        // k-steps of the expand GEMM
    const bool multi = p.nchunks > 1;
    // ---- LDS carve (all offsets multiples of 4 floats)
    float *In  = smem;                                // [k4][NPin]
    float *E   = In + p.k4 * p.NPin;                  // [ECH][NPin]
    float *Msk = E + ECH * p.NPin;            // [NPin] 1 inside the image, 0 outside
    float *Wc  = Msk + p.NPin;                        // resident: [nchunks][CH]; streamed: [2][CH] packed chunk constants
    const bool stream = multi && !p.resident;         // chunk constants double-buffered through registers
    float *Sb2 = Wc + (stream ? 2 : p.nchunks) * p.CH; // [OT*16][2]
    int2 *Geo = reinterpret_cast<int2 *>(Sb2 + OT * 32);   // [NPin] (BYTE offset inside the image relative to the tile origin, f<<24 | iy<<12 | ix or -1)
    const int o_w2 = ks1 * MT * 64, o_wd = o_w2 + (ECH / 4) * OT * 64, o_sb1 = o_wd + ECH * IRB_TAPP;

    const int epl = p.EH * p.EW;                      // input-tile elements per frame
    const long HW = (long)p.H * p.W, ics = (long)p.N * HW;
    const long OHW = (long)p.OH * p.OW, ocs = (long)p.N * OHW;
    const int nso = (p.NPout + 63) >> 6, nsi = p.NPin >> 6;

    // ---- constants that never change: Sb2 here; every chunk (resident) or chunk 0 (streamed) rides along with the
    // first tile's input loads (see phase 1)
    for (int i = tid; i < OT * 32; i += NT) Sb2[i] = p.pk[(long)p.nchunks * p.CH + i];
    const int ch4 = p.CH >> 2;
    const int n4 = (stream ? 1 : p.nchunks) * ch4;
    // ---- geometry of the input-tile elements (same for every tile)
    for (int e = tid; e < p.NPin; e += NT) {
        const int f = e / epl, rem = e - f * epl;
        const int iy = rem / p.EW, ix = rem - iy * p.EW;
        Geo[e] = make_int2((f * (int)HW + iy * p.W + ix) * 4, f < p.NF ? ((f << 24) | (iy << 12) | ix) : -1);
    }
    // ---- per-lane geometry of the output strips this wave works on
    // KS waves share a strip: wave -> (strip slot = wid / KS ... ), k-slice = wid % KS
    const int kslice = p.KS > 1 ? wid % p.KS : 0;
    const int sbase = p.KS > 1 ? wid / p.KS : wid;    // first strip of this wave
    const int sstep = p.KS > 1 ? NW / p.KS : NW;
    int ebase[SPW], o_ty[SPW], o_tq[SPW], o_f[SPW];
    bool qok[SPW];
#pragma unroll
    for (int s = 0; s < SPW; s++) {
        const int strip = sbase + sstep * s;
        const int quad = strip * 16 + jq;             // quad index inside the tile
        const int qpf = p.TH * p.TWq;
        const int f = quad / qpf, rem = quad - f * qpf;
        const int ty = rem / p.TWq, tq = rem - ty * p.TWq;
        qok[s] = strip < nso && quad * 4 < p.NPout;
        ebase[s] = qok[s] ? f * epl + ty * S * p.EW + tq * 4 * S : 0;
        o_ty[s] = ty; o_tq[s] = tq; o_f[s] = f;
    }
    const v4f_irb z = { 0.f, 0.f, 0.f, 0.f };
    IRB_T(1);
    int gc = 0;                                       // chunks processed so far: selects the constants buffer

    for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
        int b = tile;
        const int tx_i = b % p.tiles_x; b /= p.tiles_x;
        const int ty_i = b % p.tiles_y; b /= p.tiles_y;
        const int n0 = b * p.NF;
        const int oy0 = ty_i * p.TH, ox0 = tx_i * p.TW;
        const int gy0 = oy0 * S - 1, gx0 = ox0 * S - 1;   // image coordinates of input-tile element (0,0)

        // tile whose input window lies wholly inside the image and whose frames all exist: no masking needed
        // (the padded columns beyond the real window only feed outputs that are never stored)
        const bool interior = gy0 >= 0 && gx0 >= 0 && gy0 + p.EH <= p.H && gx0 + p.EW <= p.W && n0 + p.NF <= p.N;
        irb_barrier();                                  // previous tile done with In / Msk / E
        if (tile == (int)blockIdx.x) IRB_T(2);
        // ---- phase 1: input tile -> LDS (zero outside the image), validity mask.  A wave item is one channel of one
        // 64-element strip; every wave keeps 8 independent loads in flight.  Loads are unconditional (clamped to a valid
        // element, zeroed afterwards): hipcc waits for a load under a lane predicate on the spot, which would serialise
        // the whole staging loop.
        {
            const bool first = tile == (int)blockIdx.x;
            v4f_irb cr[8];
            if (first) {                                // constants: in flight underneath the input loads
#pragma unroll
                for (int u = 0; u < 8; u++) cr[u] = irb_ld<v4f_irb>(p.pk, (unsigned)min(tid + u * NT, n4 - 1) * 16u);
            }
            // (gy0 + 1, gx0 + 1) of frame n0 is always inside the image: the element rejected lanes read instead
            const float *src0 = p.in + (long)n0 * HW + (long)gy0 * p.W + gx0;
            const unsigned safe = (unsigned)(p.W + 1) * 4u;
            const int nitems = p.k4 * nsi;
            constexpr int U = 8;
            for (int base = wid; base < nitems; base += NW * U) {
                float v[U];
                bool okk[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const int wi = min(base + NW * u, nitems - 1);          // wave-uniform
                    const int c = (wi * p.inv_nsi) >> 16, e = (wi - c * nsi) * 64 + lane;
                    const int2 g = Geo[e];
                    const int f = g.y >> 24, iy = (g.y >> 12) & 0xfff, ix = g.y & 0xfff;
                    const bool ok = (g.y >= 0) & (n0 + f < p.N) & ((unsigned)(gy0 + iy) < (unsigned)p.H) &
                                    ((unsigned)(gx0 + ix) < (unsigned)p.W) & !(p.dbg_skip & 1);      // no short-circuit branches
                    const float *cb = src0 + (long)min(c, p.ic - 1) * ics;  // scalar base + 32-bit lane offset
                    v[u] = irb_ld<float>(cb, ok ? (unsigned)g.x : safe);
                    okk[u] = ok && c < p.ic;
                    if (c == 0) Msk[e] = ok ? 1.f : 0.f;
                }
#pragma unroll
                for (int u = 0; u < U; u++) if (base + NW * u < nitems) In[(base + NW * u) * 64 + lane] = okk[u] ? v[u] : 0.f;
            }
            if (first) {
#pragma unroll
                for (int u = 0; u < 8; u++) if (tid + u * NT < n4) reinterpret_cast<v4f_irb *>(Wc)[tid + u * NT] = cr[u];
                for (int i0 = tid + 8 * NT; i0 < n4; i0 += 8 * NT) {        // (only the largest blocks get here)
#pragma unroll
                    for (int u = 0; u < 8; u++) cr[u] = irb_ld<v4f_irb>(p.pk, (unsigned)min(i0 + u * NT, n4 - 1) * 16u);
#pragma unroll
                    for (int u = 0; u < 8; u++) if (i0 + u * NT < n4) reinterpret_cast<v4f_irb *>(Wc)[i0 + u * NT] = cr[u];
                }
            }
        }
        if (tile == (int)blockIdx.x) IRB_T(3);
        v4f_irb acc[SPW][OT][4];
#pragma unroll
        for (int s = 0; s < SPW; s++)
#pragma unroll
            for (int t = 0; t < OT; t++)
#pragma unroll
                for (int q = 0; q < 4; q++) acc[s][t][q] = z;

#if IRB_TRACE
        unsigned long long tacc[4] = { 0, 0, 0, 0 }, tprev = p.dbg_t ? __builtin_amdgcn_s_memrealtime() : 0;
#define IRB_TA(k) do { if (p.dbg_t) { const unsigned long long tn = __builtin_amdgcn_s_memrealtime(); tacc[k] += tn - tprev; tprev = tn; } } while (0)
#else
#define IRB_TA(k) do { } while (0)
#endif
        for (int c = 0; c < p.nchunks; c++, gc++) {
            const int ec0 = c * ECH;
            const float *W = Wc + (stream ? (gc & 1) : c) * p.CH;
            // prefetch the next chunk's constants (chunk 0 of the next tile after the last one)
            constexpr int WPT = 1024 / NT;                 // CH <= 4096 floats
            v4f_irb wreg[WPT];
            if (stream) {
                const int cn = c + 1 == p.nchunks ? 0 : c + 1;
                const v4f_irb *srcw = reinterpret_cast<const v4f_irb *>(p.pk + (long)cn * p.CH);
#pragma unroll
                for (int k = 0; k < WPT; k++) wreg[k] = (tid + NT * k < ch4) ? srcw[tid + NT * k] : z;
            }
            irb_barrier();                              // In + W visible, E free
            IRB_TA(0);
            const float *W1l = W, *W2l = W + o_w2, *Wdl = W + o_wd, *Sb1 = W + o_sb1;

            // ---- phase 2: E[chunk] = mask * act1(s1 * (W1c . In) + b1)
            for (int item = wid; item < ((p.dbg_skip & 2) ? 0 : MT * nsi); item += NW) {
                const int t = item % MT, si = item / MT;
                const int px = si * 64 + jq * 4;
                v4f_irb a4[4] = { z, z, z, z };
                for (int ks = 0; ks < ks1; ks++) {
                    const float a = W1l[(ks * MT + t) * 64 + lane];
                    const v4f_irb bv = *reinterpret_cast<const v4f_irb *>(In + (4 * ks + kq) * p.NPin + px);
                    a4[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv.x, a4[0], 0, 0, 0);
                    a4[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv.y, a4[1], 0, 0, 0);
                    a4[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv.z, a4[2], 0, 0, 0);
                    a4[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv.w, a4[3], 0, 0, 0);
                }
                v4f_irb m = { 1.f, 1.f, 1.f, 1.f };
                if (!interior) m = *reinterpret_cast<const v4f_irb *>(Msk + px);
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int ch = 16 * t + 4 * kq + r;
                    const v2f_irb sb = *reinterpret_cast<const v2f_irb *>(Sb1 + 2 * ch);
                    v4f_irb v;
                    v.x = irb_act(fmaf(a4[0][r], sb.x, sb.y), p.act1); v.y = irb_act(fmaf(a4[1][r], sb.x, sb.y), p.act1);
                    v.z = irb_act(fmaf(a4[2][r], sb.x, sb.y), p.act1); v.w = irb_act(fmaf(a4[3][r], sb.x, sb.y), p.act1);
                    if (!interior) v *= m;
                    *reinterpret_cast<v4f_irb *>(E + ch * p.NPin + px) = v;
                }
            }
            IRB_TA(1);
            irb_barrier();
            IRB_TA(2);

            // ---- phase 3: depthwise 3x3 from LDS straight into the B operand, project with W2c
            const int kmax = (min(ECH, p.ec - ec0) + 3) >> 2;     // channels really present in this chunk
#pragma unroll
            for (int s = 0; s < SPW; s++) {
                if (sbase + sstep * s >= nso || (p.dbg_skip & 4)) continue;        // wave-uniform
                for (int ks = kslice; ks < kmax; ks += p.KS) {
                    const int ch = 4 * ks + kq;
                    const float *wdp = Wdl + ch * IRB_TAPP;
                    const v4f_irb w0 = *reinterpret_cast<const v4f_irb *>(wdp), w1v = *reinterpret_cast<const v4f_irb *>(wdp + 4),
                                  w2v = *reinterpret_cast<const v4f_irb *>(wdp + 8);
                    const float tap[9] = { w0.x, w0.y, w0.z, w0.w, w1v.x, w1v.y, w1v.z, w1v.w, w2v.x };
                    const float sd = w2v.y, bd = w2v.z;
                    const float *ep = E + ch * p.NPin + ebase[s];
                    v4f_irb dv = z;
#pragma unroll
                    for (int r = 0; r < 3; r++) {
                        const float *row = ep + r * p.EW;
                        if (S == 1) {
                            const v4f_irb u = *reinterpret_cast<const v4f_irb *>(row);
                            const v2f_irb u2 = *reinterpret_cast<const v2f_irb *>(row + 4);
                            const float x[6] = { u.x, u.y, u.z, u.w, u2.x, u2.y };
#pragma unroll
                            for (int q = 0; q < 4; q++)
#pragma unroll
                                for (int kx = 0; kx < 3; kx++) dv[q] = fmaf(tap[r * 3 + kx], x[q + kx], dv[q]);
                        } else {
                            const v4f_irb u = *reinterpret_cast<const v4f_irb *>(row), u1 = *reinterpret_cast<const v4f_irb *>(row + 4);
                            const float u8 = row[8];
                            const float x[9] = { u.x, u.y, u.z, u.w, u1.x, u1.y, u1.z, u1.w, u8 };
#pragma unroll
                            for (int q = 0; q < 4; q++)
#pragma unroll
                                for (int kx = 0; kx < 3; kx++) dv[q] = fmaf(tap[r * 3 + kx], x[2 * q + kx], dv[q]);
                        }
                    }
                    v4f_irb bq;
                    bq.x = irb_act(fmaf(dv.x, sd, bd), p.actd); bq.y = irb_act(fmaf(dv.y, sd, bd), p.actd);
                    bq.z = irb_act(fmaf(dv.z, sd, bd), p.actd); bq.w = irb_act(fmaf(dv.w, sd, bd), p.actd);
#pragma unroll
                    for (int t = 0; t < OT; t++) {
                        const float a = W2l[(ks * OT + t) * 64 + lane];
                        acc[s][t][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bq.x, acc[s][t][0], 0, 0, 0);
                        acc[s][t][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bq.y, acc[s][t][1], 0, 0, 0);
                        acc[s][t][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bq.z, acc[s][t][2], 0, 0, 0);
                        acc[s][t][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bq.w, acc[s][t][3], 0, 0, 0);
                    }
                }
            }
            IRB_TA(3);
            if (stream) {                                 // park the prefetched constants in the other buffer
                float *dstw = Wc + ((gc + 1) & 1) * p.CH;
#pragma unroll
                for (int k = 0; k < WPT; k++) if (tid + NT * k < ch4) reinterpret_cast<v4f_irb *>(dstw)[tid + NT * k] = wreg[k];
            }
        }

        // ---- split-K: reduce-SCATTER through LDS.  Every slice parks its partial sums as 16-byte vectors
        // ([slice][strip][t][r][lane] x 4 pixels); afterwards wave `kslice` owns the output rows r == kslice
        // (mod KS) of its strip, so the epilogue (residual loads, activation, stores) is spread over all KS waves.
        float *red = smem + p.red_off;
#if IRB_TRACE
        if (tile == (int)blockIdx.x) { IRB_T(4); if (p.dbg_t && threadIdx.x == 0) { p.dbg_t[blockIdx.x * 16 + 8] = tacc[0]; p.dbg_t[blockIdx.x * 16 + 9] = tacc[1]; p.dbg_t[blockIdx.x * 16 + 10] = tacc[2]; p.dbg_t[blockIdx.x * 16 + 11] = tacc[3]; } }
#endif
#undef IRB_TA
        if (p.KS > 1) {
            irb_barrier();                              // phase 3 of every wave finished with E
#pragma unroll
            for (int s = 0; s < SPW; s++) {
                const int strip = sbase + sstep * s;
                if (strip < nso) {
                    float *dst = red + ((kslice * nso + strip) * OT * 4) * 256 + lane * 4;
#pragma unroll
                    for (int t = 0; t < OT; t++)
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            const v4f_irb v = { acc[s][t][0][r], acc[s][t][1][r], acc[s][t][2][r], acc[s][t][3][r] };
                            *reinterpret_cast<v4f_irb *>(dst + (t * 4 + r) * 256) = v;
                        }
                }
            }
            irb_barrier();
        }

        if (tile == (int)blockIdx.x) IRB_T(5);
        // ---- epilogue: out = act2(s2 * acc + b2) [+ residual].  No lane-divergent control flow around the residual
        // loads (clamped offsets; a load under a lane predicate is waited for at once); the loop over the wave's output
        // rows stays rolled (unrolled, its address arithmetic is hoisted out of the tile loop and spills) and fetches
        // the next row's residual while the current row is finished.
#pragma unroll
        for (int s = 0; s < SPW; s++) {
            const int oy = oy0 + o_ty[s], ox = ox0 + o_tq[s] * 4, n = n0 + o_f[s];
            const bool valid = qok[s] && !(p.dbg_skip & 8) && n < p.N && o_f[s] < p.NF && oy < p.OH && o_ty[s] < p.TH && ox < p.OW;
            const int nvalid = valid ? min(min(4, p.OW - ox), p.TW - o_tq[s] * 4) : 0;
            const unsigned pbase = valid ? (unsigned)(n * (int)OHW + oy * p.OW + ox) : 0u;   // tensors < 2^32 bytes (checked at launch)
            const int strip = sbase + sstep * s;
            const int rstep = p.KS > 1 ? p.KS : 1, nrows = p.KS > 1 ? 4 / p.KS : 4;   // this wave owns rows kslice, kslice + KS, ...
            auto issue = [&](int r, v4f_irb (&dst)[OT]) {
#pragma unroll
                for (int t = 0; t < OT; t++) {
                    const unsigned off = (unsigned)min(16 * t + 4 * kq + r, p.oc - 1) * (unsigned)ocs + pbase;
                    if (p.vec_store) dst[t] = irb_ld<v4f_irb>(p.residual, nvalid == 4 ? off * 4u : 0u);
                    else {
#pragma unroll
                        for (int q = 0; q < 4; q++) dst[t][q] = irb_ld<float>(p.residual, q < nvalid ? (off + q) * 4u : 0u);
                    }
                }
            };
            auto finish = [&](int r, const v4f_irb (&res)[OT]) {
#pragma unroll
                for (int t = 0; t < OT; t++) {
                    const int o = 16 * t + 4 * kq + r;
                    v4f_irb v;
                    if (p.KS > 1) {
                        v = *reinterpret_cast<const v4f_irb *>(red + ((strip * OT + t) * 4 + r) * 256 + lane * 4);
                        for (int sl = 1; sl < p.KS; sl++)
                            v += *reinterpret_cast<const v4f_irb *>(red + (((sl * nso + strip) * OT + t) * 4 + r) * 256 + lane * 4);
                    } else {
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            const v4f_irb a = acc[s][t][q];
                            v[q] = r == 0 ? a.x : (r == 1 ? a.y : (r == 2 ? a.z : a.w));
                        }
                    }
                    const int oo = min(o, p.oc - 1);
                    const float sc = Sb2[2 * oo], bi = Sb2[2 * oo + 1];
                    v.x = irb_act(fmaf(v.x, sc, bi), p.act2); v.y = irb_act(fmaf(v.y, sc, bi), p.act2);
                    v.z = irb_act(fmaf(v.z, sc, bi), p.act2); v.w = irb_act(fmaf(v.w, sc, bi), p.act2);
                    if (p.residual) {
                        v.x = irb_act(v.x + res[t].x, p.res_act); v.y = irb_act(v.y + res[t].y, p.res_act);
                        v.z = irb_act(v.z + res[t].z, p.res_act); v.w = irb_act(v.w + res[t].w, p.res_act);
                    }
                    const unsigned off = (unsigned)oo * (unsigned)ocs + pbase;
                    if (o < p.oc) {
                        if (p.vec_store) { if (nvalid == 4) irb_st<v4f_irb>(p.out, off * 4u, v); }
                        else {
#pragma unroll
                            for (int q = 0; q < 4; q++) if (q < nvalid) irb_st<float>(p.out, (off + q) * 4u, v[q]);
                        }
                    }
                }
            };
            v4f_irb ra[OT], rb[OT];
            if (p.residual) issue(kslice, ra);
#pragma unroll 1
            for (int j = 0; j < nrows; j += 2) {
                const bool two = j + 1 < nrows;
                if (p.residual && two) issue(kslice + (j + 1) * rstep, rb);
                finish(kslice + j * rstep, ra);
                if (two) {
                    if (p.residual && j + 2 < nrows) issue(kslice + (j + 2) * rstep, ra);
                    finish(kslice + (j + 1) * rstep, rb);
                }
            }
        }
        if (tile == (int)blockIdx.x) IRB_T(6);
    }
    IRB_T(7);
#undef IRB_T
}
