// ffgpu_irb_wave.inc -- fused inverted-residual block, WAVE-AUTONOMOUS form (gfx950):
//
//     1x1 expand (ic -> ec, act1)  ->  depthwise 3x3 (stride 1|2, pad 1, actd)
//     -> 1x1 project (ec -> oc, act2)  [-> + residual, res_act]
//
// Same arithmetic as ffgpu_irb.inc (conv-v6.c:46-91, 96-287, 46-91 and ffcnn.c:418-423), different schedule.  The
// workgroup kernel of ffgpu_irb.inc spends most of its time at barriers and in dependent LDS -> MFMA chains with idle
// waves beside them (in-kernel timeline, profiles/r01_f_irb_timeline_workgroup_kernel.txt).  Here a WAVE owns a small output tile
// (<= 16 quads = 64 pixels) and runs the whole block for it with no workgroup barrier in the main loop:
//   * the input halo tile (NSI strips of 64 pixels, k4 channels) is loaded ONCE into registers as MFMA B operands
//     (one unaligned 16-byte global load per (strip, k-step) per lane);
//   * per group of 16 expanded channels: expand on v_mfma_f32_16x16x4_f32 -> wave-private LDS slice E[16][NSI*64]
//     (zero outside the image) -> depthwise 3x3 per lane straight into the B-operand layout -> project MFMAs into
//     the wave's accumulators;
//   * weights are read as ready-made MFMA A fragments from a packed global image (coalesced 256-byte loads, L2
//     resident), double-buffered in registers one group ahead; depthwise taps and scale'/bias' sit in a small LDS
//     table shared by the workgroup (staged once, the only barrier on the G == 1 path).
// Small planes (10x10, 20x20: too few pixels to fill 1024 SIMDs with 64-pixel tiles) split the channel GROUPS of one
// tile over the G waves of a workgroup instead (every wave holds the same input tile) and reduce the partial
// accumulators through LDS in a fixed order -- deterministic, no atomics.
// Independent waves in different phases overlap MFMA, VALU (depthwise) and memory latency on their SIMD; that overlap
// is what the barrier-synchronised kernel could not get.
typedef float v4f_w __attribute__((ext_vector_type(4)));
typedef float v2f_w __attribute__((ext_vector_type(2)));

struct IrbwP {
    const float *in; float *out; const float *residual;
    const float *pk;                 // packed image (irbw_pack_layout)
    int N, H, W, OH, OW, ic, ec, oc;
    float act1, actd, act2, res_act; // slopes: act(x) = max(x, slope * x)
    int TWq, TH, EW, EH;             // output tile: TWq quads x TH rows (TWq*TH <= 16); halo tile: EW (% 4 == 0) x EH
    int tiles_x, tiles_y;
    long ntiles;                     // N * tiles_y * tiles_x
    int ngroups, G, WPB;             // 16-channel groups; waves sharing one tile; tiles per workgroup when G == 1
    int o_w2, o_cs;                  // float offsets in pk: W2 fragments, shared constants (Wd | Sb1 | Sb2)
    int cs_floats;                   // floats of the shared constants (multiple of 4)
    int xl_off;                      // XL kernels: float offset of the workgroup's split input tile in LDS (behind the E slices / reduction room)
    int red_cap;                     // partial-accumulator slots that fit in the (dead) E slices
    unsigned in_elems;               // elements of `in` (< 2^30, checked at launch)
    int vec;                         // output row access: 4 = 16-byte, 2 = 8-byte, 1 = scalar
    int half_last;                   // the last group holds at most 8 real channels, packed into accumulator registers 0 / 1 of every lane (irbw_chan): its second
                                     // channel pair (registers 2 / 3: activation + E-slice store, depthwise stage, two project k-steps) is skipped (k_irbw only)
    unsigned m_ew;                   // ceil(2^32 / EW): halo-tile row of element e = umulhi(e, m_ew)
    unsigned m_tx, m_ty, m_twq;      // the same for tiles_x, tiles_y, TWq (0: divisor 1) -- a 64-bit '/' costs a hundred instructions per tile
    int xcd;                         // workgroup -> tile order XCD by XCD (irbw_xcd_block)
    unsigned long long *dbg_t;       // make TRACE=1 only: 8 timestamps per workgroup (wave 0)
};

// Workgroup ids go round robin over the 8 XCDs (each with its own L2): p.xcd gives every XCD a CONTIGUOUS range of the launch's workgroups instead, so that
// neighbouring tiles -- shared halo rows, the rows of the same frames, the block's weights -- sit behind one L2 (+1.0 % frames/s, same box, alternating)
__device__ __forceinline__ int irbw_xcd_block(int b, int nb) { const int q = nb >> 3, r = nb & 7, x = b & 7; return x * q + min(x, r) + (b >> 3); }
__device__ __forceinline__ int irbw_div(int i, unsigned m) { return m ? (int)__umulhi((unsigned)i, m) : i; }   // i / d, m = ceil(2^32 / d), i * d < 2^32

// ---- packed image: [W1: ngroups*KS1*64][W2: ngroups*4*OT*64][Wd: ECp/2 pairs * 24][Sb1: ECp/4 * 8][Sb2: OT*32], ECp = 16*ngroups
struct IrbwPackP {
    const float *w1, *wd, *w2; float *pk;
    int ic, ec, oc, k4, OT, ngroups;
    int x3;                          // W1 region in the split-bf16 form (below) instead of fp32 A fragments
    int half;                        // the last group's channels permuted (irbw_chan) so that its real ones sit in registers 0 / 1 of every lane
};
// Position rho = 4 kq + r of a group's 16 expanded channels = accumulator register r of lane group kq.  A last group with at most 8 real channels
// (ec % 16 in 1..8: the 160 -> 80 block's 24, the 20x20 blocks' 136) keeps channel c at position 4 (c & 3) + (c >> 2): the real ones fill registers
// 0 / 1 of all four lane groups and the kernel skips everything that belongs to registers 2 / 3 -- half of that group's vector and project work.
__host__ __device__ __forceinline__ int irbw_chan(int pos, int ngroups, int half)
{
    const int g = pos >> 4, rho = pos & 15;
    return (half && g == ngroups - 1) ? 16 * g + (rho >> 2) + 4 * (rho & 3) : pos;
}

// ---- "X3": the expand GEMM on the bf16 matrix cores with fp32-equivalent accuracy (round 4).
// On gfx950 v_mfma_f32_16x16x4_f32 runs at the fp32 VECTOR rate (32 MAC / cycle / SIMD: the same ALUs); the bf16 matrix
// cores are 16x faster.  An fp32 number is EXACTLY the sum of three bf16 numbers (24 significand bits = 3 x 8, by truncation:
// p0 = x & 0xffff0000, p1 = (x - p0) & 0xffff0000, p2 = x - p0 - p1, every subtraction exact), so
//     w * x = sum over (i, j) of w_i * x_j,   and the six terms with i + j <= 2 carry everything down to 2^-24 |w x|
// (the three dropped ones are <= 2^-23 |w x| together: the size of fp32's own rounding).  bf16 x bf16 products are exact in fp32 and
// the MFMA accumulates in fp32: the result differs from the fp32 chain like one summation order differs from another
// (tools/sim_split_bf16.py: worst |d| / tolerance 0.05-0.06 over the whole net, the same as an exact float64 sum; two-part
// splits -- 2^-16 -- exceed the tolerance and are not used).
// One v_mfma_f32_16x16x32_bf16 has 32 K slots = 8 per lane group kq; a lane holds the KS1 channels 4 j + kq of its pixel
// column as now, so its slots are (channel j, x part) and the A operand carries the matching weight part in the same slot:
//   KS1 = 4:  MFMA 0: [x0 j=0..3 | x1 j=0..3] x [w0 | w0]   MFMA 1: same B x [w1 | w1]   MFMA 2: [x0 | x2] x [w2 | w0]
//   KS1 = 2:  MFMA 0: [x0 | x0 | x0 | x1] x [w0 | w1 | w2 | w0]   MFMA 1: [x1 | x2 | - | -] x [w1 | w0 | 0 | 0]
//   KS1 = 6:  five MFMAs over the 18 (part, channel pair) x weight part slots (table in irbw_x3_term)
// i.e. 3 / 2 MFMAs of ~17 cycles instead of 4 / 2 of 32.  The input tile is split ONCE per tile; weights at plan time.
#include "ffgpu_x3_terms.h"
static bool irbw_x3_has(int ks1) { return ks1 == 2 || ks1 == 4 || ks1 == 6 || ks1 == 12; }
// ---- non-finite inputs (round 6; VERDICT r05 item 5): the reference propagates a +-Inf input as w * Inf = +-Inf for every w != 0 (conv-v0.c:7-31,
// utils.h:15-23); the split form must not turn it into NaN.  Two halves:
//   * the input side: x - trunc(x) of an Inf is NaN -- its residual parts are ZERO instead (x3_resid: one v_cmp_class + one v_cndmask per split
//     value); the parts of +-Inf are (+-Inf, 0, 0), a NaN input keeps poisoning through its first part;
//   * the weight side: the Inf then meets w0, w1 AND w2 (terms w0 x0, w1 x0, w2 x0), and a part that happens to be zero -- w1 = w2 = 0 for a weight that
//     is a bf16 number, w2 = 0 for one weight in 256 -- would make 0 * Inf = NaN.  All parts of a truncation split carry the sign of w, so a zero part
//     of a non-zero weight is packed as sign(w) 2^(e - 40) (e: w's exponent; from |w| >= 2^-86 up): a relative perturbation of 2^-40 per part, 16 bits
//     below fp32's own rounding, and w_i * Inf = sign(w) Inf in every term.  A weight that IS zero keeps three zero parts: 0 * Inf = NaN, as in the reference.
// -DX3_INF_EXACT=0 (lab builds) restores round 5's arithmetic (Inf input -> NaN) to price the difference.
#ifndef X3_INF_EXACT
#define X3_INF_EXACT 1
#endif
#ifndef X3_INF_W              // lab builds: the weight half / the input half alone
#define X3_INF_W X3_INF_EXACT
#endif
#ifndef X3_INF_X
#define X3_INF_X X3_INF_EXACT
#endif
#ifndef X3_INF_X_FUSED        // lab builds: the input half in the fused blocks / in k_conv_x3 alone
#define X3_INF_X_FUSED X3_INF_X
#endif
#ifndef X3_INF_X_CONV
#define X3_INF_X_CONV X3_INF_X
#endif
__device__ __forceinline__ float x3_resid(float x)                  // x - trunc_bf16(x), exact; 0 for +-Inf
{
#if X3_WHATIF_NOSPLIT
    return 0.f;                                                       // (parts (x0, 0, 0): bf16-grade results, the detections stay roughly what they are)
#endif
    const float r = x - __uint_as_float(__float_as_uint(x) & 0xffff0000u);
#if X3_INF_X
    return __builtin_amdgcn_classf(x, 0x204) ? 0.f : r;
#else
    return r;
#endif
}
// The fused blocks are bound by vector issue, and two more instructions per split value cost 1 % of the whole net (same box, alternating: 203.2 k against
// 205.3 k frames/s).  They split a whole tile at once, so the test moves to the WAVE: m = max |x| over the tile's values (v_max3_f32 with |.| modifiers: half an
// instruction per value, NaNs ignored -- a NaN poisons through its first part anyway), one ballot, and the cndmask form of the split only in a wave that
// holds an Inf (x3_resid_t<true>); every other wave runs round 5's instruction stream.
// -DX3_WHATIF_NOSPLIT=1 (lab builds, WRONG results): the consumers' split costs nothing -- x1 = x2 = 0 -- to price a producer-side split (VERDICT r05 item 3)
#ifndef X3_WHATIF_NOSPLIT
#define X3_WHATIF_NOSPLIT 0
#endif
__device__ __forceinline__ float x3_resid2(float r)                 // the third part: r - trunc_bf16(r), exact, <= 8 significant bits
{
#if X3_WHATIF_NOSPLIT
    return 0.f;
#else
    return r - __uint_as_float(__float_as_uint(r) & 0xffff0000u);
#endif
}
template <bool INF> __device__ __forceinline__ float x3_resid_t(float x)
{
#if X3_WHATIF_NOSPLIT
    return 0.f;                                                       // (parts (x0, 0, 0): bf16-grade results, the detections stay roughly what they are)
#endif
    const float r = x - __uint_as_float(__float_as_uint(x) & 0xffff0000u);
    return (INF && X3_INF_X && __builtin_amdgcn_classf(x, 0x204)) ? 0.f : r;
}
__device__ __forceinline__ float x3_amax3(float m, float a, float b) { float d; asm("v_max3_f32 %0, |%1|, |%2|, %3" : "=v"(d) : "v"(a), "v"(b), "v"(m)); return d; }
__device__ __forceinline__ bool x3_wave_has_inf(float m)
{
#if X3_INF_X
    return __builtin_amdgcn_ballot_w64(m == __builtin_inff()) != 0ull;
#else
    return false;
#endif
}
// upper 16 bits of part `part` of the exact three-way split of w
__device__ __forceinline__ unsigned irbw_x3_part(float w, int part)
{
    const unsigned uw = __float_as_uint(w);
    const unsigned u0 = uw & 0xffff0000u;
    if (part == 0) return u0 >> 16;
    const float r = w - __uint_as_float(u0);
    const unsigned u1 = __float_as_uint(r) & 0xffff0000u;
    unsigned v = (part == 1 ? u1 : __float_as_uint(r - __uint_as_float(u1))) >> 16;
#if X3_INF_W
    const unsigned ex = (uw >> 23) & 0xffu;
    if ((v & 0x7fffu) == 0 && ex >= 41u && ex != 255u) v = ((uw >> 16) & 0x8000u) | ((ex - 40u) << 7);
#endif
    return v;
}

__global__ void k_irbw_pack(IrbwPackP p)
{
    const int ks1 = p.k4 >> 2, ecp = p.ngroups * 16, nm = irbw_x3_nm(ks1);
    const int n1 = p.x3 ? p.ngroups * nm * 256 : p.ngroups * ks1 * 64, n2 = p.ngroups * 4 * p.OT * 64, n3 = ecp * 12, n4 = ecp * 2, n5 = p.OT * 32;
    const int rl1 = p.k4 + 4, rl2 = ((p.ec + 3) & ~3) + 4;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n1 + n2 + n3 + n4 + n5; i += gridDim.x * blockDim.x) {
        float v = 0.f;
        int j = i;
        if (j < n1 && p.x3) {                                                  // [group][MFMA][lane][4 dwords] of bf16 pairs
            const int d = j & 3, l = (j >> 2) & 63, m = (j >> 8) % nm, g = (j >> 8) / nm;
            const int e = irbw_chan(16 * g + (l & 15), p.ngroups, p.half), kq = l >> 4;
            const IrbwX3Term t = irbw_x3_term(ks1, m, d);
            unsigned bits = 0;
            if (t.wp >= 0 && e < p.ec) {
                const float wa = p.w1[(long)e * rl1 + 4 * (2 * t.pair) + kq], wb = p.w1[(long)e * rl1 + 4 * (2 * t.pair + 1) + kq];   // zero beyond ic
                bits = irbw_x3_part(wa, t.wp) | (irbw_x3_part(wb, t.wp) << 16);
            }
            v = __uint_as_float(bits);
        } else if (j < n1) {
            const int l = j & 63, ks = (j >> 6) % ks1, g = (j >> 6) / ks1;
            const int e = irbw_chan(16 * g + (l & 15), p.ngroups, p.half), ci = 4 * ks + (l >> 4);
            if (e < p.ec) v = p.w1[(long)e * rl1 + ci];                    // rows are zero padded up to k4
        } else if ((j -= n1) < n2) {
            const int l = j & 63, t = (j >> 6) % p.OT, ks = ((j >> 6) / p.OT) & 3, g = (j >> 6) / (p.OT * 4);
            const int o = 16 * t + (l & 15), e = irbw_chan(16 * g + 4 * (l >> 4) + ks, p.ngroups, p.half);    // k index kq of step ks <-> channel 4kq + ks
            if (o < p.oc && e < p.ec) v = p.w2[(long)o * rl2 + e];
        } else if ((j -= n2) < n3) {                                           // [pair][k = tap 0..8, scale', bias', pad][channel of the pair]
            const int pr = j / 24, k = (j % 24) >> 1, e = irbw_chan(2 * pr + (j & 1), p.ngroups, p.half);
            if (e < p.ec && k < 11) v = k < 9 ? p.wd[(long)e * 16 + k] : p.wd[(long)e * 16 + 12 + (k - 9)];
        } else if ((j -= n3) < n4) {                                           // [4 channels][scale' x4, bias' x4]
            const int e = irbw_chan(4 * (j >> 3) + (j & 3), p.ngroups, p.half);
            if (e < p.ec) v = p.w1[(long)e * rl1 + p.k4 + ((j >> 2) & 1)];
        } else {
            j -= n4;
            const int o = j >> 1;
            if (o < p.oc) v = p.w2[(long)o * rl2 + (rl2 - 4) + (j & 1)];
        }
        p.pk[i] = v;
    }
}

typedef unsigned u4_w2 __attribute__((ext_vector_type(4)));
typedef __bf16 v8bf_w2 __attribute__((ext_vector_type(8)));
template <class T> __device__ __forceinline__ T irbw_ld(const void *base, unsigned byte_off)
{ return *reinterpret_cast<const T *>(reinterpret_cast<const char *>(base) + byte_off); }
template <class T> __device__ __forceinline__ void irbw_st(void *base, unsigned byte_off, T v)
{ *reinterpret_cast<T *>(reinterpret_cast<char *>(base) + byte_off) = v; }
__device__ __forceinline__ float irbw_act(float x, float slope, float floor) { return act_max(x, slope * x, floor); }

// KS1 = k-steps of the expand GEMM (ALIGN(ic,4)/4), OT = ceil(oc/16), S = stride, NSI = 64-pixel strips of the halo
// tile, BIG = needs more than 128 VGPRs (two waves per SIMD instead of four)
template <int KS1, int OT, int S, int NSI, bool BIG, bool X3 = false, bool XL = false>
#ifndef IRBW_MID_WAVES         // waves per SIMD the 160 -> 80 block's instantiation <1, 1, 2, 3, false> is compiled for (round 6: its 51 KB of LDS per 4-wave workgroup allow three anyway)
#define IRBW_MID_WAVES 3
#endif
__global__ void __launch_bounds__(512, BIG ? 2 : (KS1 == 1 && OT == 1 && S == 2 && NSI == 3 ? IRBW_MID_WAVES : 4)) k_irbw(IrbwP p)
{
    static_assert(!XL || (X3 && KS1 == 12), "XL: the LDS-resident split tile exists for 48 input channels");
    constexpr int NM = X3 ? irbw_x3_nm(KS1) : 1;
    struct W1T { float f[X3 ? 1 : KS1]; u4_w2 x[X3 ? NM : 1]; };     // W1 of a group: KS1 fp32 A fragments, or (X3) NM x 16 bytes of bf16 pairs per lane
#if IRB_TRACE
#define IRBW_T(k) do { if (p.dbg_t && threadIdx.x == 0 && blockIdx.x < 4096) p.dbg_t[blockIdx.x * 16 + (k)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define IRBW_T(k) do { } while (0)
#endif
    IRBW_T(0);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kq = lane >> 4, jq = lane & 15;
    // the relu floors (act_floor), once and outside every lane condition: the scalar read is a convergent operation, and under a lane condition hipcc branches around it
    const float fl_act1 = act_floor(p.act1), fl_actd = act_floor(p.actd), fl_act2 = act_floor(p.act2), fl_res = act_floor(p.res_act);
    constexpr int NPw = NSI * 64, NQ = NSI * 16;                 // pixels / pixel quads of the halo tile
    constexpr bool PIPE = !X3 && BIG && NSI * 16 + NSI * KS1 * 4 + OT * 16 + 2 * (KS1 + 4 * OT) <= 140;    // the pipelined form keeps a second set of expand accumulators
    const int ecp = p.ngroups * 16;
    const float *Wd = smem, *Sb1 = smem + ecp * 12, *Sb2 = Sb1 + ecp * 2;     // Wd: [ngroups*8 pairs][24], Sb1: [ngroups*4][s x4, b x4]
    float *Ew = smem + p.cs_floats + wid * (16 * NPw);
    const v4f_w z = { 0.f, 0.f, 0.f, 0.f };

    // ---- shared constants: loads issued first (up to 3 x 16 bytes per thread in flight underneath the input-tile and
    // weight loads), parked in LDS just before the barrier
    const int cs4 = p.cs_floats >> 2, nthr = (int)blockDim.x;
    v4f_w cst[3];
#pragma unroll
    for (int u = 0; u < 3; u++) cst[u] = irbw_ld<v4f_w>(p.pk, (unsigned)(p.o_cs + 4 * min(tid + u * nthr, cs4 - 1)) * 4u);

    // ---- this wave's tile
    const int bid = p.xcd ? irbw_xcd_block((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x;
    const int tile = p.G > 1 ? bid : bid * p.WPB + wid;
    const bool active = tile < (int)p.ntiles;                  // wave-uniform
    const int tt = active ? tile : 0;
    const int trow = irbw_div(tt, p.m_tx), tx_i = tt - trow * p.tiles_x;
    const int n = irbw_div(trow, p.m_ty), ty_i = trow - n * p.tiles_y;
    const int oy0 = ty_i * p.TH, ox0 = tx_i * p.TWq * 4;
    const int gy0 = oy0 * S - 1, gx0 = ox0 * S - 1;            // image coordinates of halo-tile element (0,0)
    const bool interior = gy0 >= 0 && gx0 >= 0 && gy0 + p.EH <= p.H && gx0 + p.EW <= p.W;

    // ---- input halo tile -> registers (B operands of the expand MFMAs); validity bits of its pixels
    v4f_w xin[XL ? 1 : NSI][KS1];
    unsigned mbits = 0;
    const int plane = p.H * p.W;
    // one strip's quads of this lane (all its channels 4 ks + kq): loaded from a clamped address; a quad that starts before the first /
    // ends after the last element of the whole tensor is moved back into place afterwards (at most two lanes of the whole launch)
    auto load_strip = [&](int si, v4f_w (&x)[KS1]) {
        const int e = si * 64 + 4 * jq;
        const int iy = (int)__umulhi((unsigned)e, p.m_ew), ix = e - iy * p.EW;     // e / EW (exact: e * EW < 2^32)
        const int rowidx = (n * p.H + min(max(gy0 + iy, 0), p.H - 1)) * p.W + gx0 + ix;
        bool anyfix = false;
#pragma unroll
        for (int ks = 0; ks < KS1; ks++) {
            const int idx = min(4 * ks + kq, p.ic - 1) * (p.N * plane) + rowidx;
            const int cl = min(max(idx, 0), (int)p.in_elems - 4);
            anyfix |= cl != idx;
            x[ks] = irbw_ld<v4f_w>(p.in, (unsigned)cl * 4u);
        }
        if (anyfix) {
#pragma unroll
            for (int ks = 0; ks < KS1; ks++) {
                const int idx = min(4 * ks + kq, p.ic - 1) * (p.N * plane) + rowidx;
                const int d = min(max(idx, 0), (int)p.in_elems - 4) - idx;     // loaded[q - d] is element idx + q
                if (d != 0) {
                    const v4f_w l = x[ks];
                    v4f_w w = z;
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const int s = q - d;
                        w[q] = s == 0 ? l.x : (s == 1 ? l.y : (s == 2 ? l.z : (s == 3 ? l.w : 0.f)));
                    }
                    x[ks] = w;
                }
            }
        }
    };
#pragma unroll
    for (int si = 0; si < NSI; si++) {
        if (!interior) {                                           // wave-uniform: interior tiles keep every pixel
            const int e = si * 64 + 4 * jq;
            const int iy = (int)__umulhi((unsigned)e, p.m_ew), ix = e - iy * p.EW;
            const int gy = gy0 + iy, gx = gx0 + ix;
            const bool rowok = (iy < p.EH) & ((unsigned)gy < (unsigned)p.H);
#pragma unroll
            for (int q = 0; q < 4; q++) mbits |= (rowok & ((unsigned)(gx + q) < (unsigned)p.W)) ? 1u << (si * 4 + q) : 0u;
        }
        if (!XL) load_strip(si, xin[XL ? 0 : si]);
    }
    // channels past ic (K is padded to 4 KS1) re-read the last channel's pixels (the clamp in load_strip).  Their weights are zero, but 0 * Inf is NaN where
    // the reference has no term at all: they count as zero, like the padded k-units of the other split kernels
    const bool kpad = 4 * (KS1 - 1) + kq >= p.ic;
    if (!XL && kpad) {
#pragma unroll
        for (int si = 0; si < NSI; si++) xin[si][KS1 - 1] = z;
    }
    // the exact three-way split of a value as the upper halves of three words (X3)
    auto split3 = [&](auto INF, float x, unsigned &u0, unsigned &u1, unsigned &u2) {
        const float r = x3_resid_t<decltype(INF)::value>(x);                          // exact (INF: 0 for +-Inf)
        const float r2 = x3_resid2(r);                                                      // exact, <= 8 significant bits
        u0 = __float_as_uint(x); u1 = __float_as_uint(r); u2 = __float_as_uint(r2);
    };
    // XL: the waves of the workgroup hold the same tile -- each produces a part of its split image in LDS (item = strip, pixel pair)
    unsigned *XI = reinterpret_cast<unsigned *>(smem) + p.xl_off;
    if (XL && active) {
        for (int item = wid; item < NSI * 2; item += p.G) {
            const int si = item >> 1, qh = item & 1;
            v4f_w x[KS1];
            load_strip(si, x);
            if (kpad) x[KS1 - 1] = z;
            float amax = 0.f;
#pragma unroll
            for (int ks = 0; ks < KS1; ks++) amax = x3_amax3(x3_amax3(amax, x[ks].x, x[ks].y), x[ks].z, x[ks].w);
            const bool xinf = X3_INF_X_FUSED && x3_wave_has_inf(amax);                  // wave-uniform
#pragma unroll
            for (int qq = 0; qq < 2; qq++) {
                const int q = 2 * qh + qq;
                unsigned b[3][KS1];
                if (xinf) {
#pragma unroll
                    for (int ks = 0; ks < KS1; ks++) { const float v = qh ? (qq ? x[ks].w : x[ks].z) : (qq ? x[ks].y : x[ks].x); split3(std::true_type{}, v, b[0][ks], b[1][ks], b[2][ks]); }
                } else {
#pragma unroll
                    for (int ks = 0; ks < KS1; ks++) { const float v = qh ? (qq ? x[ks].w : x[ks].z) : (qq ? x[ks].y : x[ks].x); split3(std::false_type{}, v, b[0][ks], b[1][ks], b[2][ks]); }
                }
                u4_w2 o[5];
#pragma unroll
                for (int i = 0; i < IRBW_XL_DW; i++) {
                    const int pt = i < 18 ? i / 6 : 0, pr = i < 18 ? i % 6 : i - 14;            // x0 a-f | x1 a-f | x2 a-f | x0 e f
                    o[i >> 2][i & 3] = __builtin_amdgcn_perm(b[pt][2 * pr + 1], b[pt][2 * pr], 0x07060302u);
                }
                u4_w2 *dst = reinterpret_cast<u4_w2 *>(XI + ((si * 4 + q) * 64 + lane) * IRBW_XL_DW);
#pragma unroll
                for (int i = 0; i < 5; i++) dst[i] = o[i];
            }
        }
    }
    // X3: the tile's exact three-way split, packed as bf16 pairs of the lane's channels: xp[strip][pixel][part][pair]
    unsigned xp[X3 && !XL ? NSI : 1][4][3][X3 && !XL ? KS1 / 2 : 1];
    if (X3 && !XL) {
        float amax = 0.f;
#pragma unroll
        for (int si = 0; si < NSI; si++)
#pragma unroll
            for (int ks = 0; ks < KS1; ks++) amax = x3_amax3(x3_amax3(amax, xin[si][ks][0], xin[si][ks][1]), xin[si][ks][2], xin[si][ks][3]);
        auto split_tile = [&](auto INF) {
#pragma unroll
            for (int si = 0; si < NSI; si++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    unsigned b[3][KS1];
#pragma unroll
                    for (int ks = 0; ks < KS1; ks++) split3(INF, xin[si][ks][q], b[0][ks], b[1][ks], b[2][ks]);
#pragma unroll
                    for (int pt = 0; pt < 3; pt++)
#pragma unroll
                        for (int pr = 0; pr < KS1 / 2; pr++) xp[si][q][pt][pr] = __builtin_amdgcn_perm(b[pt][2 * pr + 1], b[pt][2 * pr], 0x07060302u);
                }
        };
        if (X3_INF_X_FUSED && x3_wave_has_inf(amax)) split_tile(std::true_type{}); else split_tile(std::false_type{});      // (wave-uniform: see x3_resid_t)
    }
    auto bop = [&](int si, int q, int m) -> v8bf_w2 {
        u4_w2 u;
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const IrbwX3Term t = irbw_x3_term(KS1, m, d);
            u[d] = t.wp < 0 ? 0u : xp[X3 && !XL ? si : 0][q][t.xp][X3 && !XL ? t.pair : 0];
        }
        return __builtin_bit_cast(v8bf_w2, u);
    };
    // this lane's output quad and where its 3x3 windows start in the E slice
    const int ty = irbw_div(jq, p.m_twq), tq = jq - ty * p.TWq;
    const bool qvalid = ty < p.TH;
    const int ebase = qvalid ? ty * S * p.EW + tq * 4 * S : 0;

    // ---- output rows: register r of tile t holds channel 16t + 4kq + r for this lane's quad
    const int oy = oy0 + ty, ox = ox0 + tq * 4;
    const bool valid = active && qvalid && oy < p.OH && ox < p.OW;
    const int nvalid = valid ? min(4, p.OW - ox) : 0;
    const unsigned pbase = valid ? (unsigned)((n * p.OH + oy) * p.OW + ox) : 0u;
    const unsigned ocs = (unsigned)(p.N * p.OH * p.OW);
    auto res_issue = [&](int t, int r) -> v4f_w {
        const unsigned off = ((unsigned)min(16 * t + 4 * kq + r, p.oc - 1) * ocs + pbase) * 4u;
        v4f_w v;
        if (p.vec == 4) v = irbw_ld<v4f_w>(p.residual, nvalid == 4 ? off : 0u);
        else if (p.vec == 2) {
            const v2f_w a = irbw_ld<v2f_w>(p.residual, nvalid >= 2 ? off : 0u), b = irbw_ld<v2f_w>(p.residual, nvalid == 4 ? off + 8u : 0u);
            v = (v4f_w){ a.x, a.y, b.x, b.y };
        } else {
#pragma unroll
            for (int q = 0; q < 4; q++) v[q] = irbw_ld<float>(p.residual, q < nvalid ? off + 4u * q : 0u);
        }
        return v;
    };
    // one output tile per lane row (OT == 1) and no group split: all four residual rows are fetched up front
    constexpr bool RPRE = OT == 1 && KS1 <= 2;                  // (the 16 registers are not there for the wider shapes)
    v4f_w rpre[4];
    if (RPRE && p.G == 1 && p.residual) {
#pragma unroll
        for (int r = 0; r < 4; r++) rpre[r] = res_issue(0, r);
    }
    // ---- weights of one group as MFMA A fragments; the first group's ride along with the loads above
    auto loadw1 = [&](int g, W1T &w1) {
        if (X3) {
#pragma unroll
            for (int m = 0; m < NM; m++) w1.x[m] = irbw_ld<u4_w2>(p.pk, (unsigned)((g * NM + m) * 64 + lane) * 16u);
        } else {
#pragma unroll
            for (int ks = 0; ks < KS1; ks++) w1.f[ks] = irbw_ld<float>(p.pk, (unsigned)((g * KS1 + ks) * 64 + lane) * 4u);
        }
    };
    auto loadw = [&](int g, W1T &w1, float (&w2)[4 * OT]) {
        loadw1(g, w1);
#pragma unroll
        for (int i = 0; i < 4 * OT; i++) w2[i] = irbw_ld<float>(p.pk, (unsigned)(p.o_w2 + (g * 4 * OT + i) * 64 + lane) * 4u);
    };
    W1T w1a, w1b;
    float w2a[4 * OT], w2b[4 * OT];
    const int gstep = p.G > 1 ? p.G : 1, gfirst = p.G > 1 ? wid : 0;
    loadw(min(gfirst, p.ngroups - 1), w1a, w2a);

#pragma unroll
    for (int u = 0; u < 3; u++) if (tid + u * nthr < cs4) reinterpret_cast<v4f_w *>(smem)[tid + u * nthr] = cst[u];
    for (int i = tid + 3 * nthr; i < cs4; i += nthr)             // (larger tables than any block of the net has)
        reinterpret_cast<v4f_w *>(smem)[i] = irbw_ld<v4f_w>(p.pk, (unsigned)(p.o_cs + 4 * i) * 4u);
    IRBW_T(1);
    __syncthreads();                                            // shared constants visible
    IRBW_T(2);

    v4f_w acc[OT][4];
#pragma unroll
    for (int t = 0; t < OT; t++)
#pragma unroll
        for (int q = 0; q < 4; q++) acc[t][q] = z;

    // ---- one group of 16 expanded channels, in four pieces: expand MFMAs -> [activation, mask, E slice] ->
    // [depthwise from the E slice] -> project MFMAs.
    // All element-wise work runs on PAIRS of channels (v_pk_fma_f32 / v_pk_mul_f32): the expand side pairs the
    // accumulator registers (2rp, 2rp+1) = channels (4kq+2rp, +1); the E slice interleaves such a pair per pixel,
    //     E2[pair p = 2kq + rp][pixel][2],
    // and the depthwise stage of lane kq, step m takes pair p = 2kq + m, i.e. channels 4kq+2m and 4kq+2m+1, which
    // feed the project k-steps 2m and 2m+1 at k index kq (W2 is packed for that order).
    const unsigned mb = interior ? 0xffffffffu : mbits;          // branch-free masking: interior tiles keep every pixel
    auto expand_strip = [&](int si, const W1T &w1, v4f_w (&a4s)[4]) {
#pragma unroll
            for (int q = 0; q < 4; q++) a4s[q] = z;
            if (XL) {
                // operands from the workgroup's LDS image: five 16-byte windows per (strip, pixel); two pixels' chains interleaved
#pragma unroll
                for (int qh = 0; qh < 2; qh++) {
                    u4_w2 o[2][5];
#pragma unroll
                    for (int qq = 0; qq < 2; qq++) {
                        const u4_w2 *src = reinterpret_cast<const u4_w2 *>(XI + ((si * 4 + 2 * qh + qq) * 64 + lane) * IRBW_XL_DW);
#pragma unroll
                        for (int i = 0; i < 5; i++) o[qq][i] = src[i];
                    }
#pragma unroll
                    for (int m = 0; m < NM; m++) {
                        const v8bf_w2 A = __builtin_bit_cast(v8bf_w2, w1.x[m]);
#pragma unroll
                        for (int qq = 0; qq < 2; qq++)
                            a4s[2 * qh + qq] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, __builtin_bit_cast(v8bf_w2, o[qq][irbw_xl_op(m)]), a4s[2 * qh + qq], 0, 0, 0);
                    }
                }
            } else if (X3) {
#pragma unroll
                for (int m = 0; m < NM; m++) {
                    const v8bf_w2 A = __builtin_bit_cast(v8bf_w2, w1.x[m]);
#pragma unroll
                    for (int q = 0; q < 4; q++) a4s[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, bop(si, q, m), a4s[q], 0, 0, 0);
                }
            } else {
#pragma unroll
                for (int ks = 0; ks < KS1; ks++) {
                    a4s[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.f[ks], xin[si][ks].x, a4s[0], 0, 0, 0);
                    a4s[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.f[ks], xin[si][ks].y, a4s[1], 0, 0, 0);
                    a4s[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.f[ks], xin[si][ks].z, a4s[2], 0, 0, 0);
                    a4s[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.f[ks], xin[si][ks].w, a4s[3], 0, 0, 0);
                }
            }
    };
    auto expand_mfma = [&](const W1T &w1, v4f_w (&a4)[NSI][4]) {
#pragma unroll
        for (int si = 0; si < NSI; si++) expand_strip(si, w1, a4[si]);
    };
    auto halfg = [&](int g) { return p.half_last && g == p.ngroups - 1; };          // wave-uniform
    auto store_strip = [&](int g, int si, const v4f_w (&a4s)[4]) {
        const float *sbp = Sb1 + (g * 4 + kq) * 8;
        const v4f_w S4 = *reinterpret_cast<const v4f_w *>(sbp), B4 = *reinterpret_cast<const v4f_w *>(sbp + 4);
        const v2f_w sc[2] = { { S4.x, S4.y }, { S4.z, S4.w } }, bi[2] = { { B4.x, B4.y }, { B4.z, B4.w } };
#pragma unroll
        for (int rp = 0; rp < 2; rp++) {
            if (rp == 1 && halfg(g)) break;                       // registers 2 / 3 hold padding (half_last)
            v2f_w y[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const v2f_w a = rp == 0 ? (v2f_w){ a4s[q].x, a4s[q].y } : (v2f_w){ a4s[q].z, a4s[q].w };
                const v2f_w t = a * sc[rp] + bi[rp];
                const v2f_w u = t * p.act1;
                const bool in = (mb >> (si * 4 + q)) & 1u;        // the depthwise layer pads the EXPANDED tensor
                y[q] = (v2f_w){ in ? act_max(t.x, u.x, fl_act1) : 0.f, in ? act_max(t.y, u.y, fl_act1) : 0.f };
            }
            // E slice layout: [pair][half of the pixel quad][quad][2 pixels][2 channels] -- each of the two stores below
            // puts 16 bytes per lane at a 16-byte lane stride (a [pair][pixel][2] layout made them 32-byte strided:
            // 4-way bank conflicts, half of the LDS time of the block)
            float *dst = Ew + ((2 * kq + rp) * 2 * NQ + si * 16 + jq) * 4;
            *reinterpret_cast<v4f_w *>(dst) = (v4f_w){ y[0].x, y[0].y, y[1].x, y[1].y };
            *reinterpret_cast<v4f_w *>(dst + NQ * 4) = (v4f_w){ y[2].x, y[2].y, y[3].x, y[3].y };
        }
    };
    auto expand_store = [&](int g, const v4f_w (&a4)[NSI][4]) {
#pragma unroll
        for (int si = 0; si < NSI; si++) store_strip(g, si, a4[si]);
    };
    auto dw_stage = [&](int g, int m, v2f_w (&bq)[4]) {
        const int pr = 2 * kq + m;
        const float *wdp = Wd + (g * 8 + pr) * 24;                 // [tap 0..8, scale', bias'][2 channels]
        v4f_w T[6];
#pragma unroll
        for (int i = 0; i < 6; i++) T[i] = *reinterpret_cast<const v4f_w *>(wdp + 4 * i);
        const v2f_w tap[9] = { { T[0].x, T[0].y }, { T[0].z, T[0].w }, { T[1].x, T[1].y }, { T[1].z, T[1].w }, { T[2].x, T[2].y },
                               { T[2].z, T[2].w }, { T[3].x, T[3].y }, { T[3].z, T[3].w }, { T[4].x, T[4].y } };
        const v2f_w sd = { T[4].z, T[4].w }, bd = { T[5].x, T[5].y };
        const float *ep = Ew + (pr * 2 * NQ + (ebase >> 2)) * 4;          // window start = a whole quad (ebase % 4 == 0)
        v2f_w dv[4] = { { 0.f, 0.f }, { 0.f, 0.f }, { 0.f, 0.f }, { 0.f, 0.f } };
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const float *row = ep + r * p.EW;                             // EW / 4 quads further, 4 floats per quad-half
            constexpr int NX = S == 1 ? 6 : 9;
            v2f_w x[NX + 1];
#pragma unroll
            for (int i = 0; i < NX / 2; i++) {                            // pixels 2i, 2i+1: quad i/2, half i&1
                const v4f_w u = *reinterpret_cast<const v4f_w *>(row + ((i & 1) * NQ + (i >> 1)) * 4);
                x[2 * i] = (v2f_w){ u.x, u.y }; x[2 * i + 1] = (v2f_w){ u.z, u.w };
            }
            if (NX & 1) x[NX - 1] = *reinterpret_cast<const v2f_w *>(row + ((NX - 1) >> 2) * 4);   // pixel 8: quad 2, half 0, first pixel
#pragma unroll
            for (int q = 0; q < 4; q++)
#pragma unroll
                for (int kx = 0; kx < 3; kx++) dv[q] += tap[r * 3 + kx] * x[S * q + kx];
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const v2f_w t = dv[q] * sd + bd;
            const v2f_w u = t * p.actd;
            bq[q] = (v2f_w){ act_max(t.x, u.x, fl_actd), act_max(t.y, u.y, fl_actd) };
        }
    };
    auto project = [&](const float (&w2)[4 * OT], int m, const v2f_w (&bq)[4]) {
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int t = 0; t < OT; t++) {
                const float a = w2[(2 * m + j) * OT + t];
                acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, j ? bq[0].y : bq[0].x, acc[t][0], 0, 0, 0);
                acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, j ? bq[1].y : bq[1].x, acc[t][1], 0, 0, 0);
                acc[t][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, j ? bq[2].y : bq[2].x, acc[t][2], 0, 0, 0);
                acc[t][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, j ? bq[3].y : bq[3].x, acc[t][3], 0, 0, 0);
            }
    };
    auto loadw2 = [&](int g, float (&w2)[4 * OT]) {
#pragma unroll
        for (int i = 0; i < 4 * OT; i++) w2[i] = irbw_ld<float>(p.pk, (unsigned)(p.o_w2 + (g * 4 * OT + i) * 64 + lane) * 4u);
    };
    // this wave's groups: g(i) = gfirst + i * gstep, i < ngw (clamped for the prefetches that run past the end)
    const int ngw = gfirst < p.ngroups ? (p.ngroups - gfirst + gstep - 1) / gstep : 0;
    auto gi = [&](int i) { return min(gfirst + i * gstep, p.ngroups - 1); };

    if (active && ngw > 0) {
        if (PIPE) {
            // Software pipeline over the groups, one E slice: while the depthwise stage of group i works from LDS on the
            // VALU, the matrix cores already run the expand GEMM of group i+1 (its results wait in registers); then the
            // project MFMAs of group i run beside the activation / E-slice stores of group i+1.  A lone wave -- most of
            // these launches leave a SIMD one or two -- otherwise executes MFMA, VALU and LDS phases strictly in turn.
            // Weights: group index i uses w1[i & 1], w2[i & 1] (w1a/w2a even, w1b/w2b odd); a body of parity P loads
            // W1 of group i+2 and W2 of group i+1.
            v4f_w a4[NSI][4];
            v2f_w bq0[4], bq1[4];
            loadw1(gi(1), w1b);
            expand_mfma(w1a, a4);
            expand_store(gi(0), a4);
            auto body = [&](int i, W1T &w1cur, float (&w2cur)[4 * OT], W1T &w1nxt, float (&w2nxt)[4 * OT]) {
                // w1nxt holds W1(i+1) (loaded an iteration ago); w2cur holds W2(i); refill: W2(i+1) -> w2nxt, W1(i+2) -> w1cur
                loadw2(gi(i + 1), w2nxt);
                __builtin_amdgcn_sched_barrier(0);
                expand_mfma(w1nxt, a4);                            // group i+1 on the matrix cores ...
                dw_stage(gi(i), 0, bq0);                           // ... beside group i's depthwise stage
                if (!halfg(gi(i))) dw_stage(gi(i), 1, bq1);
                __builtin_amdgcn_sched_barrier(0);
                loadw1(gi(i + 2), w1cur);
                project(w2cur, 0, bq0);                            // group i's project MFMAs ...
                if (!halfg(gi(i))) project(w2cur, 1, bq1);
                expand_store(gi(i + 1), a4);                       // ... beside group i+1's activation and E-slice stores
                __builtin_amdgcn_sched_barrier(0);
            };
            auto tail = [&](int i, float (&w2cur)[4 * OT]) {
                dw_stage(gi(i), 0, bq0);
                project(w2cur, 0, bq0);
                if (halfg(gi(i))) return;
                dw_stage(gi(i), 1, bq1);
                project(w2cur, 1, bq1);
            };
            int i = 0;
            for (; i + 2 < ngw; i += 2) { body(i, w1a, w2a, w1b, w2b); body(i + 1, w1b, w2b, w1a, w2a); }
            if (i + 1 < ngw) { body(i, w1a, w2a, w1b, w2b); tail(i + 1, w2b); } else tail(i, w2a);
        } else {
            v4f_w a4[NSI][4];
            v2f_w bq[4];
#if IRB_TRACE
            unsigned long long tph[6] = { 0, 0, 0, 0, 0, 0 };
#define IRBW_TP(k) do { __builtin_amdgcn_sched_barrier(0); const unsigned long long tn_ = __builtin_amdgcn_s_memrealtime(); tph[k] += tn_ - tq0; tq0 = tn_; __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define IRBW_TP(k) do { } while (0)
#endif
            auto group = [&](int g, const W1T &w1, const float (&w2)[4 * OT]) {
#if IRB_TRACE
                unsigned long long tq0 = __builtin_amdgcn_s_memrealtime();
#endif
                expand_mfma(w1, a4);
                IRBW_TP(0);
                expand_store(g, a4);
                IRBW_TP(1);
                dw_stage(g, 0, bq);
                IRBW_TP(2);
                project(w2, 0, bq);
                IRBW_TP(3);
                if (halfg(g)) return;
                dw_stage(g, 1, bq);
                IRBW_TP(4);
                project(w2, 1, bq);
                IRBW_TP(5);
            };
            if (X3) {
                // X3 (register budget): ONE set of W1 operands, reloaded in place for the next group as soon as this group's expand MFMAs
                // have read it (it arrives under the depthwise / project stages); strips expanded and stored one after the other
                auto group_x3 = [&](int g, int gnext, const float (&w2)[4 * OT]) {
                    if (NSI > 2) {                                  // (four strips: one strip's accumulators alive at a time)
#pragma unroll
                        for (int si = 0; si < NSI; si++) { expand_strip(si, w1a, a4[0]); store_strip(g, si, a4[0]); }
                        __builtin_amdgcn_sched_barrier(0);
                        loadw1(gnext, w1a);
                    } else {
                        expand_mfma(w1a, a4);
                        __builtin_amdgcn_sched_barrier(0);
                        loadw1(gnext, w1a);
                        expand_store(g, a4);
                    }
                    dw_stage(g, 0, bq);
                    project(w2, 0, bq);
                    if (halfg(g)) return;
                    dw_stage(g, 1, bq);
                    project(w2, 1, bq);
                };
                for (int i = 0; i < ngw; i += 2) {
                    loadw2(gi(i + 1), w2b);
                    __builtin_amdgcn_sched_barrier(0);
                    group_x3(gi(i), gi(i + 1), w2a);
                    if (i + 1 < ngw) {
                        loadw2(gi(i + 2), w2a);
                        __builtin_amdgcn_sched_barrier(0);
                        group_x3(gi(i + 1), gi(i + 2), w2b);
                    }
                }
            } else
            for (int i = 0; i < ngw; i += 2) {                     // two groups per trip: the register sets swap roles
                // (the scheduling barriers keep the prefetch a prefetch: at the register limit the scheduler otherwise
                //  sinks these loads down to their first use, one group later, and every group waits a memory latency)
                loadw1(gi(i + 1), w1b); loadw2(gi(i + 1), w2b);
                __builtin_amdgcn_sched_barrier(0);
                group(gi(i), w1a, w2a);
                if (i + 1 < ngw) {
                    loadw1(gi(i + 2), w1a); loadw2(gi(i + 2), w2a);
                    __builtin_amdgcn_sched_barrier(0);
                    group(gi(i + 1), w1b, w2b);
                }
            }
#if IRB_TRACE
            if (p.dbg_t && threadIdx.x == 0 && blockIdx.x < 4096) for (int k = 0; k < 6; k++) p.dbg_t[blockIdx.x * 16 + 8 + k] = tph[k];
#endif
#undef IRBW_TP
        }
    }

    IRBW_T(3);
    const bool lin_out = p.act2 == 1.f && p.res_act == 1.f;       // wave-uniform
    auto row_out = [&](int t, int r, v4f_w v, v4f_w res) {
        const int o = 16 * t + 4 * kq + r, oo = min(o, p.oc - 1);
        const float sc = Sb2[2 * oo], bi = Sb2[2 * oo + 1];
        if (lin_out) {                                              // linear projection + linear shortcut (every block of yolo-fastest)
#pragma unroll
            for (int q = 0; q < 4; q++) { v[q] = fmaf(v[q], sc, bi); if (p.residual) v[q] += res[q]; }
        } else {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                v[q] = irbw_act(fmaf(v[q], sc, bi), p.act2, fl_act2);
                if (p.residual) v[q] = irbw_act(v[q] + res[q], p.res_act, fl_res);
            }
        }
        const unsigned off = ((unsigned)oo * ocs + pbase) * 4u;
        if (o < p.oc) {
            if (p.vec == 4) { if (nvalid == 4) irbw_st<v4f_w>(p.out, off, v); }
            else if (p.vec == 2) {
                if (nvalid >= 2) irbw_st<v2f_w>(p.out, off, (v2f_w){ v.x, v.y });
                if (nvalid == 4) irbw_st<v2f_w>(p.out, off + 8u, (v2f_w){ v.z, v.w });
            } else {
#pragma unroll
                for (int q = 0; q < 4; q++) if (q < nvalid) irbw_st<float>(p.out, off + 4u * q, v[q]);
            }
        }
    };

    if (p.G == 1) {
        if (RPRE) {
#pragma unroll
            for (int r = 0; r < 4; r++)
                row_out(0, r, (v4f_w){ acc[0][0][r], acc[0][1][r], acc[0][2][r], acc[0][3][r] }, rpre[r]);
            IRBW_T(5);
            return;
        }
        // the loop over rows stays rolled (its address arithmetic would otherwise be hoisted and spilled); the next
        // row's residual is in flight while the current row is finished
        v4f_w ra[OT], rb[OT];
        if (p.residual) {
#pragma unroll
            for (int t = 0; t < OT; t++) ra[t] = res_issue(t, 0);
        }
#pragma unroll 1
        for (int r = 0; r < 4; r += 2) {
            if (p.residual) {
#pragma unroll
                for (int t = 0; t < OT; t++) rb[t] = res_issue(t, r + 1);
            }
#pragma unroll
            for (int t = 0; t < OT; t++) {
                v4f_w v;
#pragma unroll
                for (int q = 0; q < 4; q++) v[q] = r == 0 ? acc[t][q].x : acc[t][q].z;
                row_out(t, r, v, ra[t]);
            }
            if (p.residual && r + 2 < 4) {
#pragma unroll
                for (int t = 0; t < OT; t++) ra[t] = res_issue(t, r + 2);
            }
#pragma unroll
            for (int t = 0; t < OT; t++) {
                v4f_w v;
#pragma unroll
                for (int q = 0; q < 4; q++) v[q] = r == 0 ? acc[t][q].y : acc[t][q].w;
                row_out(t, r + 1, v, rb[t]);
            }
        }
        IRBW_T(5);
        return;
    }

    // ---- G > 1: fixed-order reduction of the waves' partial sums through LDS (the E slices are dead by then).
    // Row pair pi = 4t + r goes to wave pi % G; its residual is fetched before the barriers.
    constexpr int RJ = 2 * OT;                                  // rows per wave: ceil(4 OT / G) <= 2 OT for G >= 2
    v4f_w rr[RJ];
    if (p.residual) {
#pragma unroll
        for (int j = 0; j < RJ; j++) {
            const int pi = min(wid + j * p.G, 4 * OT - 1);
            rr[j] = res_issue(pi >> 2, pi & 3);
        }
    }
    float *red = smem + p.cs_floats;
    auto put = [&](float *slot) {
#pragma unroll
        for (int t = 0; t < OT; t++)
#pragma unroll
            for (int r = 0; r < 4; r++)
                *reinterpret_cast<v4f_w *>(slot + (t * 4 + r) * 256 + lane * 4) = (v4f_w){ acc[t][0][r], acc[t][1][r], acc[t][2][r], acc[t][3][r] };
    };
    int nlive = p.G;
    while (nlive > p.red_cap) {                                 // fold the upper half onto the lower half
        const int h = (nlive + 1) >> 1;
        __syncthreads();
        if (wid >= h && wid < nlive) put(red + (wid - h) * (OT * 1024));
        __syncthreads();
        if (wid + h < nlive) {
            const float *slot = red + wid * (OT * 1024);
#pragma unroll
            for (int t = 0; t < OT; t++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const v4f_w v = *reinterpret_cast<const v4f_w *>(slot + (t * 4 + r) * 256 + lane * 4);
                    acc[t][0][r] += v.x; acc[t][1][r] += v.y; acc[t][2][r] += v.z; acc[t][3][r] += v.w;
                }
        }
        nlive = h;
    }
    __syncthreads();
    if (wid < nlive) put(red + wid * (OT * 1024));
    __syncthreads();
    IRBW_T(4);
#pragma unroll
    for (int j = 0; j < RJ; j++) {
        const int pi = wid + j * p.G;
        if (pi >= 4 * OT) break;                                // wave-uniform
        v4f_w v = *reinterpret_cast<const v4f_w *>(red + pi * 256 + lane * 4);
        for (int s = 1; s < nlive; s++) v += *reinterpret_cast<const v4f_w *>(red + s * (OT * 1024) + pi * 256 + lane * 4);
        row_out(pi >> 2, pi & 3, v, rr[j]);
    }
    IRBW_T(5);
#undef IRBW_T
}
