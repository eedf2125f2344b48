// ffgpu_pw_mfma.inc -- pointwise (1x1) convolution on the fp32 matrix cores (gfx950).
//
// Restates conv-v6.c:46-91: Out[oc][p] = act(scale'[oc] * sum_ci W[oc][ci] * In[ci][p] + bias'[oc]).
// In the CNHW layout every channel is ONE contiguous run of P = N*H*W pixels, so
// the layer is the skinny GEMM  Out[oc x P] = W[oc x ic] * In[ic x P]  with a huge P.
//
//  * v_mfma_f32_16x16x4_f32 (exact fp32, k-ordered fmaf chain): A = 16 oc x 4 ic of
//    weights, B = 4 ic x 16 px.  A lane's B operand is one component of a 16-byte
//    load of 4 consecutive pixels, so each 16-lane group streams 256 contiguous
//    bytes of one input channel; the 4 components drive 4 MFMAs whose results are
//    again 4 consecutive pixels per lane -> 16-byte stores.  No LDS transpose.
//  * weights live in LDS in fragment order (one ds_read_b32 per A operand, reused
//    by the 4 MFMAs of a k-step); scale'/bias' ride along.
//  * a wave keeps OT 16-channel output tiles (OT*16 accumulator VGPRs) for a strip
//    of 64 pixels and walks strips grid-stride; blockIdx.y selects the block of
//    OT*16 output channels.  Input is read once per channel block.
//  * small pixel counts (the 10x10 / 20x20 tail of the net at modest batch): KSP = 4 makes the four
//    waves of a workgroup split the K loop of ONE strip and reduce through LDS, so the launch has
//    4x the waves and each wave 1/4 of the serial MFMA chain.
//  * optional fused residual (the shortcut that follows every linear projection in
//    yolo-fastest, ffcnn.c:418-423): out = act2(act(conv) + residual).
typedef float v4f_pw __attribute__((ext_vector_type(4)));

// activations (utils.h:15-23): linear / relu / leaky share the branch-free form max(x, slope*x); sigmoid
// (never used by a conv layer of yolo-fastest, kept for conv.h completeness) goes through ONE out-of-line
// helper so the double-precision exp is not inlined 64 times into the epilogue.
__device__ __noinline__ v4f_pw pw_sigmoid4(v4f_pw v)
{
    v4f_pw r;
    r.x = 1.0f / (1.0f + (float)exp((double)-v.x)); r.y = 1.0f / (1.0f + (float)exp((double)-v.y));
    r.z = 1.0f / (1.0f + (float)exp((double)-v.z)); r.w = 1.0f / (1.0f + (float)exp((double)-v.w));
    return r;
}
// acc * sc + bi for four accumulators of one output row, as FOUR PLAIN v_fma_f32 kept apart.  Left alone hipcc packs them into
//     v_pk_fma_f32 v[6:7], v[2:3], v[0:1], v[0:1] op_sel:[0,0,1] op_sel_hi:[1,0,1]        (scale' and bias' broadcast out of ONE register pair)
// and that instruction sporadically returns acc * sc + 0 on lanes 48-63 while a bf16 MFMA is in flight on the SIMD -- its own wave's (k_pw_x3, where it
// was found) or ANOTHER wave's, of another kernel: with the split-bf16 kernels of round 4 running in neighbouring chains, this kernel's heads' layers lost
// the bias of 16 outputs about once in 500 forwards (tools/x3s_exec_race.py; no bf16 MFMA anywhere: never).  tools/isa_lint.py (run by the library build and by tests/test_isa_lint.py) keeps the pattern out.
__device__ __forceinline__ v4f_pw pw_fma4_apart(float a0, float a1, float a2, float a3, float sc, float bi)
{
    float f0 = fmaf(a0, sc, bi), f1 = fmaf(a1, sc, bi), f2 = fmaf(a2, sc, bi), f3 = fmaf(a3, sc, bi);
    asm volatile("" : "+v"(f0)); asm volatile("" : "+v"(f1)); asm volatile("" : "+v"(f2)); asm volatile("" : "+v"(f3));
    return (v4f_pw){ f0, f1, f2, f3 };
}
__device__ __forceinline__ v4f_pw pw_act4(v4f_pw v, float slope, bool sigm)
{
    if (sigm) return pw_sigmoid4(v);                     // wave-uniform
    v4f_pw r;
    r.x = act_max(v.x, slope * v.x, act_floor(slope)); r.y = act_max(v.y, slope * v.y, act_floor(slope)); r.z = act_max(v.z, slope * v.z, act_floor(slope)); r.w = act_max(v.w, slope * v.w, act_floor(slope));
    return r;
}

struct PwP {
    const float *in; const float *filt; float *out; const float *residual;
    long  P;             // pixels per channel = N*H*W (P % 4 == 0)
    int   ic, oc, k4;    // k4 = ALIGN(ic, 4); filter row length = k4 + 4
    int   act, res_act;
    long  nstrips;       // ceil(P / 64)
    const float *wpack;  // optional: the LDS image precomputed at plan time (per output-channel block)
};

template <int OT, int KSP, int NW>
__global__ void __launch_bounds__(NW * 64) k_pw_mfma(PwP p)
{
    constexpr int NT = NW * 64;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform, and known to be
    const int oc0 = blockIdx.y * (OT * 16);
    const int ksteps = p.k4 >> 2;
    const int rl = p.k4 + 4;
    // LDS image: wl[(ks*OT + t)*64 + lane] = W[oc0 + 16 t + (lane & 15)][4 ks + (lane >> 4)]
    float *wl = smem;
    float *sb = smem + (size_t)ksteps * OT * 64;            // [OT*16][2] scale', bias'
    float *red = sb + OT * 32;                              // KSP > 1: [3 waves][OT*16][64] partial sums
    const int img = ksteps * OT * 64 + OT * 32;             // floats in the LDS image of one channel block
    if (p.wpack) {
        const v4f_pw *src = reinterpret_cast<const v4f_pw *>(p.wpack + (size_t)blockIdx.y * img);
        for (int i = tid; i < img / 4; i += NT) reinterpret_cast<v4f_pw *>(smem)[i] = src[i];
    } else {
        for (int i = tid; i < ksteps * OT * 64; i += NT) {
            const int l = i & 63, t = (i >> 6) % OT, ks = (i >> 6) / OT;
            const int o = oc0 + 16 * t + (l & 15), ci = 4 * ks + (l >> 4);
            wl[i] = (o < p.oc) ? p.filt[(long)o * rl + ci] : 0.f;   // rows are zero padded up to k4
        }
        for (int i = tid; i < OT * 16; i += NT) {
            const int o = oc0 + i;
            sb[2 * i] = o < p.oc ? p.filt[(long)o * rl + p.k4] : 0.f;
            sb[2 * i + 1] = o < p.oc ? p.filt[(long)o * rl + p.k4 + 1] : 0.f;
        }
    }
    __syncthreads();

    const float slope = p.act == 2 ? 0.1f : (p.act == 1 ? 0.f : 1.f), rslope = p.res_act == 2 ? 0.1f : (p.res_act == 1 ? 0.f : 1.f);
    const int kq = lane >> 4;                  // which of the 4 channels of a k-step this lane feeds
    const int px = (lane & 15) * 4;            // pixel offset of this lane inside the strip
    const v4f_pw z = { 0.f, 0.f, 0.f, 0.f };
    const long strip0 = KSP == 1 ? (long)blockIdx.x * NW + wid : (long)blockIdx.x;
    const long sstride = KSP == 1 ? (long)gridDim.x * NW : (long)gridDim.x;
    for (long strip = strip0; strip < p.nstrips; strip += sstride) {
        const long p0 = strip * 64 + px;
        const bool pok = p0 < p.P;             // P % 4 == 0: a lane's 4 pixels are all in or all out
        v4f_pw acc[OT][4];
#pragma unroll
        for (int t = 0; t < OT; t++)
#pragma unroll
            for (int q = 0; q < 4; q++) acc[t][q] = z;
        const int kfirst = KSP == 1 ? 0 : wid;             // KSP waves interleave the k-steps of one strip
        // This wave's k-steps are ks(i) = kfirst + i*KSP, i < nmine.  PF of their B operands are in flight ahead
        // of the MFMAs (register ring, statically indexed).  Loads are UNCONDITIONAL -- a load under a lane
        // predicate makes hipcc wait for it on the spot (s_waitcnt vmcnt(0) inside the branch), which serialises
        // the whole ring: out-of-range pixels are redirected to the strip's first quad (their columns are never
        // stored), padded channels to channel ic-1 and past-the-end prefetches re-read the last k-step.  A padded
        // channel's weights are zero, but 0 x Inf is NaN where the reference has no term at all: what a padded
        // k-slot re-read counts as ZERO: a select on the B operand, true only for the padded lanes of the last
        // k-step (tests/conv_kernels/test_gpu_kernels.py::test_non_finite_inputs[pw_mfma-*]).
#ifndef PW_MFMA_PF
#define PW_MFMA_PF 4
#endif
        constexpr int PF = PW_MFMA_PF;
        const int nmine = ksteps > kfirst ? (ksteps - kfirst + KSP - 1) / KSP : 0;
        // address = wave-uniform row pointer (k-step and strip: scalar arithmetic) + a 32-bit lane offset that never changes
        // (channel inside the k-step, pixel quad) except in the last k-step, where padded channels clamp to ic - 1;
        // eight vector instructions of 64-bit index arithmetic per load otherwise -- one per MFMA in the loop below
        const float *sbase = p.in + strip * 64;
        const unsigned lpx = pok ? (unsigned)px : 0u;
        const unsigned vo_norm = (unsigned)kq * (unsigned)p.P + lpx;
        const unsigned vo_last = (unsigned)min(kq, p.ic - 1 - 4 * (ksteps - 1)) * (unsigned)p.P + lpx;
        auto ldb = [&](int i) -> v4f_pw {
            const int ks = kfirst + min(i, nmine - 1) * KSP;
            return *reinterpret_cast<const v4f_pw *>(sbase + (long)ks * 4 * p.P + (ks == ksteps - 1 ? vo_last : vo_norm));
        };
        const bool kpad = 4 * (ksteps - 1) + kq >= p.ic;   // this lane's channel of the LAST k-step is padding (ic % 4 != 0 only)
        auto mma = [&](int i, v4f_pw bc) {
            const int ks = kfirst + i * KSP;
            bc = (kpad & (ks == ksteps - 1)) ? z : bc;     // a select, no branch: loop and tail keep their shape (and with it the ring's waits)
#pragma unroll
            for (int t = 0; t < OT; t++) {
                const float a = wl[(ks * OT + t) * 64 + lane];
                acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bc.x, acc[t][0], 0, 0, 0);
                acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bc.y, acc[t][1], 0, 0, 0);
                acc[t][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bc.z, acc[t][2], 0, 0, 0);
                acc[t][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bc.w, acc[t][3], 0, 0, 0);
            }
        };
        if (nmine > 0) {
            v4f_pw b[PF];
#pragma unroll
            for (int j = 0; j < PF; j++) b[j] = ldb(j);
            int i = 0;
            for (; i + PF <= nmine; i += PF) {               // full groups: no predicates inside
#pragma unroll
                for (int j = 0; j < PF; j++) { const v4f_pw c = b[j]; b[j] = ldb(i + PF + j); mma(i + j, c); }
            }
#pragma unroll
            for (int j = 0; j < PF - 1; j++) if (i + j < nmine) mma(i + j, b[j]);     // tail: operands are already in the ring
        }
        if (KSP > 1) {                                   // reduce the K slices of waves 1..3 into wave 0
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // LDS-only barrier: stores of the previous strip stay in flight
            __builtin_amdgcn_s_barrier();                  // (also: previous strip's reduction fully consumed)
            if (wid > 0) {
                float *dst = red + (size_t)(wid - 1) * OT * 16 * 64 + lane;
#pragma unroll
                for (int t = 0; t < OT; t++)
#pragma unroll
                    for (int q = 0; q < 4; q++)
#pragma unroll
                        for (int r = 0; r < 4; r++) dst[((t * 4 + q) * 4 + r) * 64] = acc[t][q][r];
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            if (wid == 0) {
                for (int w = 0; w < KSP - 1; w++) {
                    const float *srcr = red + (size_t)w * OT * 16 * 64 + lane;
#pragma unroll
                    for (int t = 0; t < OT; t++)
#pragma unroll
                        for (int q = 0; q < 4; q++)
#pragma unroll
                            for (int r = 0; r < 4; r++) acc[t][q][r] += srcr[((t * 4 + q) * 4 + r) * 64];
                }
            }
        }
        // D fragment: acc[t][q][r] = Out[oc0 + 16 t + 4 (lane>>4) + r][p0 + q]
        if (pok && (KSP == 1 || wid == 0)) {
#pragma unroll
            for (int t = 0; t < OT; t++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int ol = 16 * t + 4 * kq + r, o = oc0 + ol;
                    if (o < p.oc) {
                        const float sc = sb[2 * ol], bi = sb[2 * ol + 1];
                        v4f_pw v = pw_fma4_apart(acc[t][0][r], acc[t][1][r], acc[t][2][r], acc[t][3][r], sc, bi);
                        v = pw_act4(v, slope, p.act == 3);
                        const long off = (long)o * p.P + p0;
                        if (p.residual) {
                            const v4f_pw rr = *reinterpret_cast<const v4f_pw *>(p.residual + off);
                            v = pw_act4(v + rr, rslope, p.res_act == 3);
                        }
                        *reinterpret_cast<v4f_pw *>(p.out + off) = v;
                    }
                }
        }
    }
}
