// ffgpu_pw_bf16.inc -- OPT-IN reduced-precision form of the compute-bound pointwise convolution (FFGPU_BF16_PW): inputs and
// weights rounded to bf16 (round to nearest even), products accumulated in fp32 on v_mfma_f32_32x32x16_bf16.  NEVER the
// default: the reference is fp32 end to end (conv-v6.c:46-91) and the parity bar of this repo is fp32.  The north star
// allows "MFMA bf16/fp32 GEMM where the channel count makes it a dense contraction"; on BASELINE config[2] (256 -> 512
// channels, 20x20, batch 256) the bf16 matrix rate is 16x the fp32 one, so the layer flips from MFMA-bound (floor 171 us)
// to HBM-bound (315 MB: floor 39 us at 8 TB/s).  Its own tolerance: per output |d| <= 2^-7 * scale' * sum_k |w_k x_k|
// (two roundings of relative size 2^-9 per product, worst case; tests/test_gpu_kernels.py::test_pw_bf16).
//
// Same tiling as ffgpu_pw_gemm32.inc: workgroup tile 128 channels x 128 pixels, 4 waves (2 x 2), wave tile 64 x 64 = 2 x 2
// accumulators of 32 x 32 (the C/D map does not depend on the input type); K in chunks of 32 = two MFMA k-steps of 16.
//   A (weights): plan-time bf16 image that is the LDS chunk image: [k-step][wave row][row block][lane][8 bf16] -- a lane's
//     operand (row lane & 31, k = 8 (lane >> 5) .. + 7) is one ds_read_b128.
//   B (input):   fp32 channel rows from global memory (16-byte loads, 512 contiguous bytes per row), converted with
//     v_cvt_pk_bf16_f32 and written TRANSPOSED to LDS as [pixel][k] (pitch 80 bytes): a lane's operand (pixel column, 8
//     consecutive k) is again one ds_read_b128.  Register-staged, two LDS buffers, one barrier per chunk.
//   The two pixel blocks of a wave are pixels 2n, 2n + 1 (as in the fp32 kernel): 8-byte stores, no transpose in the epilogue.
typedef __bf16 v8bf_pb __attribute__((ext_vector_type(8)));
typedef __bf16 v2bf_pb __attribute__((ext_vector_type(2)));

struct PwBf16P {
    const float *in; float *out; const float *residual;
    const unsigned *wpack;       // bf16 image (as dwords) + fp32 scale' / bias'
    long P, ntn;
    int  ic, oc, nchunks, ntm;   // nchunks = ceil(ic / 32), ntm = channel tiles of 128
    int  img;                    // dwords per channel tile: nchunks * 2048 + 256
    int  act, res_act, per_xcd;
};

constexpr int PWB_KC = 32;

// per channel tile mt, per chunk c: dword index ((((ks * 2 + wm) * 2 + r) * 64 + lane) * 4 + q) holds bf16 pair
// W[128 mt + 64 wm + 32 r + (lane & 31)][32 c + 16 ks + 8 (lane >> 5) + 2 q + (0, 1)]; then [128][2] fp32 scale', bias'
struct PwBf16PackP { const float *filt; unsigned *pk; int ic, oc, k4, nchunks, ntm; };
__global__ void k_pw_bf16_pack(PwBf16PackP p)
{
    const int img = p.nchunks * 2048 + 256, total = img * p.ntm, rl = p.k4 + 4;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int mt = i / img, j = i - mt * img;
        unsigned v = 0;
        if (j < p.nchunks * 2048) {
            const int c = j >> 11, e = j & 2047;
            const int q = e & 3, l = (e >> 2) & 63, r = (e >> 8) & 1, wm = (e >> 9) & 1, ks = e >> 10;
            const int o = 128 * mt + 64 * wm + 32 * r + (l & 31), k = PWB_KC * c + 16 * ks + 8 * (l >> 5) + 2 * q;
            const float w0 = (o < p.oc && k < p.ic) ? p.filt[(long)o * rl + k] : 0.f, w1 = (o < p.oc && k + 1 < p.ic) ? p.filt[(long)o * rl + k + 1] : 0.f;
            const v2bf_pb b = { (__bf16)w0, (__bf16)w1 };
            v = __builtin_bit_cast(unsigned, b);
        } else {
            const int t = j - p.nchunks * 2048, o = 128 * mt + (t >> 1);
            const float f = o < p.oc ? p.filt[(long)o * rl + p.k4 + (t & 1)] : 0.f;
            v = __builtin_bit_cast(unsigned, f);
        }
        p.pk[i] = v;
    }
}

__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) k_pw_bf16(PwBf16P p)
{
    constexpr int TN = 128, ACH = 2048, BPITCH = 20, BCH = TN * BPITCH;   // dwords: A chunk; B row pitch (80 bytes) and chunk
    typedef float v4 __attribute__((ext_vector_type(4)));
    typedef float v2 __attribute__((ext_vector_type(2)));
    typedef float v16 __attribute__((ext_vector_type(16)));
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    typedef unsigned u2 __attribute__((ext_vector_type(2)));
    __shared__ __attribute__((aligned(16))) unsigned smem[2 * ACH + 2 * BCH + 256];
    unsigned (*sA)[ACH] = reinterpret_cast<unsigned (*)[ACH]>(smem);
    unsigned (*sB)[BCH] = reinterpret_cast<unsigned (*)[BCH]>(smem + 2 * ACH);
    float *sSB = reinterpret_cast<float *>(smem + 2 * ACH + 2 * BCH);

    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wid >> 1, wn = wid & 1;
    const long total = (long)p.ntm * p.ntn;
    const long tile = (long)(blockIdx.x & 7) * p.per_xcd + (blockIdx.x >> 3);          // XCD-aware order (see ffgpu_pw_gemm32.inc)
    if ((int)(blockIdx.x >> 3) >= p.per_xcd || tile >= total) return;
    const int mt = (int)(tile % p.ntm);
    const long p0 = (tile / p.ntm) * TN;
    const unsigned *wimg = p.wpack + (size_t)mt * p.img;
    sSB[tid] = __builtin_bit_cast(float, wimg[p.nchunks * 2048 + tid]);

    // staging: thread = (4 pixels, 4 channels) of the chunk: 4 loads of 16 bytes, 8 conversions, 4 ds_write_b64 ([pixel][k])
    const int pxg = tid & 31, kg = tid >> 5;
    long px = p0 + 4 * pxg;
    if (px > p.P - 4) px = p.P - 4;                                   // ragged last tile: clamped (its results are not stored)
    const float *bsrc = p.in + px;
    u4 ra[2];
    v4 rb[4];
    auto gload = [&](int c) {
        ra[0] = reinterpret_cast<const u4 *>(wimg + (size_t)c * ACH)[tid];
        ra[1] = reinterpret_cast<const u4 *>(wimg + (size_t)c * ACH)[tid + 256];
#pragma unroll
        for (int j = 0; j < 4; j++)        // channels beyond ic: the last valid row, zeroed in lstore
            rb[j] = *reinterpret_cast<const v4 *>(bsrc + (long)min(PWB_KC * c + 4 * kg + j, p.ic - 1) * p.P);
    };
    // c: the chunk in the registers.  Channels beyond ic (the last chunk of a ragged ic) count as ZERO: their weights are zero in the image, but a re-read
    // row would give 0 x Inf = NaN where the reference has no term (tests/conv_kernels/test_gpu_kernels.py::test_non_finite_inputs[pw_bf16-*])
    const bool kragged = (p.ic & (PWB_KC - 1)) != 0;                  // uniform
    auto lstore = [&](int buf, int c) {
        reinterpret_cast<u4 *>(sA[buf])[tid] = ra[0];
        reinterpret_cast<u4 *>(sA[buf])[tid + 256] = ra[1];
        if (kragged && c == p.nchunks - 1) {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (PWB_KC * c + 4 * kg + j >= p.ic) rb[j] = (v4){ 0.f, 0.f, 0.f, 0.f };
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {                                 // pixel 4 pxg + i: k = 4 kg .. 4 kg + 3 -> two dwords
            const v2bf_pb lo = { (__bf16)rb[0][i], (__bf16)rb[1][i] }, hi = { (__bf16)rb[2][i], (__bf16)rb[3][i] };
            *reinterpret_cast<u2 *>(&sB[buf][(4 * pxg + i) * BPITCH + 2 * kg]) = (u2){ __builtin_bit_cast(unsigned, lo), __builtin_bit_cast(unsigned, hi) };
        }
    };

    v16 acc[2][2];
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[r][j][e] = 0.f;

    gload(0);
    lstore(0, 0);
    __syncthreads();
    for (int c = 0; c < p.nchunks; c++) {
        const int buf = c & 1;
        if (c + 1 < p.nchunks) gload(c + 1);
#pragma unroll
        for (int ks = 0; ks < 2; ks++) {
            v8bf_pb fa[2], fb[2];
#pragma unroll
            for (int r = 0; r < 2; r++)
                fa[r] = __builtin_bit_cast(v8bf_pb, *reinterpret_cast<const u4 *>(&sA[buf][(((ks * 2 + wm) * 2 + r) * 64 + lane) * 4]));
#pragma unroll
            for (int j = 0; j < 2; j++)                               // pixel 2 (lane & 31) + j of the wave's 64, k = 16 ks + 8 (lane >> 5) ..
                fb[j] = __builtin_bit_cast(v8bf_pb, *reinterpret_cast<const u4 *>(&sB[buf][(wn * 64 + 2 * (lane & 31) + j) * BPITCH + 8 * ks + 4 * (lane >> 5)]));
#pragma unroll
            for (int r = 0; r < 2; r++)
#pragma unroll
                for (int j = 0; j < 2; j++)
                    acc[r][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[r], fb[j], acc[r][j], 0, 0, 0);
        }
        if (c + 1 < p.nchunks) lstore(buf ^ 1, c + 1);
        __syncthreads();
    }

    // epilogue (fp32): as ffgpu_pw_gemm32.inc -- row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5), pixels 2 (lane & 31) + (0, 1)
    const float slope = p.act == 2 ? 0.1f : (p.act == 1 ? 0.f : 1.f), rslope = p.res_act == 2 ? 0.1f : (p.res_act == 1 ? 0.f : 1.f);
    const long pxo = p0 + wn * 64 + 2 * (lane & 31);
    if (pxo >= p.P) return;
    auto act1 = [&](float t, int a, float sl) { return a == 3 ? 1.0f / (1.0f + (float)exp((double)-t)) : act_max(t, sl * t, act_floor(sl)); };
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const int ol = 64 * wm + 32 * r + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5), o = 128 * mt + ol;
            if (o >= p.oc) continue;
            const float sc = sSB[2 * ol], bi = sSB[2 * ol + 1];
            v2 v = { act1(fmaf(acc[r][0][e], sc, bi), p.act, slope), act1(fmaf(acc[r][1][e], sc, bi), p.act, slope) };
            const long off = (long)o * p.P + pxo;
            if (p.residual) {
                const v2 q = *reinterpret_cast<const v2 *>(p.residual + off);
                v = (v2){ act1(v.x + q.x, p.res_act, rslope), act1(v.y + q.y, p.res_act, rslope) };
            }
            *reinterpret_cast<v2 *>(p.out + off) = v;
        }
}
