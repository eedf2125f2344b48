// ffgpu_conv_dense.inc -- dense (groups == 1) KxK convolution with few input channels: the
// network's first layer (3x3 stride 2, 3 -> 8 channels; im2row + dot in the reference,
// conv-v6.c:9-42).  One thread owns PPT output pixels and 8 output channels in registers.
// The taps sit in LDS as [tap][8 channels] so a tap costs two broadcast 16-byte LDS reads that
// serve 8 * PPT FMAs (scalar loads of 216 taps per pixel were the bottleneck of the first
// version: profiles/r01_b_layers_b64_stream_mfma.txt).  Input pixels come through L1 (each is
// reused by up to fs*fs/stride^2 neighbouring threads).  Reads the frame-major batch input or a
// CNHW tensor (general strides), writes CNHW.  Accumulation order = reference order (ci, ky, kx).
typedef float v4f_cd __attribute__((ext_vector_type(4)));

template <int FS, int PPT>
__global__ void __launch_bounds__(256) k_conv_dense8(ConvDesc d)
{
    extern __shared__ __attribute__((aligned(16))) float cd_w[];     // [K][8] taps, then [8][2] scale', bias'
    const int ob = blockIdx.y * 8;                     // first output channel of this block
    const int K = FS * FS * d.ic;
    const int k4 = (K + 3) & ~3, rl = k4 + 4;
    for (int i = threadIdx.x; i < K * 8; i += 256) {
        const int o = ob + (i & 7), tap = i >> 3;
        cd_w[i] = o < d.oc ? d.filt[(long)o * rl + tap] : 0.f;
    }
    for (int i = threadIdx.x; i < 16; i += 256) {
        const int o = ob + (i >> 1);
        cd_w[K * 8 + i] = o < d.oc ? d.filt[(long)o * rl + k4 + (i & 1)] : 0.f;
    }
    __syncthreads();
    const long npx = (long)d.N * d.oh * d.ow;
    const long span = (npx + PPT - 1) / PPT;           // thread i owns pixels i, i + span, ...
    const gfp in0 = to_global(d.in_ind ? *d.in_ind : d.in);    // executor parameter block (one graph for every input buffer)
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < span; idx += (long)gridDim.x * blockDim.x) {
        float acc[PPT][8];
        gfp src[PPT];
        int x[PPT], y[PPT];
        bool live[PPT];
#pragma unroll
        for (int p = 0; p < PPT; p++) {
            const long id = idx + p * span;
            live[p] = id < npx;
            const long ii = live[p] ? id : 0;
            x[p] = (int)(ii % d.ow);
            const long t = ii / d.ow;
            y[p] = (int)(t % d.oh);
            src[p] = in0 + (t / d.oh) * d.in_ns;
#pragma unroll
            for (int o = 0; o < 8; o++) acc[p][o] = 0.f;
        }
        for (int ci = 0; ci < d.ic; ci++) {
#pragma unroll
            for (int ky = 0; ky < FS; ky++) {
#pragma unroll
                for (int kx = 0; kx < FS; kx++) {
                    const int tap = (ci * FS + ky) * FS + kx;
                    const v4f_cd w0 = *reinterpret_cast<const v4f_cd *>(cd_w + tap * 8), w1 = *reinterpret_cast<const v4f_cd *>(cd_w + tap * 8 + 4);
#pragma unroll
                    for (int p = 0; p < PPT; p++) {
                        // unconditional load from a clamped address, zeroed afterwards: a load under a lane predicate
                        // is waited for on the spot by hipcc and the 27 taps would serialise
                        const int sy = y[p] * d.stride - d.pad + ky, sx = x[p] * d.stride - d.pad + kx;
                        const bool ok = live[p] && (unsigned)sy < (unsigned)d.ih && (unsigned)sx < (unsigned)d.iw;
                        const int cy = min(max(sy, 0), d.ih - 1), cx = min(max(sx, 0), d.iw - 1);
                        const float ld = src[p][(long)ci * d.in_cs + (long)cy * d.iw + cx];
                        const float v = ok ? ld : 0.f;
                        acc[p][0] = fmaf(v, w0.x, acc[p][0]); acc[p][1] = fmaf(v, w0.y, acc[p][1]);
                        acc[p][2] = fmaf(v, w0.z, acc[p][2]); acc[p][3] = fmaf(v, w0.w, acc[p][3]);
                        acc[p][4] = fmaf(v, w1.x, acc[p][4]); acc[p][5] = fmaf(v, w1.y, acc[p][5]);
                        acc[p][6] = fmaf(v, w1.z, acc[p][6]); acc[p][7] = fmaf(v, w1.w, acc[p][7]);
                    }
                }
            }
        }
#pragma unroll
        for (int p = 0; p < PPT; p++) {
            if (!live[p]) continue;
            const long id = idx + p * span;
            const long n = id / ((long)d.oh * d.ow);
#pragma unroll
            for (int o = 0; o < 8; o++) {
                if (ob + o >= d.oc) break;
                float v = act_apply(fmaf(acc[p][o], cd_w[K * 8 + 2 * o], cd_w[K * 8 + 2 * o + 1]), d.act);
                const long off = (long)(ob + o) * d.out_cs + n * d.out_ns + (long)y[p] * d.ow + x[p];
                if (d.residual) v = act_apply(v + d.residual[(long)(ob + o) * d.res_cs + n * d.res_ns + (long)y[p] * d.ow + x[p]], d.res_act);
                d.out[off] = v;
            }
        }
    }
}

// ---- the net's first layer in its usual form: 3x3, stride 2, pad 1, groups 1, <= 8 output channels per block, input
// width = 2 * output width, output width % 4 == 0.  One thread owns FOUR adjacent output pixels: per (channel, tap
// row) it needs input columns 8xq-1 .. 8xq+7, fetched as two aligned 16-byte loads and one scalar, all offsets in
// 32 bits; results leave as 16-byte stores; the 216 FMAs per pixel run as packed pairs.  A third of the vector-ALU
// instructions of k_conv_dense8 per pixel (one 4-byte load per tap and pixel, 64-bit index arithmetic).  Alone it is
// slower than k_conv_dense8 (55 vs 46 us: a quarter of the threads, longer dependent chains) -- with several batches in
// flight, where issue slots are what is scarce, it is the cheaper one.  Same accumulation order (ci, ky, kx).
// ST = 1 (round 4): the first layer of the other darknet cfgs (3x3, stride 1, pad 1, 3 -> 16 / 32 channels on the full input plane): input columns
// 4xq-1 .. 4xq+4 = one aligned 16-byte load and two scalars.
template <int IC, int ST = 2>
__global__ void __launch_bounds__(256) k_conv_first(ConvDesc d, unsigned m_owq)
{
    extern __shared__ __attribute__((aligned(16))) float cf_w[];     // [K][8] taps, then [8][2] scale', bias'
    const int ob = blockIdx.z * 8;
    constexpr int K = 9 * IC;
    const int k4 = (K + 3) & ~3, rl = k4 + 4;
    for (int i = threadIdx.x; i < K * 8; i += 256) {
        const int o = ob + (i & 7), tap = i >> 3;
        cf_w[i] = o < d.oc ? d.filt[o * rl + tap] : 0.f;
    }
    for (int i = threadIdx.x; i < 16; i += 256) {
        const int o = ob + (i >> 1);
        cf_w[K * 8 + i] = o < d.oc ? d.filt[o * rl + k4 + (i & 1)] : 0.f;
    }
    __syncthreads();
    const int owq = d.ow >> 2;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= d.oh * owq) return;
    const int n = blockIdx.y;
    const int oy = m_owq ? (int)__umulhi((unsigned)t, m_owq) : t, xq = t - oy * owq;
    const gfp src = to_global(d.in_ind ? *d.in_ind : d.in) + (long)n * d.in_ns;   // frame base (via the executor's parameter block); everything below is 32-bit
    v4f_cd acc[8];
#pragma unroll
    for (int o = 0; o < 8; o++) acc[o] = (v4f_cd){ 0.f, 0.f, 0.f, 0.f };
#pragma unroll
    for (int ci = 0; ci < IC; ci++) {
#pragma unroll
        for (int ky = 0; ky < 3; ky++) {
            const int sy = ST * oy - 1 + ky;
            const bool rok = (unsigned)sy < (unsigned)d.ih;
            const unsigned ro = (unsigned)ci * (unsigned)d.in_cs + (unsigned)(rok ? sy : 0) * d.iw + 4 * ST * xq;
            // unconditional loads from clamped addresses, zeroed afterwards (a load under a lane predicate is waited for
            // on the spot)
            const v4f_cd a = gld<v4f_cd>(src + ro);
            const float l = src[ro - (xq > 0 ? 1 : 0)];
            float x[9];
            x[0] = (rok && xq > 0) ? l : 0.f; x[1] = rok ? a.x : 0.f; x[2] = rok ? a.y : 0.f; x[3] = rok ? a.z : 0.f; x[4] = rok ? a.w : 0.f;
            if (ST == 2) {
                const v4f_cd b = gld<v4f_cd>(src + ro + 4);
                x[5] = rok ? b.x : 0.f; x[6] = rok ? b.y : 0.f; x[7] = rok ? b.z : 0.f; x[8] = rok ? b.w : 0.f;
            } else {
                const bool rin = 4 * xq + 4 < d.iw;
                const float r = src[ro + (rin ? 4 : 0)];
                x[5] = (rok && rin) ? r : 0.f; x[6] = x[7] = x[8] = 0.f;
            }
#pragma unroll
            for (int kx = 0; kx < 3; kx++) {
                const int tap = (ci * 3 + ky) * 3 + kx;
                const v4f_cd w0 = *reinterpret_cast<const v4f_cd *>(cf_w + tap * 8), w1 = *reinterpret_cast<const v4f_cd *>(cf_w + tap * 8 + 4);
                const v4f_cd v = { x[kx], x[ST + kx], x[2 * ST + kx], x[3 * ST + kx] };
                acc[0] += v * w0.x; acc[1] += v * w0.y; acc[2] += v * w0.z; acc[3] += v * w0.w;
                acc[4] += v * w1.x; acc[5] += v * w1.y; acc[6] += v * w1.z; acc[7] += v * w1.w;
            }
        }
    }
    const unsigned po = (unsigned)n * (unsigned)d.out_ns + (unsigned)oy * d.ow + 4 * xq;
    const float slope = d.act == 2 ? 0.1f : (d.act == 1 ? 0.f : 1.f);
#pragma unroll
    for (int o = 0; o < 8; o++) {
        if (ob + o >= d.oc) break;
        const float sc = cf_w[K * 8 + 2 * o], bi = cf_w[K * 8 + 2 * o + 1];
        // (four plain v_fma_f32 kept apart: hipcc otherwise packs them into v_pk_fma_f32 with sc / bi broadcast out of ONE register pair -- DESIGN.md 5.10, tools/isa_lint.py)
        v4f_cd v = pw_fma4_apart(acc[o].x, acc[o].y, acc[o].z, acc[o].w, sc, bi);
#pragma unroll
        for (int j = 0; j < 4; j++) v[j] = act_max(v[j], slope * v[j], act_floor(slope));
        *reinterpret_cast<v4f_cd *>(d.out + (long)(ob + o) * d.out_cs + po) = v;
    }
}
