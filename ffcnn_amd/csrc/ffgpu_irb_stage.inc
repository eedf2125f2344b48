// ffgpu_irb_stage.inc -- a RUN of fused inverted-residual blocks on one small plane as ONE launch, one frame per workgroup (gfx950):
//
//     B x [ 1x1 expand (48 -> 224, act1) -> depthwise 3x3 (stride 1, pad 1, actd) -> linear 1x1 project (224 -> 48) -> + the block's input ]
//
// The 10x10 stage of yolo-fastest is five such blocks.  Launched one by one (k_irbw<12,3,1,2,true,true,true>, two 10x5 tiles per frame, seven waves
// sharing a tile's fourteen groups) each block costs a workgroup's latency times the rounds its tiles take on the device, expands the halo of every
// tile a second time, and writes the 19 KB frame to memory for the next block to read back.  Here the FRAME is the tile and stays in LDS:
//   * F  [48][H x W] fp32: the block's input and shortcut, overwritten row by row with the block's output; memory sees it once, after block B - 1;
//   * XI the frame's exact three-way bf16 split (k_irbw's XL image), rebuilt from F once per block by the seven waves together;
//   * E  per wave: 8 channel pairs x a (H + 2) x P pixel plane (P = 4 ceil(W / 4) + 2) whose one-pixel ring stays zero -- the depthwise layer's
//        padding -- so the expand strips cover the H x W real pixels only, without a border select;
//   * the reduction of the seven waves' partial sums runs in OT = 3 passes of one 16-channel tile each through the (then dead) E slices, which is why
//     a wave zeroes its slice again before the next block's groups.
// Per-output arithmetic is k_irbw's XL form operation for operation -- split, K order of the
// expand MFMAs, scale' / bias' / activation, taps ascending, groups w and w + 7 on wave w, partial sums added in wave order, pw_fma4_apart for the
// rows' scale' and bias', then the shortcut -- so a net gives the same bits whether the run is merged or not (tests/irb_stage).
// Each block's constants are the packed image k_irbw_pack writes for it; the parameter block carries one pointer per block.
// ---- the pieces of a group's arithmetic, restated from the lambdas of k_irbw (ffgpu_irb_wave.inc) as functions: the two kernels place their data
// differently and compute every output with the same operations in the same order.  k_irbw keeps its own text: calling these from it moved the
// register allocation and the schedule of all 28 instantiations (listings compared), and their measured speed is what the planner's choices rest on.
// XL: one pixel's KS1 channel values (this lane's channels 4 ks + kq) -> its split image, IRBW_XL_DW dwords read back as five 16-byte windows
template <int KS1> __device__ __forceinline__ void irbw_xl_split_px(bool xinf, const float (&v)[KS1], u4_w2 (&o)[5])
{
    unsigned b[3][KS1];
    if (xinf) {
#pragma unroll
        for (int ks = 0; ks < KS1; ks++) {
            const float r = x3_resid_t<true>(v[ks]), r2 = x3_resid2(r);
            b[0][ks] = __float_as_uint(v[ks]); b[1][ks] = __float_as_uint(r); b[2][ks] = __float_as_uint(r2);
        }
    } else {
#pragma unroll
        for (int ks = 0; ks < KS1; ks++) {
            const float r = x3_resid_t<false>(v[ks]), r2 = x3_resid2(r);
            b[0][ks] = __float_as_uint(v[ks]); b[1][ks] = __float_as_uint(r); b[2][ks] = __float_as_uint(r2);
        }
    }
#pragma unroll
    for (int i = 0; i < IRBW_XL_DW; i++) {
        const int pt = i < 18 ? i / 6 : 0, pr = i < 18 ? i % 6 : i - 14;            // x0 a-f | x1 a-f | x2 a-f | x0 e f
        o[i >> 2][i & 3] = __builtin_amdgcn_perm(b[pt][2 * pr + 1], b[pt][2 * pr], 0x07060302u);
    }
}
// XL: the expand MFMAs of two pixels from their split images, the two chains interleaved
template <int NM> __device__ __forceinline__ void irbw_xl_expand2(const u4_w2 *src0, const u4_w2 *src1, const u4_w2 (&w1x)[NM], v4f_w &a0, v4f_w &a1)
{
    u4_w2 o[2][5];
#pragma unroll
    for (int i = 0; i < 5; i++) o[0][i] = src0[i];
#pragma unroll
    for (int i = 0; i < 5; i++) o[1][i] = src1[i];
#pragma unroll
    for (int m = 0; m < NM; m++) {
        const v8bf_w2 A = __builtin_bit_cast(v8bf_w2, w1x[m]);
        a0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, __builtin_bit_cast(v8bf_w2, o[0][irbw_xl_op(m)]), a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, __builtin_bit_cast(v8bf_w2, o[1][irbw_xl_op(m)]), a1, 0, 0, 0);
    }
}
// scale', bias' and activation of one channel pair of an expanded pixel
__device__ __forceinline__ v2f_w irbw_expand_act(v2f_w a, v2f_w sc, v2f_w bi, float act1, float fl_act1)
{
    const v2f_w t = a * sc + bi;
    const v2f_w u = t * act1;
    return (v2f_w){ act_max(t.x, u.x, fl_act1), act_max(t.y, u.y, fl_act1) };
}
// the depthwise constants of one channel pair: [tap 0..8, scale', bias'][2 channels]
struct IrbwTaps { v2f_w tap[9], sd, bd; };
__device__ __forceinline__ void irbw_dw_taps(const float *wdp, IrbwTaps &k)
{
    v4f_w T[6];
#pragma unroll
    for (int i = 0; i < 6; i++) T[i] = *reinterpret_cast<const v4f_w *>(wdp + 4 * i);
    k.tap[0] = (v2f_w){ T[0].x, T[0].y }; k.tap[1] = (v2f_w){ T[0].z, T[0].w }; k.tap[2] = (v2f_w){ T[1].x, T[1].y };
    k.tap[3] = (v2f_w){ T[1].z, T[1].w }; k.tap[4] = (v2f_w){ T[2].x, T[2].y }; k.tap[5] = (v2f_w){ T[2].z, T[2].w };
    k.tap[6] = (v2f_w){ T[3].x, T[3].y }; k.tap[7] = (v2f_w){ T[3].z, T[3].w }; k.tap[8] = (v2f_w){ T[4].x, T[4].y };
    k.sd = (v2f_w){ T[4].z, T[4].w }; k.bd = (v2f_w){ T[5].x, T[5].y };
}
// window row r of a quad's four outputs (x: the row's pixels from the quad's first window column on), taps ascending
template <int S> __device__ __forceinline__ void irbw_dw_row(const IrbwTaps &k, int r, const v2f_w *x, v2f_w (&dv)[4])
{
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int kx = 0; kx < 3; kx++) dv[q] += k.tap[r * 3 + kx] * x[S * q + kx];
}
__device__ __forceinline__ void irbw_dw_out(const IrbwTaps &k, const v2f_w (&dv)[4], float actd, float fl_actd, v2f_w (&bq)[4])
{
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const v2f_w t = dv[q] * k.sd + k.bd;
        const v2f_w u = t * actd;
        bq[q] = (v2f_w){ act_max(t.x, u.x, fl_actd), act_max(t.y, u.y, fl_actd) };
    }
}
// the project MFMAs of one depthwise stage (channel pair m of every lane group: k-steps 2m and 2m+1)
template <int OT> __device__ __forceinline__ void irbw_project(v4f_w (&acc)[OT][4], const float (&w2)[4 * OT], int m, const v2f_w (&bq)[4])
{
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
}

#define IRBS_WAVES 7
struct IrbStageP {
    const float *in; float *out;
    const float *pk[IRBS_MAXB];      // the blocks' packed images (irbw layout: x3, 14 groups, OT = 3)
    int B, N, H, W;
    float act1, actd;                // slopes, the same in every block of the run; project and shortcut are linear
    int TWq, P, EP;                  // quads per plane row; E row pitch and pixels per channel-pair plane (P x (H + 2)), both even
    int o_w2, o_cs, cs_floats;       // float offsets in a packed image, floats of the shared constants
    int e_off, e_slice, xi_off, f_off;   // float offsets in LDS
    unsigned m_w, m_twq, m_plane;    // ceil(2^32 / W), and the same for TWq and H x W (0: divisor 1)
};

__global__ void __launch_bounds__(IRBS_WAVES * 64, 2) k_irb_stage(IrbStageP p)
{
    constexpr int KS1 = 12, OT = 3, NM = irbw_x3_nm(KS1), G = IRBS_WAVES;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    int lane = tid & 63, kq = lane >> 4, jq = lane & 15;
    const int n = (int)blockIdx.x, plane = p.H * p.W, nstrips = (plane + 63) >> 6;
    const float fl_act1 = act_floor(p.act1), fl_actd = act_floor(p.actd);
    const int ecp = 14 * 16;
    const float *Wd = smem, *Sb1 = smem + ecp * 12, *Sb2 = Sb1 + ecp * 2;
    float *Ew = smem + p.e_off + wid * p.e_slice;
    unsigned *XI = reinterpret_cast<unsigned *>(smem) + p.xi_off;
    float *F = smem + p.f_off;
    const v4f_w z = { 0.f, 0.f, 0.f, 0.f };
    const int cs4 = p.cs_floats >> 2;                            // <= 2 x 448 sixteen-byte pieces (checked at launch)

    // ---- the frame -> F; block 0's constants -> LDS
    for (int i = tid; i < 48 * plane; i += G * 64) {
        const int c = irbw_div(i, p.m_plane), px = i - c * plane;
        F[i] = p.in[((long)c * p.N + n) * plane + px];
    }
    for (int i = tid; i < cs4; i += G * 64) reinterpret_cast<v4f_w *>(smem)[i] = irbw_ld<v4f_w>(p.pk[0], (unsigned)(p.o_cs + 4 * i) * 4u);

    int ebase[2], fbase[2], nvalid[2];
    const bool strip1 = p.TWq * p.H > 16;                        // uniform: the plane has more than 16 quads

    struct W1T { u4_w2 x[NM]; };
    W1T w1a;
    float w2[4 * OT];
    auto loadw1 = [&](const float *pk, int g) {
#pragma unroll
        for (int m = 0; m < NM; m++) w1a.x[m] = irbw_ld<u4_w2>(pk, (unsigned)((g * NM + m) * 64 + lane) * 16u);
    };
    auto loadw2 = [&](const float *pk, int g, float (&w)[4 * OT]) {
#pragma unroll
        for (int i = 0; i < 4 * OT; i++) w[i] = irbw_ld<float>(pk, (unsigned)(p.o_w2 + (g * 4 * OT + i) * 64 + lane) * 4u);
    };
    loadw1(p.pk[0], wid);

    v4f_w acc[2][OT][4];
    // one group of 16 expanded channels over the whole frame: expand strips -> E (real pixels only) -> per output strip depthwise + project
    auto group = [&](const float *pk, int g, int gnext) {
        loadw2(pk, g, w2);                                       // (for the project MFMAs: arrives under the expand strips)
        __builtin_amdgcn_sched_barrier(0);
        const float *sbp = Sb1 + (g * 4 + kq) * 8;
        const v4f_w S4 = *reinterpret_cast<const v4f_w *>(sbp), B4 = *reinterpret_cast<const v4f_w *>(sbp + 4);
        const v2f_w sc[2] = { { S4.x, S4.y }, { S4.z, S4.w } }, bi[2] = { { B4.x, B4.y }, { B4.z, B4.w } };
#pragma unroll
        for (int si = 0; si < 2; si++) {                         // one strip's accumulators alive at a time
            if (si >= nstrips) break;
            v4f_w a4[4] = { z, z, z, z };
#pragma unroll
            for (int qh = 0; qh < 2; qh++) {
                const u4_w2 *src = reinterpret_cast<const u4_w2 *>(XI + ((si * 4 + 2 * qh) * 64 + lane) * IRBW_XL_DW);
                irbw_xl_expand2<NM>(src, src + 64 * IRBW_XL_DW / 4, w1a.x, a4[2 * qh], a4[2 * qh + 1]);
            }
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int e = si * 64 + 4 * jq + q;
                const int y = irbw_div(e, p.m_w), x = e - y * p.W;
                if (e < plane) {                                 // a lane whose slot lies past the plane stores nothing
                    float *dst = Ew + ((y + 1) * p.P + x + 1) * 2;
#pragma unroll
                    for (int rp = 0; rp < 2; rp++) {
                        const v2f_w a = rp == 0 ? (v2f_w){ a4[q].x, a4[q].y } : (v2f_w){ a4[q].z, a4[q].w };
                        *reinterpret_cast<v2f_w *>(dst + (2 * kq + rp) * p.EP * 2) = irbw_expand_act(a, sc[rp], bi[rp], p.act1, fl_act1);
                    }
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (gnext >= 0) loadw1(pk, gnext);                       // the next group's W1 arrives under the depthwise / project stages
#pragma unroll
        for (int m = 0; m < 2; m++) {
            const int pr = 2 * kq + m;
            IrbwTaps k;
            irbw_dw_taps(Wd + (g * 8 + pr) * 24, k);
#pragma unroll
            for (int so = 0; so < 2; so++) {
                if (so == 1 && !strip1) break;
                const float *ep = Ew + pr * p.EP * 2 + ebase[so];
                v2f_w dv[4] = { { 0.f, 0.f }, { 0.f, 0.f }, { 0.f, 0.f }, { 0.f, 0.f } }, bq[4];
#pragma unroll
                for (int r = 0; r < 3; r++) {
                    const float *row = ep + r * p.P * 2;
                    v2f_w x[6];
#pragma unroll
                    for (int i = 0; i < 3; i++) {
                        const v4f_w u = *reinterpret_cast<const v4f_w *>(row + 4 * i);
                        x[2 * i] = (v2f_w){ u.x, u.y }; x[2 * i + 1] = (v2f_w){ u.z, u.w };
                    }
                    irbw_dw_row<1>(k, r, x, dv);
                }
                irbw_dw_out(k, dv, p.actd, fl_actd, bq);
                irbw_project<OT>(acc[so], w2, m, bq);
            }
        }
    };

    for (int b = 0; b < p.B; b++) {
        const float *pk = p.pk[b];
        // ---- this wave's E slice zeroed (the ring; the reduction of the block before ran through it), the frame's split image from F
        for (int i = lane; i < (p.e_slice >> 2); i += 64) reinterpret_cast<v4f_w *>(Ew)[i] = z;
        // an opaque zero (the ring's corner): everything a lane derives from its number is recomputed per block.  Hoisted out of the block loop that
        // arithmetic held 65 registers and spilled into the group loop
        lane = (tid & 63) + __float_as_int(Ew[0]); kq = lane >> 4; jq = lane & 15;
        // ---- this lane's two output quads (strip so: quad 16 so + jq of the plane's TWq x H) and their places in E and F
#pragma unroll
        for (int so = 0; so < 2; so++) {
            const int j = so * 16 + jq, ty = irbw_div(j, p.m_twq), tq = j - ty * p.TWq;
            const bool qv = ty < p.H;
            ebase[so] = qv ? (ty * p.P + 4 * tq) * 2 : 0;           // window start in a pair plane, floats (even pixel: 16-byte aligned)
            fbase[so] = qv ? ty * p.W + 4 * tq : 0;
            nvalid[so] = qv ? min(4, p.W - 4 * tq) : 0;
        }
        if (b == 0) __syncthreads();                             // F and the constants visible (later blocks: the barrier behind the rows)
        for (int item = wid; item < nstrips * 4; item += G) {    // item = (strip, pixel of the lane's quad)
            const int si = item >> 2, q = item & 3, e = si * 64 + 4 * jq + q;
            float v[KS1];
#pragma unroll
            for (int ks = 0; ks < KS1; ks++) v[ks] = e < plane ? F[(4 * ks + kq) * plane + e] : 0.f;
            float amax = 0.f;
#pragma unroll
            for (int ks = 0; ks < KS1; ks += 2) amax = x3_amax3(amax, v[ks], v[ks + 1]);
            const bool xinf = X3_INF_X_FUSED && x3_wave_has_inf(amax);                  // wave-uniform
            u4_w2 o[5];
            irbw_xl_split_px<KS1>(xinf, v, o);
            u4_w2 *dst = reinterpret_cast<u4_w2 *>(XI + (item * 64 + lane) * IRBW_XL_DW);
#pragma unroll
            for (int i = 0; i < 5; i++) dst[i] = o[i];
        }
#pragma unroll
        for (int so = 0; so < 2; so++)
#pragma unroll
            for (int t = 0; t < OT; t++)
#pragma unroll
                for (int q = 0; q < 4; q++) acc[so][t][q] = z;
        __syncthreads();                                         // the split image complete

        // ---- groups wid and wid + 7 (k_irbw at G = 7: gfirst = wid, gstep = 7)
        group(pk, wid, wid + G);
        group(pk, wid + G, -1);
        __builtin_amdgcn_sched_barrier(0);

        // the next block's constants and first weights are fetched underneath the reduction
        const bool more = b + 1 < p.B;
        const float *pkn = p.pk[more ? b + 1 : b];
        v4f_w cst[2];
#pragma unroll
        for (int u = 0; u < 2; u++) cst[u] = irbw_ld<v4f_w>(pkn, (unsigned)(p.o_cs + 4 * min(tid + u * G * 64, cs4 - 1)) * 4u);
        loadw1(pkn, wid);

        // ---- reduction, one 16-channel tile per pass: every wave parks its partial sums of the tile in its own E slice, [strip][register r][lane] x 4
        // pixels; row (so, r) is then summed in wave order by wave (4 so + r) % 7 and finished: scale', bias', + the shortcut from F, back into F -- or,
        // in the last block, out to memory
#pragma unroll
        for (int t = 0; t < OT; t++) {
            if (t > 0) __syncthreads();                          // the rows of the pass before have read this slice
#pragma unroll
            for (int so = 0; so < 2; so++)
#pragma unroll
                for (int r = 0; r < 4; r++)
                    *reinterpret_cast<v4f_w *>(Ew + ((so * 4 + r) * 64 + lane) * 4) = (v4f_w){ acc[so][t][0][r], acc[so][t][1][r], acc[so][t][2][r], acc[so][t][3][r] };
            __syncthreads();
            for (int row = wid; row < 8; row += G) {
                const int so = row >> 2, r = row & 3;
                if (so == 1 && !strip1) break;
                const float *red = smem + p.e_off + (row * 64 + lane) * 4;
                v4f_w v = *reinterpret_cast<const v4f_w *>(red);
                for (int s = 1; s < G; s++) v += *reinterpret_cast<const v4f_w *>(red + s * p.e_slice);
                const int o = 16 * t + 4 * kq + r;
                v = pw_fma4_apart(v.x, v.y, v.z, v.w, Sb2[2 * o], Sb2[2 * o + 1]);
                const int nv = so ? nvalid[1] : nvalid[0];
                float *fp = F + o * plane + (so ? fbase[1] : fbase[0]);
                float *gp = p.out + ((long)o * p.N + n) * plane + (so ? fbase[1] : fbase[0]);
                if ((p.W & 3) == 0) {
                    if (nv == 4) {
                        v += *reinterpret_cast<const v4f_w *>(fp);
                        if (more) *reinterpret_cast<v4f_w *>(fp) = v; else *reinterpret_cast<v4f_w *>(gp) = v;
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < 4; q++)
                        if (q < nv) { const float w = v[q] + fp[q]; if (more) fp[q] = w; else gp[q] = w; }
                }
            }
        }
        if (!more) break;
        __syncthreads();                                         // F complete; slices and constants free
#pragma unroll
        for (int u = 0; u < 2; u++) if (tid + u * G * 64 < cs4) reinterpret_cast<v4f_w *>(smem)[tid + u * G * 64] = cst[u];
    }
}
