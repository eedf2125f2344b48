// ffgpu_irb_wave2.inc -- the wave-autonomous fused block (ffgpu_irb_wave.inc) with TWO output strips per wave, for
// stride-1 blocks with at most 16 output channels on planes that are big enough (40x40 and up, one wave per tile).
//
// A 64-pixel output tile needs a 128-pixel halo tile: every expanded value is computed twice over.  A tile of up to
// 32 quads (20x6, 12x10, ...: TWq * ceil(TH / 2) <= 16) shares one halo of THREE strips (24x8 = 192 pixels for 20x6): 1.6 expanded pixels per
// output pixel instead of 2.1, i.e. a fifth less expand MFMA work, activation / store VALU work and per-tile
// overhead per output -- which is what bounds these launches (DESIGN.md section 5.4: the pipes' times add up).
// Same arithmetic, packed weight image and LDS constant table as k_irbw (conv-v6.c:46-91, 96-229, 46-91 and
// ffcnn.c:418-423); no group split, no pipelined form (those stay in k_irbw).
// X3: the expand GEMM as split-bf16 products on v_mfma_f32_16x16x32_bf16 (see ffgpu_irb_wave.inc "X3"): same results as the fp32
// form to within a summation order, 3 / 2 matrix instructions of ~17 cycles per (strip, pixel) instead of 4 / 2 of 32.
#ifndef IRBW2_X3_KS2_MINB
#define IRBW2_X3_KS2_MINB 2
#endif
template <int KS1, int NSI, bool X3>
__global__ void __launch_bounds__(256, (X3 && KS1 == 2) ? IRBW2_X3_KS2_MINB : 2) k_irbw2(IrbwP p)
{
    constexpr int NM = X3 ? irbw_x3_nm(KS1) : 1;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kq = lane >> 4, jq = lane & 15;
    // the relu floors (act_floor), once and outside every lane condition: the scalar read is a convergent operation, and under a lane condition hipcc branches around it
    const float fl_act1 = act_floor(p.act1), fl_actd = act_floor(p.actd), fl_act2 = act_floor(p.act2), fl_res = act_floor(p.res_act);
    constexpr int NPw = NSI * 64, NQ = NSI * 16, NSO = 2;
    const int ecp = p.ngroups * 16;
    const float *Wd = smem, *Sb1 = smem + ecp * 12, *Sb2 = Sb1 + ecp * 2;
    float *Ew = smem + p.cs_floats + wid * (16 * NPw);
    const v4f_w z = { 0.f, 0.f, 0.f, 0.f };

    const int cs4 = p.cs_floats >> 2, nthr = (int)blockDim.x;
    v4f_w cst[3];
#pragma unroll
    for (int u = 0; u < 3; u++) cst[u] = irbw_ld<v4f_w>(p.pk, (unsigned)(p.o_cs + 4 * min(tid + u * nthr, cs4 - 1)) * 4u);

    const int tile = (p.xcd ? irbw_xcd_block((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x) * p.WPB + wid;
    const bool active = tile < (int)p.ntiles;                  // wave-uniform
    const int tt = active ? tile : 0;
    const int trow = irbw_div(tt, p.m_tx), tx_i = tt - trow * p.tiles_x;
    const int n = irbw_div(trow, p.m_ty), ty_i = trow - n * p.tiles_y;
    const int oy0 = ty_i * p.TH, ox0 = tx_i * p.TWq * 4;
    const int gy0 = oy0 - 1, gx0 = ox0 - 1;                     // image coordinates of halo-tile element (0,0)
    const bool interior = gy0 >= 0 && gx0 >= 0 && gy0 + p.EH <= p.H && gx0 + p.EW <= p.W;

    // ---- input halo tile -> registers (B operands of the expand MFMAs); validity bits of its pixels
    v4f_w xin[NSI][KS1];
    unsigned mbits = 0;
    {
        const int plane = p.H * p.W;
        bool anyfix = false;
#pragma unroll
        for (int si = 0; si < NSI; si++) {
            const int e = si * 64 + 4 * jq;
            const int iy = (int)__umulhi((unsigned)e, p.m_ew), ix = e - iy * p.EW;
            const int gy = gy0 + iy, gx = gx0 + ix;
            if (!interior) {
                const bool rowok = (iy < p.EH) & ((unsigned)gy < (unsigned)p.H);
#pragma unroll
                for (int q = 0; q < 4; q++) mbits |= (rowok & ((unsigned)(gx + q) < (unsigned)p.W)) ? 1u << (si * 4 + q) : 0u;
            }
            const int rowidx = (n * p.H + min(max(gy, 0), p.H - 1)) * p.W + gx;
#pragma unroll
            for (int ks = 0; ks < KS1; ks++) {
                const int idx = min(4 * ks + kq, p.ic - 1) * (p.N * plane) + rowidx;
                const int cl = min(max(idx, 0), (int)p.in_elems - 4);
                anyfix |= cl != idx;
                xin[si][ks] = irbw_ld<v4f_w>(p.in, (unsigned)cl * 4u);
            }
        }
        if (anyfix) {                                           // see k_irbw: the two ends of the whole tensor
#pragma unroll
            for (int si = 0; si < NSI; si++) {
                const int e = si * 64 + 4 * jq;
                const int iy = (int)__umulhi((unsigned)e, p.m_ew), ix = e - iy * p.EW;
                const int rowidx = (n * p.H + min(max(gy0 + iy, 0), p.H - 1)) * p.W + gx0 + ix;
#pragma unroll
                for (int ks = 0; ks < KS1; ks++) {
                    const int idx = min(4 * ks + kq, p.ic - 1) * (p.N * plane) + rowidx;
                    const int d = min(max(idx, 0), (int)p.in_elems - 4) - idx;
                    if (d != 0) {
                        const v4f_w l = xin[si][ks];
                        v4f_w w = z;
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            const int s = q - d;
                            w[q] = s == 0 ? l.x : (s == 1 ? l.y : (s == 2 ? l.z : (s == 3 ? l.w : 0.f)));
                        }
                        xin[si][ks] = w;
                    }
                }
            }
        }
    }
    if (4 * (KS1 - 1) + kq >= p.ic) {                           // see k_irbw: padded input channels count as zero (0 * Inf)
#pragma unroll
        for (int si = 0; si < NSI; si++) xin[si][KS1 - 1] = z;
    }
    // X3: the tile's exact three-way split, packed as bf16 pairs of the lane's channels (2 pr, 2 pr + 1): xp[strip][pixel][part][pair]
    unsigned xp[X3 ? NSI : 1][4][3][X3 ? KS1 / 2 : 1];
    if (X3) {
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
                    for (int ks = 0; ks < KS1; ks++) {
                        const float x = xin[si][ks][q];
                        const float r = x3_resid_t<decltype(INF)::value>(x);                      // exact (INF: 0 for +-Inf)
                        const float r2 = x3_resid2(r);                                                      // exact, <= 8 significant bits
                        b[0][ks] = __float_as_uint(x); b[1][ks] = __float_as_uint(r); b[2][ks] = __float_as_uint(r2);   // (the parts are the upper halves)
                    }
#pragma unroll
                    for (int pt = 0; pt < 3; pt++)
#pragma unroll
                        for (int pr = 0; pr < KS1 / 2; pr++) xp[si][q][pt][pr] = __builtin_amdgcn_perm(b[pt][2 * pr + 1], b[pt][2 * pr], 0x07060302u);
                }
        };
        if (X3_INF_X_FUSED && x3_wave_has_inf(amax)) split_tile(std::true_type{}); else split_tile(std::false_type{});      // (wave-uniform: ffgpu_irb_wave.inc, x3_resid_t)
    }
    auto bop = [&](int si, int q, int m) -> v8bf_w2 {               // B operand of MFMA m: 8 K slots of this lane's pixel column
        u4_w2 u;
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const IrbwX3Term t = irbw_x3_term(KS1, m, d);
            u[d] = t.wp < 0 ? 0u : xp[X3 ? si : 0][q][t.xp][X3 ? t.pair : 0];
        }
        return __builtin_bit_cast(v8bf_w2, u);
    };
    // this lane's two output quads: the SAME columns in two adjacent rows (rows 2 jq / TWq and + 1, TWq * ceil(TH / 2)
    // <= 16), so their 3x3 windows share two of their three E rows -- four row reads for two quads instead of six (the
    // fused blocks are as short of LDS bandwidth as of issue slots) -- and where the upper window starts
    int ebase[NSO], nvalid[NSO];
    unsigned pbase[NSO];
    const int typ = irbw_div(jq, p.m_twq), tq = jq - typ * p.TWq;
#pragma unroll
    for (int so = 0; so < NSO; so++) {
        const int ty = 2 * typ + so;
        const bool qvalid = ty < p.TH;
        ebase[so] = qvalid ? ty * p.EW + tq * 4 : 0;
        const int oy = oy0 + ty, ox = ox0 + tq * 4;
        const bool valid = active && qvalid && oy < p.OH && ox < p.OW;
        nvalid[so] = valid ? min(4, p.OW - ox) : 0;
        pbase[so] = valid ? (unsigned)((n * p.OH + oy) * p.OW + ox) : 0u;
    }
    const unsigned ocs = (unsigned)(p.N * p.OH * p.OW);

    // W1 of a group: KS1 fp32 A fragments, or (X3) NM x 16 bytes of bf16 pairs per lane
    struct W1T { float f[X3 ? 1 : KS1]; u4_w2 x[X3 ? NM : 1]; };
    auto loadw = [&](int g, W1T &w1, float (&w2)[4]) {
        if (X3) {
#pragma unroll
            for (int m = 0; m < NM; m++) w1.x[m] = irbw_ld<u4_w2>(p.pk, (unsigned)((g * NM + m) * 64 + lane) * 16u);
        } else {
#pragma unroll
            for (int ks = 0; ks < KS1; ks++) w1.f[ks] = irbw_ld<float>(p.pk, (unsigned)((g * KS1 + ks) * 64 + lane) * 4u);
        }
#pragma unroll
        for (int i = 0; i < 4; i++) w2[i] = irbw_ld<float>(p.pk, (unsigned)(p.o_w2 + (g * 4 + i) * 64 + lane) * 4u);
    };
    W1T w1a, w1b;
    float w2a[4], w2b[4];
    loadw(0, w1a, w2a);

#pragma unroll
    for (int u = 0; u < 3; u++) if (tid + u * nthr < cs4) reinterpret_cast<v4f_w *>(smem)[tid + u * nthr] = cst[u];
    for (int i = tid + 3 * nthr; i < cs4; i += nthr)
        reinterpret_cast<v4f_w *>(smem)[i] = irbw_ld<v4f_w>(p.pk, (unsigned)(p.o_cs + 4 * i) * 4u);
    __syncthreads();                                            // shared constants visible (the only barrier)

    v4f_w acc[NSO][4];
#pragma unroll
    for (int so = 0; so < NSO; so++)
#pragma unroll
        for (int q = 0; q < 4; q++) acc[so][q] = z;
    const unsigned mb = interior ? 0xffffffffu : mbits;

    auto group = [&](int g, const W1T &w1, const float (&w2)[4]) {
        // expand: 16 channels x NSI strips -> activation, mask -> E slice [pair][half of the quad][quad][2 px][2 ch]
        const float *sbp = Sb1 + (g * 4 + kq) * 8;
        const v4f_w S4 = *reinterpret_cast<const v4f_w *>(sbp), B4 = *reinterpret_cast<const v4f_w *>(sbp + 4);
        const v2f_w sc[2] = { { S4.x, S4.y }, { S4.z, S4.w } }, bi[2] = { { B4.x, B4.y }, { B4.z, B4.w } };
#pragma unroll
        for (int si = 0; si < NSI; si++) {
            v4f_w a4[4] = { z, z, z, z };
            if (X3) {
#pragma unroll
                for (int m = 0; m < NM; m++) {
                    const v8bf_w2 A = __builtin_bit_cast(v8bf_w2, w1.x[m]);
#pragma unroll
                    for (int q = 0; q < 4; q++) a4[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, bop(si, q, m), a4[q], 0, 0, 0);
                }
            } else {
#pragma unroll
                for (int ks = 0; ks < KS1; ks++) {
                    a4[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.f[ks], xin[si][ks].x, a4[0], 0, 0, 0);
                    a4[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.f[ks], xin[si][ks].y, a4[1], 0, 0, 0);
                    a4[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.f[ks], xin[si][ks].z, a4[2], 0, 0, 0);
                    a4[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.f[ks], xin[si][ks].w, a4[3], 0, 0, 0);
                }
            }
#pragma unroll
            for (int rp = 0; rp < 2; rp++) {
                v2f_w y[4];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const v2f_w a = rp == 0 ? (v2f_w){ a4[q].x, a4[q].y } : (v2f_w){ a4[q].z, a4[q].w };
                    const v2f_w t = a * sc[rp] + bi[rp];
                    const v2f_w u = t * p.act1;
                    const bool in = (mb >> (si * 4 + q)) & 1u;      // the depthwise layer pads the EXPANDED tensor
                    y[q] = (v2f_w){ in ? act_max(t.x, u.x, fl_act1) : 0.f, in ? act_max(t.y, u.y, fl_act1) : 0.f };
                }
                float *dst = Ew + ((2 * kq + rp) * 2 * NQ + si * 16 + jq) * 4;
                *reinterpret_cast<v4f_w *>(dst) = (v4f_w){ y[0].x, y[0].y, y[1].x, y[1].y };
                *reinterpret_cast<v4f_w *>(dst + NQ * 4) = (v4f_w){ y[2].x, y[2].y, y[3].x, y[3].y };
            }
        }
        // depthwise on channel pairs from the E slice -> project MFMAs, for both output strips
#pragma unroll
        for (int m = 0; m < 2; m++) {
            const int pr = 2 * kq + m;
            const float *wdp = Wd + (g * 8 + pr) * 24;
            v4f_w T[6];
#pragma unroll
            for (int i = 0; i < 6; i++) T[i] = *reinterpret_cast<const v4f_w *>(wdp + 4 * i);
            const v2f_w tap[9] = { { T[0].x, T[0].y }, { T[0].z, T[0].w }, { T[1].x, T[1].y }, { T[1].z, T[1].w }, { T[2].x, T[2].y },
                                   { T[2].z, T[2].w }, { T[3].x, T[3].y }, { T[3].z, T[3].w }, { T[4].x, T[4].y } };
            const v2f_w sd = { T[4].z, T[4].w }, bd = { T[5].x, T[5].y };
            // rows r = 0..3 of the upper window: row r feeds tap row r of the upper quad and tap row r - 1 of the lower one
            // (per output the reference's order: tap rows ascending)
            const float *ep = Ew + (pr * 2 * NQ + (ebase[0] >> 2)) * 4;
            v2f_w dv[NSO][4];
#pragma unroll
            for (int so = 0; so < NSO; so++)
#pragma unroll
                for (int q = 0; q < 4; q++) dv[so][q] = (v2f_w){ 0.f, 0.f };
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float *row = ep + r * p.EW;
                v2f_w x[6];
#pragma unroll
                for (int i = 0; i < 3; i++) {                      // pixels 2i, 2i+1: quad i/2, half i&1
                    const v4f_w u = *reinterpret_cast<const v4f_w *>(row + ((i & 1) * NQ + (i >> 1)) * 4);
                    x[2 * i] = (v2f_w){ u.x, u.y }; x[2 * i + 1] = (v2f_w){ u.z, u.w };
                }
                if (r < 3) {
#pragma unroll
                    for (int q = 0; q < 4; q++)
#pragma unroll
                        for (int kx = 0; kx < 3; kx++) dv[0][q] += tap[r * 3 + kx] * x[q + kx];
                }
                if (r >= 1) {
#pragma unroll
                    for (int q = 0; q < 4; q++)
#pragma unroll
                        for (int kx = 0; kx < 3; kx++) dv[1][q] += tap[(r - 1) * 3 + kx] * x[q + kx];
                }
            }
#pragma unroll
            for (int so = 0; so < NSO; so++) {
                v2f_w bq[4];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const v2f_w t = dv[so][q] * sd + bd;
                    const v2f_w u = t * p.actd;
                    bq[q] = (v2f_w){ act_max(t.x, u.x, fl_actd), act_max(t.y, u.y, fl_actd) };
                }
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    const float a = w2[2 * m + j];
                    acc[so][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, j ? bq[0].y : bq[0].x, acc[so][0], 0, 0, 0);
                    acc[so][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, j ? bq[1].y : bq[1].x, acc[so][1], 0, 0, 0);
                    acc[so][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, j ? bq[2].y : bq[2].x, acc[so][2], 0, 0, 0);
                    acc[so][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, j ? bq[3].y : bq[3].x, acc[so][3], 0, 0, 0);
                }
            }
        }
    };

    if (active) {
        for (int g = 0; g < p.ngroups; g += 2) {                // two groups per trip: the register sets swap roles
            loadw(min(g + 1, p.ngroups - 1), w1b, w2b);
            __builtin_amdgcn_sched_barrier(0);                  // the prefetch stays a prefetch (see k_irbw)
            group(g, w1a, w2a);
            if (g + 1 < p.ngroups) {
                loadw(min(g + 2, p.ngroups - 1), w1a, w2a);
                __builtin_amdgcn_sched_barrier(0);
                group(g + 1, w1b, w2b);
            }
        }
    }

    // ---- output rows: register r holds channel 4kq + r for the lane's quad of each strip.  Three straight-line copies
    // (linear + shortcut: every block of yolo-fastest; linear; general): with the activation tests inside the element loop
    // the compiler computed every variant and selected per element -- 50 instructions per row instead of 8
    const bool lin_out = p.act2 == 1.f && p.res_act == 1.f;       // wave-uniform
    auto rows_out = [&](auto MODE) {
        constexpr int M = decltype(MODE)::value;                    // 0: linear + residual, 1: linear, 2: general
#pragma unroll
        for (int so = 0; so < NSO; so++) {
            v4f_w res[4];
            if (M == 0 || (M == 2 && p.residual)) {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const unsigned off = ((unsigned)min(4 * kq + r, p.oc - 1) * ocs + pbase[so]) * 4u;
                    if (p.vec == 4) res[r] = irbw_ld<v4f_w>(p.residual, nvalid[so] == 4 ? off : 0u);
                    else {
#pragma unroll
                        for (int q = 0; q < 4; q++) res[r][q] = irbw_ld<float>(p.residual, q < nvalid[so] ? off + 4u * q : 0u);
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int o = 4 * kq + r, oo = min(o, p.oc - 1);
                const v2f_w sb = *reinterpret_cast<const v2f_w *>(Sb2 + 2 * oo);
                // (four plain v_fma_f32 kept apart: left alone hipcc packs them into v_pk_fma_f32 with scale' / bias' broadcast out of the ONE register pair
                //  the ds_read_b64 above delivers -- the operand form that drops its addend next to bf16 MFMAs, DESIGN.md 5.10; tools/isa_lint.py keeps it out)
                v4f_w v = pw_fma4_apart(acc[so][0][r], acc[so][1][r], acc[so][2][r], acc[so][3][r], sb.x, sb.y);
                if (M == 0) v += res[r];
                if (M == 2) {
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        v[q] = irbw_act(v[q], p.act2, fl_act2);
                        if (p.residual) v[q] = irbw_act(v[q] + res[r][q], p.res_act, fl_res);
                    }
                }
                const unsigned off = ((unsigned)oo * ocs + pbase[so]) * 4u;
                if (o < p.oc) {
                    if (p.vec == 4) { if (nvalid[so] == 4) irbw_st<v4f_w>(p.out, off, v); }
                    else {
#pragma unroll
                        for (int q = 0; q < 4; q++) if (q < nvalid[so]) irbw_st<float>(p.out, off + 4u * q, v[q]);
                    }
                }
            }
        }
    };
    if (lin_out && p.residual) rows_out(std::integral_constant<int, 0>());
    else if (lin_out) rows_out(std::integral_constant<int, 1>());
    else rows_out(std::integral_constant<int, 2>());
}
