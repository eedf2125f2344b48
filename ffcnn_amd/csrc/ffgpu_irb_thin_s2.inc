// ffgpu_irb_thin_s2.inc -- a thin STRIDE-2 inverted-residual block (layers 9-11 of yolo-fastest: 4 -> 24 -> 8 channels, 160x160 -> 80x80) as one
// streaming kernel on the vector ALU: no MFMA, no LDS beyond the tap table.
//
//     1x1 expand (IC -> EC, act1) -> depthwise 3x3 s2 p1 (actd) -> 1x1 project (EC -> OC, act2)
//
// The design is k_irb_thin's (ffgpu_irb_thin.inc), turned to stride 2:
//   * a wave owns a band of OUTPUT rows and walks down it; F = 64 / lpr frames lie side by side in the wave (lpr = ceil(OW / NC) lanes per row, at most
//     32: NC = 3 on the 80-pixel rows gives 27 lanes, two frames, 54 lanes busy).  All slots walk the same band and row, so everything wave-uniform
//     stays wave-uniform.  An idle slot of the batch's last group re-reads the group's first frame and stores nothing;
//   * a lane owns NC output columns x0 .. x0 + NC - 1, that is input columns 2 x0 .. 2 x0 + 2 NC - 1; the one column to their left (2 x0 - 1) is the
//     left neighbour's last one and comes by a DPP shift, zero at a slot's first lane.  Where OW is not a multiple of NC the LAST lane of a row slides
//     left to end with the row (k_front's rule at three columns): it recomputes up to NC - 1 of its neighbour's outputs and stores the same values;
//   * output row y reads expanded rows 2y - 1, 2y, 2y + 1, so ONE partial row of depthwise sums is live (EC x NC values per lane): row 2y adds its
//     middle taps, row 2y + 1 the last ones -- the row is then scaled, activated and projected -- and at once starts row y + 1 with the first taps.
//     Per output that is the reference's tap order w0 .. w8 (the sum starts as the product w0 x, where the reference adds it to a zero: the same value,
//     but for the sign of a zero sum in front of the bias).  Row 2 y0 - 1 of a band's first step is the band's halo: one extra expanded row per band;
//   * an expanded value is computed once per band and never stored; outside the plane (row -1, row H of an odd height) it is zero -- the depthwise
//     layer pads the EXPANDED tensor -- while the loads are unconditional from clamped addresses;
//   * arithmetic is packed fp32 on channel PAIRS, the expand, the affine maps and the activations written as ffgpu_irb_thin_body.inc writes them;
//     the projection sums c = 0 .. EC - 1 in order; one store per output channel;
//   * the next input row is in flight during this row's arithmetic.
// The kernel reads the filter rows themselves (IrbDesc::w1 / wd / w2, staged into LDS once per workgroup); a wave-form plan's packed image is not touched.
// Restates conv-v6.c:46-91 / 96-229 / 46-91 (same tap order per layer).
struct ThinS2P {
    const float *in; float *out;
    const float *w1, *wd, *w2;       // filter rows (conv.h layout): w1 [EC][k4+4], wd [EC][16], w2 [OC][EC4+4]
    int W, H, N, OW, OH;             // input plane (W even), frames, output plane
    int lpr, F;                      // lanes per row = ceil(OW / NC) <= 32 (OW >= NC), frames per wave = 64 / lpr
    int band, nbands;                // output rows per wave
    float act1, actd, act2;          // slopes: act(x) = max(x, slope x)
    long ntasks;                     // ceil(N / F) * nbands
};

template <int IC, int EC, int OC, int NC>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) k_irb_thin_s2(ThinS2P p)
{
    static_assert(EC % 2 == 0 && OC % 2 == 0, "channel pairs");
    static_assert(NC >= 2 && NC <= 4, "columns per lane");
    constexpr int K4 = (IC + 3) & ~3, RL1 = K4 + 4, RL2 = ((EC + 3) & ~3) + 4, OCP = (OC + 3) & ~3, CP = EC / 2, NI = 2 * NC;
    // LDS tables, per channel pair cp (halves of a pair: expanded channels 2cp, 2cp+1):
    //   t1 [cp][IC + 2][2] : (w1[2cp][ci], w1[2cp+1][ci]) ..., (scale', scale'), (bias', bias')
    //   te [cp][4][2]      : the middle tap pairs w3 w4 w5, 0                     (an even input row reads these)
    //   to [cp][8][2]      : tap pairs w6 w7 w8, scale', bias', w0 w1 w2          (an odd input row: finish a row, start the next)
    //   t2 [cp][2][OCP]    : w2[k][2cp], k = 0..OCP-1, then w2[k][2cp+1]
    //   sb2 [2][OCP]       : scale' and bias' of the projection
    constexpr int T1 = (IC + 2) * 2, TE = 8, TO = 16, T2 = 2 * OCP;
    static_assert(T1 % 4 == 0 && T2 % 4 == 0, "16-byte table reads");
    __shared__ __attribute__((aligned(16))) float tw[CP * (T1 + TE + TO + T2) + 2 * OCP];
    float *t1 = tw, *te = tw + CP * T1, *to = te + CP * TE, *t2 = to + CP * TO, *tsb = t2 + CP * T2;
    for (int i = threadIdx.x; i < CP * T1; i += 256) {
        const int cp = i / T1, j = (i % T1) >> 1, c = 2 * cp + (i & 1);
        t1[i] = p.w1[c * RL1 + (j < IC ? j : K4 + (j - IC))];
    }
    for (int i = threadIdx.x; i < CP * TE; i += 256) {
        const int cp = i / TE, j = (i % TE) >> 1, c = 2 * cp + (i & 1);
        te[i] = j < 3 ? p.wd[c * 16 + 3 + j] : 0.f;
    }
    for (int i = threadIdx.x; i < CP * TO; i += 256) {
        const int cp = i / TO, j = (i % TO) >> 1, c = 2 * cp + (i & 1);
        to[i] = p.wd[c * 16 + (j < 3 ? 6 + j : (j < 5 ? 9 + j : j - 5))];      // w6 w7 w8 | scale' bias' (wd[12], wd[13]) | w0 w1 w2
    }
    for (int i = threadIdx.x; i < CP * T2; i += 256) {
        const int cp = i / T2, h = (i % T2) / OCP, k = i % OCP;
        t2[i] = k < OC ? p.w2[k * RL2 + 2 * cp + h] : 0.f;
    }
    for (int i = threadIdx.x; i < 2 * OCP; i += 256) { const int k = i % OCP; tsb[i] = k < OC ? p.w2[k * RL2 + RL2 - 4 + i / OCP] : 0.f; }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int task = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // wave-uniform, and known to be
    if (task >= p.ntasks) return;
    const int g = task / p.nbands, band_i = task - g * p.nbands;      // g: the group of F frames g F .. g F + F - 1
    const int slot = lane / p.lpr, hl = lane - slot * p.lpr;          // the lane's frame slot and its place in the row
    // a slot past the batch (the last group's) or past F (the wave's spare lanes) re-reads the group's first frame and stores nothing; nothing of it
    // reaches another slot (the left-neighbour select below is the kernel's only cross-lane traffic, and a slot's first lane takes zero instead)
    const bool have = slot < p.F && g * p.F + slot < p.N;
    const bool first_col = hl == 0, last_col = hl == p.lpr - 1;
    const int sl = p.lpr * NC - p.OW;                                 // wave-uniform: output columns the last lane slides left (0 .. NC - 1)
    const int x0 = last_col ? p.OW - NC : hl * NC;
    const int n = have ? g * p.F + slot : g * p.F;
    const unsigned HW = (unsigned)p.W * p.H, OHW = (unsigned)p.OW * p.OH;
    const unsigned cs = (unsigned)p.N * HW, ocs = (unsigned)p.N * OHW;       // channel strides; IC * cs, OC * ocs < 2^30 (the block's wave plan checks)
    // addresses = wave-uniform pointer (scalar registers) + 32-bit offset (the lane's frame is part of the offset)
    const unsigned lo = (unsigned)n * HW + 2u * x0, oo = (unsigned)n * OHW + x0;
    const int y0 = band_i * p.band, y1 = min(y0 + p.band, p.OH);
    typedef float v2f_s2 __attribute__((ext_vector_type(2)));
    const v2f_s2 z2 = { 0.f, 0.f };

    // input row r (clamped into the image: the loads are unconditional): 2 NC floats per channel from an 8-byte aligned address (W even), declared
    // dword aligned as the thin kernels' three- and five-column rows are
    typedef float v4a4 __attribute__((ext_vector_type(4), aligned(4)));
    typedef float v3a4 __attribute__((ext_vector_type(3), aligned(4)));
    typedef float v2a4 __attribute__((ext_vector_type(2), aligned(4)));
    struct Row { float c[IC][NI]; };
    auto load_row = [&](int r, Row &x) __attribute__((always_inline)) {
        const unsigned ro = (unsigned)min(max(r, 0), p.H - 1) * p.W + lo;
#pragma unroll
        for (int ci = 0; ci < IC; ci++) {
            const float *src = p.in + (ci * cs + ro);
            const v4a4 a = *reinterpret_cast<const v4a4 *>(src);
            x.c[ci][0] = a.x; x.c[ci][1] = a.y; x.c[ci][2] = a.z; x.c[ci][3] = a.w;
            if constexpr (NC == 3) { const v2a4 b = *reinterpret_cast<const v2a4 *>(src + 4); x.c[ci][4] = b.x; x.c[ci][5] = b.y; }
            if constexpr (NC == 4) { const v4a4 b = *reinterpret_cast<const v4a4 *>(src + 4); x.c[ci][4] = b.x; x.c[ci][5] = b.y; x.c[ci][6] = b.z; x.c[ci][7] = b.w; }
        }
    };
    // table reads: uniform addresses (broadcast), 16 bytes each
    struct W1T { v4f q[T1 / 4]; };
    struct WET { v4f q[TE / 4]; };
    struct WOT { v4f q[TO / 4]; v4f w2[T2 / 4]; };
    auto ld1 = [&](int cp) { W1T r;
#pragma unroll
        for (int j = 0; j < T1 / 4; j++) r.q[j] = *reinterpret_cast<const v4f *>(t1 + cp * T1 + 4 * j);
        return r; };
    auto lde = [&](int cp) { WET r;
#pragma unroll
        for (int j = 0; j < TE / 4; j++) r.q[j] = *reinterpret_cast<const v4f *>(te + cp * TE + 4 * j);
        return r; };
    auto ldo = [&](int cp) { WOT r;
#pragma unroll
        for (int j = 0; j < TO / 4; j++) r.q[j] = *reinterpret_cast<const v4f *>(to + cp * TO + 4 * j);
#pragma unroll
        for (int j = 0; j < T2 / 4; j++) r.w2[j] = *reinterpret_cast<const v4f *>(t2 + cp * T2 + 4 * j);
        return r; };

    v2f_s2 S[CP][NC];                 // the depthwise sums of the one output row under way, [pair][pixel]
    Row X[2];                         // input rows: odd rows arrive in X[0], even rows in X[1]; one is computed on while the other is in flight
#pragma unroll
    for (int c = 0; c < CP; c++)
#pragma unroll
        for (int j = 0; j < NC; j++) S[c][j] = z2;
    load_row(2 * y0 - 1, X[0]);

    // expanded row r arrives.  Even (r = 2y): the middle taps of output row y.  Odd (r = 2y + 1): the last taps of row y, which is finished, projected
    // and stored (not at the band's halo row 2 y0 - 1), then the first taps of row y + 1.
    auto step = [&](int r, auto PAR) {
        constexpr bool ODD = decltype(PAR)::value != 0;
        asm volatile("" ::: "memory");                             // the tables are re-read every row (hoisted out of the loop they would take every register)
        const bool rin = r >= 0 && r < p.H, fin = ODD && r > 2 * y0;   // wave-uniform
        const Row &x = X[ODD ? 0 : 1];
        if (r < 2 * y1 - 1) load_row(r + 1, X[ODD ? 1 : 0]);       // lands during this row's arithmetic
        v2f_s2 o[OCP / 2][NC];
        if constexpr (ODD) {
#pragma unroll
            for (int k = 0; k < OCP / 2; k++)
#pragma unroll
                for (int j = 0; j < NC; j++) o[k][j] = z2;
        }
        W1T n1 = ld1(0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int cp = 0; cp < CP; cp++) {
            // table reads run one stage ahead of their use; sched_barriers pin that order (as in ffgpu_irb_thin_body.inc)
            const W1T c1 = n1;
            WET ce; WOT co;
            if constexpr (ODD) co = ldo(cp); else ce = lde(cp);
            __builtin_amdgcn_sched_barrier(0);
            auto w1p = [&](int j) { return (j & 1) ? (v2f_s2){ c1.q[j >> 1].z, c1.q[j >> 1].w } : (v2f_s2){ c1.q[j >> 1].x, c1.q[j >> 1].y }; };
            auto wep = [&](int j) { return (j & 1) ? (v2f_s2){ ce.q[j >> 1].z, ce.q[j >> 1].w } : (v2f_s2){ ce.q[j >> 1].x, ce.q[j >> 1].y }; };
            auto wop = [&](int j) { return (j & 1) ? (v2f_s2){ co.q[j >> 1].z, co.q[j >> 1].w } : (v2f_s2){ co.q[j >> 1].x, co.q[j >> 1].y }; };
            v2f_s2 win[NI + 1];                                    // input column 2 x0 - 1 | the lane's 2 NC columns
            if (rin) {
#pragma unroll
                for (int j = 0; j < NI; j++) {
                    v2f_s2 a = w1p(0) * x.c[0][j];
#pragma unroll
                    for (int ci = 1; ci < IC; ci++) a += w1p(ci) * x.c[ci][j];
                    a = a * w1p(IC) + w1p(IC + 1);
                    const v2f_s2 u = a * p.act1;
                    win[1 + j] = (v2f_s2){ act_max(a.x, u.x, act_floor(p.act1)), act_max(a.y, u.y, act_floor(p.act1)) };
                }
            } else {                                               // the depthwise layer pads the EXPANDED tensor with zeros
#pragma unroll
                for (int j = 0; j < NI; j++) win[1 + j] = z2;
            }
            if (cp + 1 < CP) n1 = ld1(cp + 1);
            // the left neighbour's last column; the slid last lane's left column 2 (OW - NC) - 1 is its neighbour's column 2 NC - 1 - 2 sl; a slot's
            // first lane takes the padding (lane 0 receives the DPP's 0, the other slots' first lanes their neighbour slot's last column)
            win[0] = (v2f_s2){ dpp_shr1(win[NI].x), dpp_shr1(win[NI].y) };
            if (sl) {
                v2f_s2 src = win[NI - 2];
#pragma unroll
                for (int k = 2; k < NC; k++) if (sl == k) src = win[NI - 2 * k];
                const v2f_s2 alt = { dpp_shr1(src.x), dpp_shr1(src.y) };
                win[0] = (v2f_s2){ last_col ? alt.x : win[0].x, last_col ? alt.y : win[0].y };
            }
            win[0] = (v2f_s2){ first_col ? 0.f : win[0].x, first_col ? 0.f : win[0].y };
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (!ODD) {
#pragma unroll
                for (int j = 0; j < NC; j++) {
                    v2f_s2 m = S[cp][j];
                    m += wep(0) * win[2 * j]; m += wep(1) * win[2 * j + 1]; m += wep(2) * win[2 * j + 2];
                    S[cp][j] = m;
                }
            } else {
                if (fin) {
#pragma unroll
                    for (int j = 0; j < NC; j++) {
                        v2f_s2 d = S[cp][j];
                        d += wop(0) * win[2 * j]; d += wop(1) * win[2 * j + 1]; d += wop(2) * win[2 * j + 2];
                        d = d * wop(3) + wop(4);
                        const v2f_s2 u = d * p.actd;
                        d = (v2f_s2){ act_max(d.x, u.x, act_floor(p.actd)), act_max(d.y, u.y, act_floor(p.actd)) };
                        // projection: output-channel pairs, expanded channel 2cp then 2cp+1 (the reference's order)
#pragma unroll
                        for (int k = 0; k < OCP / 2; k++) {
                            const v4f &wa = co.w2[k >> 1], &wb = co.w2[(OCP / 2 + k) >> 1];
                            const v2f_s2 w2a = (k & 1) ? (v2f_s2){ wa.z, wa.w } : (v2f_s2){ wa.x, wa.y };
                            const v2f_s2 w2b = ((OCP / 2 + k) & 1) ? (v2f_s2){ wb.z, wb.w } : (v2f_s2){ wb.x, wb.y };
                            o[k][j] += w2a * d.x;
                            o[k][j] += w2b * d.y;
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < NC; j++) {
                    v2f_s2 s = wop(5) * win[2 * j];
                    s += wop(6) * win[2 * j + 1]; s += wop(7) * win[2 * j + 2];
                    S[cp][j] = s;
                }
            }
            // pin this pair's results here: plain arithmetic may otherwise be sunk past the barriers to its first use (the next row), which keeps
            // every channel's expanded values alive at once
#pragma unroll
            for (int j = 0; j < NC; j++) asm volatile("" : "+v"(S[cp][j]));
            if constexpr (ODD) {
                if (fin) {
#pragma unroll
                    for (int k = 0; k < OCP / 2; k++)
#pragma unroll
                        for (int j = 0; j < NC; j++) asm volatile("" : "+v"(o[k][j]));
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (ODD) {
            if (fin && have) {
                v4f sb[2 * OCP / 4];
#pragma unroll
                for (int j = 0; j < 2 * OCP / 4; j++) sb[j] = *reinterpret_cast<const v4f *>(tsb + 4 * j);
                const unsigned orow = (unsigned)((r - 1) >> 1) * p.OW + oo;
#pragma unroll
                for (int k = 0; k < OC / 2; k++) {
                    const v4f &sq = sb[k >> 1], &bq = sb[(OCP / 2 + k) >> 1];
                    const v2f_s2 sc = (k & 1) ? (v2f_s2){ sq.z, sq.w } : (v2f_s2){ sq.x, sq.y };
                    const v2f_s2 bi = ((OCP / 2 + k) & 1) ? (v2f_s2){ bq.z, bq.w } : (v2f_s2){ bq.x, bq.y };
                    v2f_s2 v[4];
#pragma unroll
                    for (int j = 0; j < NC; j++) {
                        const v2f_s2 t = o[k][j] * sc + bi, u = t * p.act2;
                        v[j] = (v2f_s2){ act_max(t.x, u.x, act_floor(p.act2)), act_max(t.y, u.y, act_floor(p.act2)) };
                    }
#pragma unroll
                    for (int h = 0; h < 2; h++) {
                        float *dst = p.out + ((2 * k + h) * ocs + orow);
                        if constexpr (NC == 2) *reinterpret_cast<v2a4 *>(dst) = (v2a4){ v[0][h], v[1][h] };
                        else if constexpr (NC == 3) *reinterpret_cast<v3a4 *>(dst) = (v3a4){ v[0][h], v[1][h], v[2][h] };
                        else *reinterpret_cast<v4a4 *>(dst) = (v4a4){ v[0][h], v[1][h], v[2][h], v[3][h] };
                    }
                }
            }
        }
    };
    step(2 * y0 - 1, std::integral_constant<int, 1>());            // the band's halo row
    for (int y = y0; y < y1; y++) {
        step(2 * y, std::integral_constant<int, 0>());
        step(2 * y + 1, std::integral_constant<int, 1>());
    }
}
