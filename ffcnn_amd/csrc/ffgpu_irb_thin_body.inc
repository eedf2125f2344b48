// ffgpu_irb_thin_body.inc -- the body of k_irb_thin and of k_irb_thin_pair (ffgpu_irb_thin.inc includes it into each, so that both are kernels
// that read their own parameter block): IC, EC, OC, NC (columns per lane) and PAIR (two frames per wave) are the including kernel's constants.
    static_assert(EC % 2 == 0 && OC % 2 == 0, "channel pairs");
    static_assert(PAIR ? (NC >= 3 && NC <= 5) : NC == 4, "columns per lane");
    constexpr int K4 = (IC + 3) & ~3, RL1 = K4 + 4, RL2 = ((EC + 3) & ~3) + 4, OCP = (OC + 3) & ~3, CP = EC / 2;
    // All arithmetic runs on PAIRS (v_pk_fma_f32 / v_pk_mul_f32) whose halves are two CHANNELS at one pixel -- expanded
    // channels (2cp, 2cp+1) in the expand and depthwise stages, output channels (2kp, 2kp+1) in the projection -- so
    // a pixel's neighbour is simply another register pair (pairing adjacent PIXELS costs a v_mov per shifted tap: that
    // version issued 2.3 x the instructions).  LDS tables, per channel pair cp:
    //   t1 [cp][IC + 2][2] : (w1[2cp][ci], w1[2cp+1][ci]) ..., (scale', scale'), (bias', bias')
    //   td [cp][12][2]     : nine tap pairs, scale' pair, bias' pair, 0
    //   t2 [cp][2][OCP]    : w2[k][2cp], k = 0..OCP-1, then w2[k][2cp+1]
    //   sb2 [2][OCP]       : scale' and bias' of the projection
    constexpr int T1 = (IC + 2) * 2, TD = 24, T2 = 2 * OCP;
    __shared__ __attribute__((aligned(16))) float tw[CP * (T1 + TD + T2) + 2 * OCP];
    float *t1 = tw, *td = tw + CP * T1, *t2 = td + CP * TD, *tsb = t2 + CP * T2;
    for (int i = threadIdx.x; i < CP * T1; i += 256) {
        const int cp = i / T1, j = (i % T1) >> 1, c = 2 * cp + (i & 1);
        t1[i] = p.w1[c * RL1 + (j < IC ? j : K4 + (j - IC))];
    }
    for (int i = threadIdx.x; i < CP * TD; i += 256) {
        const int cp = i / TD, j = (i % TD) >> 1, c = 2 * cp + (i & 1);
        td[i] = j < 9 ? p.wd[c * 16 + j] : (j < 11 ? p.wd[c * 16 + 3 + j] : 0.f);
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
    const int n = task / p.nbands, band_i = task - n * p.nbands;      // n: the frame (PAIR: the frame pair, frames 2n and 2n + 1)
    const int lpr = PAIR ? p.W / NC : p.W >> 2;
    const int hl = PAIR ? lane & 31 : lane;                           // the lane within its frame's row
    // PAIR: the upper half of an odd batch's last pair has no frame -- it re-reads the pair's first frame and stores nothing; nothing
    // of it reaches another lane (the two neighbour selects below are the kernel's only cross-lane traffic)
    const bool have = !PAIR || lane < 32 || 2 * n + 1 < p.N;
    const bool on = PAIR ? hl < lpr && have : lane < lpr, last_col = hl == lpr - 1, first_col = hl == 0;
    const long HW = (long)p.W * p.H;
    const unsigned cs = (unsigned)p.N * (unsigned)HW;                 // channel stride; max(IC, OC) * cs < 2^30 (irb_thin_ok checks)
    // addresses = wave-uniform pointer (scalar registers) + 32-bit offset (PAIR: the upper half's frame is part of the offset)
    const unsigned lo = PAIR ? (hl < lpr ? hl * NC : 0) + (lane >= 32 && have ? (unsigned)HW : 0u) : (on ? lane * 4 : 0);   // idle lanes work on column 0; nothing of theirs is stored
    const float *ip = p.in + (long)(PAIR ? 2 * n : n) * HW;
    float *op = p.out + (long)(PAIR ? 2 * n : n) * HW;
    const float *rp = p.residual ? p.residual + (long)(PAIR ? 2 * n : n) * HW : nullptr;
    const int y0 = band_i * p.band, y1 = min(y0 + p.band, p.H);
    const v2f_t z2 = { 0.f, 0.f };

    // input row r (clamped into the image: the loads are unconditional)
    // NC = 5: columns 0-3 in the v4f, the fifth beside it; NC = 3: the v4f's first three.  A lane's 4 NC bytes start dword aligned, no
    // more, and the access types say so (as k_front's three-column form: gfx9 global accesses of 12 / 16 bytes need only that)
    typedef float v4a4 __attribute__((ext_vector_type(4), aligned(4)));
    typedef float v3a4 __attribute__((ext_vector_type(3), aligned(4)));
    constexpr int NE = NC == 5 ? 1 : 0;                               // fifth columns held
    constexpr bool RES_LATE = PAIR && IC + OC + (NC == 5 ? 4 : 0) >= 16;   // residual row read where it is added, not a step's arithmetic ahead
    auto load_cols = [&](const float *src, v4f &q, float &e) __attribute__((always_inline)) {
        if constexpr (NC == 4) q = *reinterpret_cast<const v4f *>(src);
        else if constexpr (NC == 5) { q = (v4f)*reinterpret_cast<const v4a4 *>(src); e = src[4]; }
        else { const v3a4 t = *reinterpret_cast<const v3a4 *>(src); q = (v4f){ t.x, t.y, t.z, 0.f }; }
    };
    auto load_row = [&](int r, v4f (&x)[IC], float (&xe)[IC * NE + 1]) {
        const unsigned ro = (unsigned)min(max(r, 0), p.H - 1) * p.W + lo;
#pragma unroll
        for (int ci = 0; ci < IC; ci++) load_cols(ip + (ci * cs + ro), x[ci], xe[ci * NE]);
    };
    // table reads: uniform addresses (broadcast), 16 bytes each
    struct W1T { v4f q[T1 / 4]; };
    struct WDT { v4f q[TD / 4]; v4f w2[T2 / 4]; };
    auto ld1 = [&](int cp) { W1T r;
#pragma unroll
        for (int j = 0; j < T1 / 4; j++) r.q[j] = *reinterpret_cast<const v4f *>(t1 + cp * T1 + 4 * j);
        return r; };
    auto ldd = [&](int cp) { WDT r;
#pragma unroll
        for (int j = 0; j < TD / 4; j++) r.q[j] = *reinterpret_cast<const v4f *>(td + cp * TD + 4 * j);
#pragma unroll
        for (int j = 0; j < T2 / 4; j++) r.w2[j] = *reinterpret_cast<const v4f *>(t2 + cp * T2 + 4 * j);
        return r; };
    auto pairof = [](const v4f (&q)[TD / 4 > T1 / 4 ? TD / 4 : T1 / 4], int j) { return (j & 1) ? (v2f_t){ q[j >> 1].z, q[j >> 1].w } : (v2f_t){ q[j >> 1].x, q[j >> 1].y }; };
    (void)pairof;

    // depthwise sums under way, [pair][pixel]: at a step of parity P, A[P] = the row being finished, A[P^1] = the row at its middle taps
    v2f_t A[2][CP][NC];
    v4f X[2][IC];                     // input rows: a step of parity P computes on X[P] while X[P^1] is in flight
    float XE[2][IC * NE + 1];         // (NC = 5: their fifth columns)
#pragma unroll
    for (int c = 0; c < CP; c++)
#pragma unroll
        for (int j = 0; j < NC; j++) A[0][c][j] = A[1][c][j] = z2;
    load_row(y0 - 1, X[0], XE[0]);

    // expanded row r arrives: finishes output row r - 1, continues r, starts r + 1 (per output the reference's tap order w0..w8)
    auto step = [&](int r, auto PAR) {
        constexpr int P = decltype(PAR)::value;
        asm volatile("" ::: "memory");                             // the tables are re-read every row (hoisted out of the loop they would take 200 registers)
        const bool rin = r >= 0 && r < p.H, fin = r > y0;          // wave-uniform
        const v4f (&x)[IC] = X[P];
        const float (&xe)[IC * NE + 1] = XE[P];
        auto xcol = [&](int ci, int j) __attribute__((always_inline)) {   // column j of the lane's NC
            if constexpr (NC == 5) return j < 4 ? x[ci][j & 3] : xe[ci];
            else return x[ci][j];
        };
        v4f res[OC];
        float rese[OC * NE + 1];
        if (r < y1) load_row(r + 1, X[P ^ 1], XE[P ^ 1]);          // lands during this step's arithmetic
        auto load_res = [&]() __attribute__((always_inline)) {
#pragma unroll
            for (int k = 0; k < OC; k++) load_cols(rp + (k * cs + (unsigned)(r - 1) * p.W + lo), res[k], rese[k * NE]);
        };
        if constexpr (!RES_LATE) if (fin && rp) load_res();
        v2f_t o[OCP / 2][NC];
#pragma unroll
        for (int k = 0; k < OCP / 2; k++)
#pragma unroll
            for (int j = 0; j < NC; j++) o[k][j] = z2;
        W1T n1 = ld1(0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int cp = 0; cp < CP; cp++) {
            // table reads run one stage ahead of their use; sched_barriers pin that order (left alone, the scheduler issues
            // every read of the row first and holds them all in registers)
            const W1T c1 = n1;
            const WDT cd = ldd(cp);
            __builtin_amdgcn_sched_barrier(0);
            auto w1p = [&](int j) { return (j & 1) ? (v2f_t){ c1.q[j >> 1].z, c1.q[j >> 1].w } : (v2f_t){ c1.q[j >> 1].x, c1.q[j >> 1].y }; };
            auto wdp = [&](int j) { return (j & 1) ? (v2f_t){ cd.q[j >> 1].z, cd.q[j >> 1].w } : (v2f_t){ cd.q[j >> 1].x, cd.q[j >> 1].y }; };
            v2f_t win[NC + 2];                                     // column -1 | the lane's NC pixels | column +NC
            if (rin) {
#pragma unroll
                for (int j = 0; j < NC; j++) {
                    v2f_t a = w1p(0) * xcol(0, j);
#pragma unroll
                    for (int ci = 1; ci < IC; ci++) a += w1p(ci) * xcol(ci, j);
                    a = a * w1p(IC) + w1p(IC + 1);
                    const v2f_t u = a * p.act1;
                    win[1 + j] = (v2f_t){ act_max(a.x, u.x, act_floor(p.act1)), act_max(a.y, u.y, act_floor(p.act1)) };
                }
            } else {                                               // the depthwise layer pads the EXPANDED tensor with zeros
#pragma unroll
                for (int j = 0; j < NC; j++) win[1 + j] = z2;
            }
            if (cp + 1 < CP) n1 = ld1(cp + 1);
            // neighbours: column -1 (lane 0 receives the DPP's 0) and column +NC (0 at the plane's right edge)
            win[0] = (v2f_t){ dpp_shr1(win[NC].x), dpp_shr1(win[NC].y) };
            if constexpr (PAIR) win[0] = (v2f_t){ first_col ? 0.f : win[0].x, first_col ? 0.f : win[0].y };   // (lane 32 receives frame A's last column)
            const v2f_t sr = { dpp_shl1(win[1].x), dpp_shl1(win[1].y) };
            win[NC + 1] = (v2f_t){ last_col ? 0.f : sr.x, last_col ? 0.f : sr.y };
            __builtin_amdgcn_sched_barrier(0);
            if (fin) {
#pragma unroll
                for (int j = 0; j < NC; j++) {
                    v2f_t d = A[P][cp][j];
                    d += wdp(6) * win[j]; d += wdp(7) * win[j + 1]; d += wdp(8) * win[j + 2];
                    d = d * wdp(9) + wdp(10);
                    const v2f_t u = d * p.actd;
                    d = (v2f_t){ act_max(d.x, u.x, act_floor(p.actd)), act_max(d.y, u.y, act_floor(p.actd)) };
                    // projection: output-channel pairs, expanded channel 2cp then 2cp+1 (the reference's order)
#pragma unroll
                    for (int k = 0; k < OCP / 2; k++) {
                        const v4f &wa = cd.w2[k >> 1], &wb = cd.w2[(OCP / 2 + k) >> 1];
                        const v2f_t w2a = (k & 1) ? (v2f_t){ wa.z, wa.w } : (v2f_t){ wa.x, wa.y };
                        const v2f_t w2b = ((OCP / 2 + k) & 1) ? (v2f_t){ wb.z, wb.w } : (v2f_t){ wb.x, wb.y };
                        o[k][j] += w2a * d.x;
                        o[k][j] += w2b * d.y;
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < NC; j++) {
                v2f_t m = A[P ^ 1][cp][j];
                m += wdp(3) * win[j]; m += wdp(4) * win[j + 1]; m += wdp(5) * win[j + 2];
                A[P ^ 1][cp][j] = m;
                v2f_t s = wdp(0) * win[j];
                s += wdp(1) * win[j + 1]; s += wdp(2) * win[j + 2];
                A[P][cp][j] = s;
            }
            // pin this pair's results here: plain arithmetic may otherwise be sunk past the barriers to its first use (the
            // next step), which keeps every channel's expanded values alive at once
#pragma unroll
            for (int j = 0; j < NC; j++) asm volatile("" : "+v"(A[0][cp][j]), "+v"(A[1][cp][j]));
            if (fin) {
#pragma unroll
                for (int k = 0; k < OCP / 2; k++)
#pragma unroll
                    for (int j = 0; j < NC; j++) asm volatile("" : "+v"(o[k][j]));
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (fin && on) {
            if constexpr (RES_LATE) if (rp) load_res();                // (the widest paired forms: prefetched, the residual row is what spills)
            v4f sb[2 * OCP / 4];
#pragma unroll
            for (int j = 0; j < 2 * OCP / 4; j++) sb[j] = *reinterpret_cast<const v4f *>(tsb + 4 * j);
#pragma unroll
            for (int k = 0; k < OC / 2; k++) {
                const v4f &sq = sb[k >> 1], &bq = sb[(OCP / 2 + k) >> 1];
                const v2f_t sc = (k & 1) ? (v2f_t){ sq.z, sq.w } : (v2f_t){ sq.x, sq.y };
                const v2f_t bi = ((OCP / 2 + k) & 1) ? (v2f_t){ bq.z, bq.w } : (v2f_t){ bq.x, bq.y };
                v2f_t v[NC < 4 ? 4 : NC];
#pragma unroll
                for (int j = 0; j < NC; j++) {
                    const v2f_t t = o[k][j] * sc + bi, u = t * p.act2;
                    v[j] = (v2f_t){ act_max(t.x, u.x, act_floor(p.act2)), act_max(t.y, u.y, act_floor(p.act2)) };
                }
                if constexpr (NC < 4) v[3] = z2;
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    v4f q = { v[0][h], v[1][h], v[2][h], v[3][h] };
                    float qe = NC == 5 ? v[NC - 1][h] : 0.f;
                    if (rp) {
                        q += res[2 * k + h];
                        q.x = act_max(q.x, p.res_act * q.x, act_floor(p.res_act)); q.y = act_max(q.y, p.res_act * q.y, act_floor(p.res_act)); q.z = act_max(q.z, p.res_act * q.z, act_floor(p.res_act)); q.w = act_max(q.w, p.res_act * q.w, act_floor(p.res_act));
                        if constexpr (NC == 5) { qe += rese[2 * k + h]; qe = act_max(qe, p.res_act * qe, act_floor(p.res_act)); }
                    }
                    float *dst = op + ((2 * k + h) * cs + (unsigned)(r - 1) * p.W + lo);
                    if constexpr (NC == 4) *reinterpret_cast<v4f *>(dst) = q;
                    else if constexpr (NC == 5) { *reinterpret_cast<v4a4 *>(dst) = (v4a4)q; dst[4] = qe; }
                    else *reinterpret_cast<v3a4 *>(dst) = (v3a4){ q.x, q.y, q.z };
                }
            }
        }
    };
    int r = y0 - 1;                                                // steps y0-1 .. y1, two per trip (the parity is a compile-time role swap)
    for (; r < y1; r += 2) {
        step(r, std::integral_constant<int, 0>());
        step(r + 1, std::integral_constant<int, 1>());
    }
    if (r == y1) step(r, std::integral_constant<int, 0>());
