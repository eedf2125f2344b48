// ffgpu_irb_thin.inc -- the THIN inverted-residual blocks of yolo-fastest (8 expanded channels at 160x160:
// layers 1-3 and 4-8) as one streaming kernel, no LDS, no MFMA.
//
//     1x1 expand (IC -> EC, act1) -> depthwise 3x3 s1 p1 (actd) -> 1x1 project (EC -> OC, act2) [+ residual]
//
// With so few channels the three layers are pure bandwidth (48 B of traffic per pixel once fused, 160 B as
// three kernels) and the matrix cores would run 50-75 % empty, so this kernel is the streaming design of
// ffgpu_dw_stream.inc with the two pointwise layers folded in:
//   * a wave owns a frame's row segment: lane -> 4 columns; it walks DOWN a band of rows;
//   * per new input row: IC 16-byte loads, the expand is IC*EC*4 VALU FMAs per lane (taps are wave-uniform
//     scalars), the result is zeroed outside the image (the depthwise layer pads the EXPANDED tensor);
//   * an expanded row is never stored: channel by channel it is folded at once into the depthwise sums of the THREE
//     output rows it touches -- the row above gets its last tap row (and is then scaled, activated and projected), the
//     row itself its middle one, the row below its first -- which is the reference's tap order per output (w0..w8) and
//     leaves two partial rows (2 x EC x 4 px) in registers instead of three expanded ones; +-1 column taps come from the
//     neighbour lanes by DPP wave shifts, once per expanded value;
//   * projection + shortcut happen in registers; one 16-byte store per output channel;
//   * the 200-odd filter taps / scales sit in LDS (staged once per workgroup) and are read as broadcast 16-byte
//     ds_reads: as global loads (the compiler cannot keep that many in SGPRs, and cannot prove the output does not alias
//     them) every channel of every row waited for an L2 round trip -- the kernel ran at a third of its ALU time;
//   * the input row of the NEXT step is in flight while this step's depthwise / projection work runs.
// Restates conv-v6.c:46-91 / 96-229 / 46-91 and ffcnn.c:418-423 (same tap order per layer).
struct ThinP {
    const float *in; float *out; const float *residual;
    const float *w1, *wd, *w2;       // filter rows (conv.h layout): w1 [EC][k4+4], wd [EC][16], w2 [OC][EC4+4]
    int W, H, N;                     // plane geometry (W % 4 == 0, W/4 <= 64), frames
    int band, nbands;
    float act1, actd, act2, res_act; // slopes: act(x) = max(x, slope x)
    long ntasks;                     // N * nbands
};

typedef float v2f_t __attribute__((ext_vector_type(2)));

template <int IC, int EC, int OC>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) k_irb_thin(ThinP p)
{
    static_assert(EC % 2 == 0 && OC % 2 == 0, "channel pairs");
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
    const int n = task / p.nbands, band_i = task - n * p.nbands;
    const int lpr = p.W >> 2;
    const bool on = lane < lpr, last_col = lane == lpr - 1;
    const long HW = (long)p.W * p.H;
    const unsigned cs = (unsigned)p.N * (unsigned)HW;                 // channel stride; max(IC, OC) * cs < 2^30 (irb_thin_ok checks)
    // addresses = wave-uniform pointer (scalar registers) + 32-bit offset
    const unsigned lo = on ? lane * 4 : 0;                            // idle lanes work on column 0; nothing of theirs is stored
    const float *ip = p.in + (long)n * HW;
    float *op = p.out + (long)n * HW;
    const float *rp = p.residual ? p.residual + (long)n * HW : nullptr;
    const int y0 = band_i * p.band, y1 = min(y0 + p.band, p.H);
    const v2f_t z2 = { 0.f, 0.f };

    // input row r (clamped into the image: the loads are unconditional)
    auto load_row = [&](int r, v4f (&x)[IC]) {
        const unsigned ro = (unsigned)min(max(r, 0), p.H - 1) * p.W + lo;
#pragma unroll
        for (int ci = 0; ci < IC; ci++) x[ci] = *reinterpret_cast<const v4f *>(ip + (ci * cs + ro));
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
    v2f_t A[2][CP][4];
    v4f X[2][IC];                     // input rows: a step of parity P computes on X[P] while X[P^1] is in flight
#pragma unroll
    for (int c = 0; c < CP; c++)
#pragma unroll
        for (int j = 0; j < 4; j++) A[0][c][j] = A[1][c][j] = z2;
    load_row(y0 - 1, X[0]);

    // expanded row r arrives: finishes output row r - 1, continues r, starts r + 1 (per output the reference's tap order w0..w8)
    auto step = [&](int r, auto PAR) {
        constexpr int P = decltype(PAR)::value;
        asm volatile("" ::: "memory");                             // the tables are re-read every row (hoisted out of the loop they would take 200 registers)
        const bool rin = r >= 0 && r < p.H, fin = r > y0;          // wave-uniform
        const v4f (&x)[IC] = X[P];
        v4f res[OC];
        if (r < y1) load_row(r + 1, X[P ^ 1]);                     // lands during this step's arithmetic
        if (fin && rp) {
#pragma unroll
            for (int k = 0; k < OC; k++) res[k] = *reinterpret_cast<const v4f *>(rp + (k * cs + (unsigned)(r - 1) * p.W + lo));
        }
        v2f_t o[OCP / 2][4];
#pragma unroll
        for (int k = 0; k < OCP / 2; k++)
#pragma unroll
            for (int j = 0; j < 4; j++) o[k][j] = z2;
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
            v2f_t win[6];                                          // column -1 | the lane's four pixels | column +4
            if (rin) {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    v2f_t a = w1p(0) * x[0][j];
#pragma unroll
                    for (int ci = 1; ci < IC; ci++) a += w1p(ci) * x[ci][j];
                    a = a * w1p(IC) + w1p(IC + 1);
                    const v2f_t u = a * p.act1;
                    win[1 + j] = (v2f_t){ act_max(a.x, u.x, act_floor(p.act1)), act_max(a.y, u.y, act_floor(p.act1)) };
                }
            } else {                                               // the depthwise layer pads the EXPANDED tensor with zeros
#pragma unroll
                for (int j = 0; j < 4; j++) win[1 + j] = z2;
            }
            if (cp + 1 < CP) n1 = ld1(cp + 1);
            // neighbours: column -1 (lane 0 receives the DPP's 0) and column +4 (0 at the plane's right edge)
            win[0] = (v2f_t){ dpp_shr1(win[4].x), dpp_shr1(win[4].y) };
            const v2f_t sr = { dpp_shl1(win[1].x), dpp_shl1(win[1].y) };
            win[5] = (v2f_t){ last_col ? 0.f : sr.x, last_col ? 0.f : sr.y };
            __builtin_amdgcn_sched_barrier(0);
            if (fin) {
#pragma unroll
                for (int j = 0; j < 4; j++) {
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
            for (int j = 0; j < 4; j++) {
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
            for (int j = 0; j < 4; j++) asm volatile("" : "+v"(A[0][cp][j]), "+v"(A[1][cp][j]));
            if (fin) {
#pragma unroll
                for (int k = 0; k < OCP / 2; k++)
#pragma unroll
                    for (int j = 0; j < 4; j++) asm volatile("" : "+v"(o[k][j]));
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (fin && on) {
            v4f sb[2 * OCP / 4];
#pragma unroll
            for (int j = 0; j < 2 * OCP / 4; j++) sb[j] = *reinterpret_cast<const v4f *>(tsb + 4 * j);
#pragma unroll
            for (int k = 0; k < OC / 2; k++) {
                const v4f &sq = sb[k >> 1], &bq = sb[(OCP / 2 + k) >> 1];
                const v2f_t sc = (k & 1) ? (v2f_t){ sq.z, sq.w } : (v2f_t){ sq.x, sq.y };
                const v2f_t bi = ((OCP / 2 + k) & 1) ? (v2f_t){ bq.z, bq.w } : (v2f_t){ bq.x, bq.y };
                v2f_t v[4];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const v2f_t t = o[k][j] * sc + bi, u = t * p.act2;
                    v[j] = (v2f_t){ act_max(t.x, u.x, act_floor(p.act2)), act_max(t.y, u.y, act_floor(p.act2)) };
                }
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    v4f q = { v[0][h], v[1][h], v[2][h], v[3][h] };
                    if (rp) {
                        q += res[2 * k + h];
                        q.x = act_max(q.x, p.res_act * q.x, act_floor(p.res_act)); q.y = act_max(q.y, p.res_act * q.y, act_floor(p.res_act)); q.z = act_max(q.z, p.res_act * q.z, act_floor(p.res_act)); q.w = act_max(q.w, p.res_act * q.w, act_floor(p.res_act));
                    }
                    *reinterpret_cast<v4f *>(op + ((2 * k + h) * cs + (unsigned)(r - 1) * p.W + lo)) = q;
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
}
