// ffgpu_dw_pair.inc -- depthwise 5x5 (stride 1, pad 2) on the SMALL planes of the detection heads (10x10x96, 20x20x120),
// two channels at a time.  Restates conv-v6.c:291-465 (tap order ky, kx per output; without the row-omission defect,
// which stays with k_dw_lds under FFGPU_COMPAT_V6).
//
// k_dw_lds spends five instructions around every FMA on these shapes (per-element index arithmetic while staging, one
// 4-byte LDS read per tap, scalar FMAs).  Here
//   * a workgroup owns ONE channel pair (2cp, 2cp+1) and NI frames: the 25 tap pairs are the same for every thread;
//   * the two planes of a frame are staged INTERLEAVED -- LDS tile [row][column][2 channels], zero border -- by
//     16-byte (8-byte when W % 4 != 0) global loads, so a pixel's two channels are one register pair and every tap is a
//     v_pk_fma_f32 whose operands are whole pairs (pairing adjacent PIXELS would cost a v_mov per shifted tap);
//   * a thread produces a 4-pixel x BR-row patch: input row r of the patch window is read once (four 16-byte LDS reads)
//     and folded into every output row it touches, ky ascending per output = the reference's order.
struct DwPairP {
    const float *in; const float *filt; float *out;
    int W, H, N, rowlen;
    int NI;                 // frames per workgroup
    int quads, bands, TPI;  // 4-pixel column groups, BR-row bands, threads per frame = quads * bands
    int LW, LH;             // tile row length in pixels (quads * 4 + 4) and rows (bands * BR + 4)
    int WQ;                 // staging units per row: W / VEC
    float slope;            // act(x) = max(x, slope x)
    unsigned m_tpi, m_quads, m_hwq, m_wq;     // ceil(2^32 / d): i / d == umulhi(i, m) while i * d < 2^32
};

typedef float v2f_dp __attribute__((ext_vector_type(2)));

template <int FS, int BR, int VEC>
__global__ void __launch_bounds__(256) k_dw_pair(DwPairP p)
{
    extern __shared__ __attribute__((aligned(16))) float dp_tile[];      // [NI][LH][LW][2]
    constexpr int PAD = FS / 2;
    const int tid = threadIdx.x;
    const int cp = blockIdx.y, n0 = blockIdx.x * p.NI, ni = min(p.NI, p.N - n0);
    const int plane2 = p.LH * p.LW * 2;
    const unsigned HW = (unsigned)p.W * p.H;
    // taps, scale', bias' of the two channels (the same addresses in every lane)
    const float *f0 = p.filt + (long)(2 * cp) * p.rowlen, *f1 = f0 + p.rowlen;
    v2f_dp tap[FS * FS];
#pragma unroll
    for (int t = 0; t < FS * FS; t++) tap[t] = (v2f_dp){ f0[t], f1[t] };
    const v2f_dp sc = { f0[p.rowlen - 4], f1[p.rowlen - 4] }, bi = { f0[p.rowlen - 3], f1[p.rowlen - 3] };

    // zero the tile (the border stays zero; the interior is overwritten below), then the interior
    for (int i = tid * 4; i < ni * plane2; i += 1024) *reinterpret_cast<v4f *>(dp_tile + i) = (v4f){ 0.f, 0.f, 0.f, 0.f };
    __syncthreads();
    const float *in0 = p.in + ((long)(2 * cp) * p.N + n0) * HW;          // channel 2cp, frame n0; channel 2cp+1 is N * HW further
    const unsigned chs = (unsigned)p.N * HW;
    const int units = ni * p.H * p.WQ;
    typedef float vin __attribute__((ext_vector_type(VEC)));
    for (int u0 = tid; u0 < units; u0 += 256 * 4) {
        vin a[4], b[4];
        unsigned dst[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {                                    // 8 loads in flight (unconditional, clamped)
            const int u = min(u0 + 256 * k, units - 1);
            const int i = (int)__umulhi((unsigned)u, p.m_hwq), rem = u - i * (p.H * p.WQ);
            const int y = (int)__umulhi((unsigned)rem, p.m_wq), xq = rem - y * p.WQ;
            const unsigned so = (unsigned)i * HW + (unsigned)y * p.W + xq * VEC;
            a[k] = *reinterpret_cast<const vin *>(in0 + so);
            b[k] = *reinterpret_cast<const vin *>(in0 + (chs + so));
            dst[k] = (unsigned)i * plane2 + ((y + PAD) * p.LW + xq * VEC + PAD) * 2;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (u0 + 256 * k >= units) break;
#pragma unroll
            for (int j = 0; j < VEC; j++) *reinterpret_cast<v2f_dp *>(dp_tile + dst[k] + 2 * j) = (v2f_dp){ a[k][j], b[k][j] };
        }
    }
    __syncthreads();

    const int i = (int)__umulhi((unsigned)tid, p.m_tpi);
    if (i >= ni) return;
    const int rem = tid - i * p.TPI;
    const int band = (int)__umulhi((unsigned)rem, p.m_quads), xq = rem - band * p.quads;
    const int y0 = band * BR;
    // window origin: tile row y0 (input row y0 - PAD), tile column 4 xq (input column 4 xq - PAD)
    const float *base = dp_tile + (unsigned)i * plane2 + (y0 * p.LW + xq * 4) * 2;
    v2f_dp acc[BR][4];
#pragma unroll
    for (int o = 0; o < BR; o++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[o][j] = (v2f_dp){ 0.f, 0.f };
    constexpr int NW = 4 + FS - 1, NQ = (NW + 1) / 2;                    // window pixels, 16-byte reads (2 pixels each)
#pragma unroll
    for (int r = 0; r < BR + FS - 1; r++) {
        v2f_dp win[2 * NQ];
#pragma unroll
        for (int k = 0; k < NQ; k++) {
            const v4f t = *reinterpret_cast<const v4f *>(base + r * p.LW * 2 + 4 * k);
            win[2 * k] = (v2f_dp){ t.x, t.y }; win[2 * k + 1] = (v2f_dp){ t.z, t.w };
        }
#pragma unroll
        for (int o = 0; o < BR; o++) {
            const int ky = r - o;
            if (ky < 0 || ky >= FS) continue;
#pragma unroll
            for (int kx = 0; kx < FS; kx++)
#pragma unroll
                for (int j = 0; j < 4; j++) acc[o][j] += win[j + kx] * tap[ky * FS + kx];
        }
    }
    float *out0 = p.out + ((long)(2 * cp) * p.N + n0) * HW;
#pragma unroll
    for (int o = 0; o < BR; o++) {
        if (y0 + o >= p.H) break;
        v2f_dp v[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const v2f_dp t = acc[o][j] * sc + bi, u = t * p.slope;
            v[j] = (v2f_dp){ act_max(t.x, u.x, act_floor(p.slope)), act_max(t.y, u.y, act_floor(p.slope)) };
        }
        const unsigned oo = (unsigned)i * HW + (unsigned)(y0 + o) * p.W + xq * 4;
        if (VEC == 4) {
            *reinterpret_cast<v4f *>(out0 + oo) = (v4f){ v[0].x, v[1].x, v[2].x, v[3].x };
            *reinterpret_cast<v4f *>(out0 + (chs + oo)) = (v4f){ v[0].y, v[1].y, v[2].y, v[3].y };
        } else {                                                         // W even: pixel pairs are valid together
            if (xq * 4 < p.W) {
                *reinterpret_cast<v2f_dp *>(out0 + oo) = (v2f_dp){ v[0].x, v[1].x };
                *reinterpret_cast<v2f_dp *>(out0 + (chs + oo)) = (v2f_dp){ v[0].y, v[1].y };
            }
            if (xq * 4 + 2 < p.W) {
                *reinterpret_cast<v2f_dp *>(out0 + oo + 2) = (v2f_dp){ v[2].x, v[3].x };
                *reinterpret_cast<v2f_dp *>(out0 + (chs + oo + 2)) = (v2f_dp){ v[2].y, v[3].y };
            }
        }
    }
}
