// ffgpu_conv_x3.inc -- dense 3x3 / stride 1 / pad 1 convolution (the backbone layer of every darknet cfg) with fp32-equivalent results on the
// BF16 matrix cores (gfx950), round 4.  The 3x3 sibling of ffgpu_pw_x3.inc.
//
// Restates conv-v0.c:7-44 for fs = 3, stride = 1, pad = 1, groups = 1:
//     Out[o][y][x] = act(scale'[o] * sum over (ci, ky, kx) of W[o][(ci * 3 + ky) * 3 + kx] * In[ci][y + ky - 1][x + kx - 1] + bias'[o]),   taps outside the plane skipped.
//
// Why: k_conv_igemm runs on v_mfma_f32_32x32x2_f32 at 0.40-0.48 of the fp32 matrix peak, and that peak is the fp32 VECTOR rate (157 TFLOP/s).  An
// fp32 number is exactly three bf16 numbers (see ffgpu_irb_wave.inc "X3"): six bf16 MFMAs with fp32 accumulation give what one fp32 MFMA gives -- to
// within a summation order -- in 6 / 16 of the matrix time.
//
// Structure: a workgroup of NW waves owns 16 MT output channels x NW pixel tiles; a WAVE owns 64 pixels x 16 MT channels for the whole K loop.
//   * pixel space: every output row padded to owp = ALIGN(ow, 4) columns; a lane (kq = lane >> 4, n = lane & 15) owns the QUAD of four consecutive
//     pixels 4 n .. 4 n + 3 of the wave's 64 (one row, whatever the width: the last quad of a ragged row slides left to end with the row) and, of every k-step, the eight k's 8 kq .. 8 kq + 7 -- as in k_pw_x3 its four
//     accumulators per 16 rows are four consecutive pixels (16-byte stores).
//   * K order: a k-UNIT = (block of 8 input channels, tap row ky); a GROUP = four consecutive units, one per lane quarter kq (3 ceil(ic / 8) units: no
//     padding to 32 channels -- a 16-channel layer is two groups) = three k-steps kx = 0, 1, 2 whose 32 k's are the four units at tap column kx.  The
//     lane loads, for each of its unit's 8 channels, input row y + ky - 1 at columns x - 1 .. x + 4 (the quad as one 16-byte load, its left and right
//     neighbour as two 4-byte loads), splits these 48 values ONCE into their three bf16 parts and packs the 8 channels of column j and part into one
//     16-byte MFMA operand pk[j][part]: the operand of pixel q at tap column kx is pk[q + kx][part] -- no further data movement, every loaded value
//     serves up to three taps (16 splits per k-step against the 32 of the pointwise kernel).
//   * weights: plan-time image of the three parts in fragment order, per (channel tile, group) one chunk of 9 MT pieces of 1 KB
//     [kx][16-row block][part][lane][16 bytes]; the chunk of the NEXT group arrives by LDS-DMA (global_load_lds_dwordx4, no staging registers) while
//     this group's MFMAs run: two LDS buffers, one barrier per group.  The next group's input loads are issued between the MFMAs as well (into the raw
//     registers the conversion has just emptied), so a group is a short pure-vector phase (the split) followed by a long matrix phase that carries all
//     memory instructions; with two workgroups of four waves per CU the two waves of a SIMD belong to different workgroups and run out of phase.
//   * per group and wave: 3 x MT x 6 terms x 4 pixels MFMAs (288 for MT = 4) against ~350 vector instructions of load / mask / split / pack.
// Workgroups of one pixel range sit on ONE XCD (its L2 serves the range's input rows to every channel tile), as in k_pw_x3.
struct IgX3P {
    const float *in; float *out; const float *residual; const float *filt;
    const unsigned *wpack;       // [channel tile][group][kx][row block][part][lane][4 dwords]
    long P, Pp;                  // pixels per channel: real (N oh ow) and row-padded (N oh owp)
    long ntn, npg;               // pixel tiles of 64 padded pixels; pixel ranges of NW tiles
    unsigned in_cs, in_ns;       // input strides in floats ((ic + 32) in_cs + N in_ns < 2^30: 32-bit lane offsets, checked by the launcher)
    int  iw, ih, ow, oh, ic, oc, owp, k4;   // input plane, output plane (= the input plane for stride 1), output row pitch of the padded pixel space
    int  nunits, ngr;            // k-units (8 input channels x one tap row) = 3 ic / 8 (ic % 8 == 0); groups of four units (one per lane quarter) = ceil(nunits / 4)
    int  nrb, ntm;               // 16-row blocks, channel tiles of MT blocks
    int  act, res_act;
    // the sparse forms of a yolo head's pointwise layer (SP = 1, 2; below): the head's list of pixel quads, its counter, the list's capacity in quads
    // (P / 4), the head's class count and objectness threshold
    int *sp_list, *sp_ctr;
    int  sp_cap, sp_classes;
    float sp_thresh;
};

// SPARSE HEAD (FS = 1; DESIGN.md 5.11): the layer in front of a yolo head (3 anchors, 5 + classes channels each) as two launches of this kernel, each on
// a row-permuted image of its own.  Row r of a form's image is the layer's output channel x3_sp_chan(r) (-1: a padding row):
//   SP = 1, the BOX pass: the 15 rows r = 5 a + v (v = tx, ty, tw, th, objectness) of anchor a, all pixels; a wave then puts the quads that hold a
//           (pixel, anchor) whose objectness passes k_yolo's own test (yolo_obj_pass) on the head's list;
//   SP = 2, the CLASS pass: the 3 x classes rows r = a classes + c, the listed quads only, sixteen list slots per wave.
// An output value depends on its filter row, its pixel and the K order alone -- not on the row block or the pixel slot that computes it -- so both passes
// write the dense launch's bits.
template <int SP>
__host__ __device__ static inline int x3_sp_chan(int classes, int r)
{
    if (SP == 1) return r < 15 ? (r / 5) * (5 + classes) + r % 5 : -1;
    if (SP == 2) return r < 3 * classes ? (r / classes) * (5 + classes) + 5 + r % classes : -1;
    return r;
}

struct IgX3PackP { const float *filt; unsigned *pk; int ic, oc, k4, nunits, ngr, ntm, MT, fs, sp, classes; };
__global__ void k_conv_x3_pack(IgX3PackP p)
{
    const int nkx = p.fs;                                             // k-steps per group: the tap columns (3), or one (pointwise form)
    const long total = (long)p.ntm * p.ngr * 3 * nkx * p.MT * 256;
    const int rl = p.k4 + 4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int d = (int)(i & 3), l = (int)((i >> 2) & 63);
        long t = i >> 8;
        const int part = (int)(t % 3); t /= 3;
        const int rb = (int)(t % p.MT); t /= p.MT;
        const int kx = (int)(t % nkx); t /= nkx;
        const int gr = (int)(t % p.ngr), mt = (int)(t / p.ngr);
        const int u = 4 * gr + (l >> 4), cb8 = u / nkx, ky = u - nkx * cb8;                // this lane quarter's k-unit (zero beyond the last one)
        const int r = 16 * (mt * p.MT + rb) + (l & 15), c = u < p.nunits ? 8 * cb8 + 2 * d : p.ic;
        const int o = p.sp == 1 ? x3_sp_chan<1>(p.classes, r) : (p.sp == 2 ? x3_sp_chan<2>(p.classes, r) : r);      // (the sparse forms' row maps; -1: a padding row)
        const float w0 = (o >= 0 && o < p.oc && c < p.ic) ? p.filt[(long)o * rl + (c * nkx + ky) * nkx + kx] : 0.f;
        const float w1 = (o >= 0 && o < p.oc && c + 1 < p.ic) ? p.filt[(long)o * rl + ((c + 1) * nkx + ky) * nkx + kx] : 0.f;
        p.pk[i] = irbw_x3_part(w0, part) | (irbw_x3_part(w1, part) << 16);
    }
}

// FS = 3: the 3x3 form described above.  FS = 1: the POINTWISE form of the same machinery for the small 1x1 layers of the heads (k_pw_x3 holds a whole
// weight tile in LDS and walks pixel tiles persistently: built for config[2], too coarse for 120 -> 255 channels on 25 600 pixels): a k-unit = 8
// channels, a group = ONE k-step of 32 channels, quads are four consecutive pixels of the flat CNHW pixel space (P % 4 == 0), no neighbours, no row masks.
// ST = 2 (FS = 3 only; even planes, iw = 2 ow): the downsampling 3x3 layers of yolov3 / yolov4-tiny.  A quad of four output pixels reads the NINE input columns
// 2 x - 1 .. 2 x + 7 (left neighbour + two quads, all inside the row), the operand of pixel q at tap column kx is pk[2 q + kx]; 108 + 72 registers of packed / raw
// values leave room for two 16-row blocks per wave at most.
// SP (FS = 1 only): 0 the dense form, 1 / 2 the box and the class pass of a sparse head (above).
template <int MT, int NW, int FS, int ST = 1, int SP = 0>
__global__ void __launch_bounds__(64 * NW, 8 / NW) __attribute__((amdgpu_waves_per_eu(2))) k_conv_x3(IgX3P p)
{
    static_assert(SP == 0 || (FS == 1 && ST == 1), "the sparse forms are pointwise");
    constexpr int NKX = FS, NCOL = FS == 1 ? 4 : (ST == 2 ? 9 : 6);   // k-steps per group; input columns per lane
    constexpr int CH = 3 * NKX * MT * 256;                            // dwords per weight chunk (one group)
    typedef v4f_x3 v4a4 __attribute__((aligned(4)));                  // (a row starts at any dword)
    typedef __attribute__((address_space(3))) void *lds_t;
    typedef const __attribute__((address_space(1))) void *glb_t;
    extern __shared__ __attribute__((aligned(16))) unsigned igx_lds[];    // [2][CH] + scale' / bias' [16 MT][2]
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kq = lane >> 4, n = lane & 15;
    const int xcd = (int)(blockIdx.x & 7);
    const long rr_ = (long)(blockIdx.x >> 3);
    const int mtile = (int)(rr_ % p.ntm);
    const long pg = (rr_ / p.ntm) * 8 + xcd;                          // pixel range: all its channel tiles on XCD blockIdx % 8
    if (pg >= p.npg) return;
    // class pass: the list's length (a count above the capacity comes from a forward that died midway: ALL quads then, by arithmetic index); a workgroup
    // whose first slot lies behind it has nothing to do.  The grid is the dense launch's (sixteen slots per wave cover P / 4 quads): it does not depend on data.
    unsigned sp_cnt = 0; bool sp_all = false;
    if (SP == 2) {
        const unsigned c = (unsigned)*p.sp_ctr;
        sp_all = c > (unsigned)p.sp_cap;
        sp_cnt = sp_all ? (unsigned)p.sp_cap : c;
        if ((unsigned long)pg * (16 * NW) >= sp_cnt) return;
    }
    const int rb0 = mtile * MT;
    float *sb = reinterpret_cast<float *>(igx_lds + 2 * CH);
    {
        const int rl = p.k4 + 4;
        for (int i = tid; i < MT * 32; i += 64 * NW) {
            const int o = x3_sp_chan<SP>(p.sp_classes, 16 * rb0 + (i >> 1));
            sb[i] = (o >= 0 && o < p.oc) ? p.filt[(long)o * rl + p.k4 + (i & 1)] : 0.f;
        }
    }

    // ---- this lane's quad: frame, row, first column in the row-padded pixel space
    const long pxt = pg * NW + wid;
    long pq = pxt * 64 + 4 * n;
    bool qvalid = pq < p.Pp;
    if (SP == 2) {                                                    // list slot 16 pxt + n: the quad's index (clamped: a lane never leaves the tensor)
        const unsigned slot = (unsigned)pxt * 16u + (unsigned)n;
        qvalid = slot < sp_cnt;
        const unsigned quad = !qvalid ? 0u : (sp_all ? slot : min((unsigned)p.sp_list[slot], (unsigned)p.sp_cap - 1u));
        pq = 4L * quad;
    }
    const unsigned pqu = (unsigned)(qvalid ? pq : 0);
    unsigned qn = 0; int qy = 0, qa = 0, qskip = 0;
    unsigned base_pix = pqu;                                          // FS = 1: contiguous CNHW, the flat pixel index itself
    bool okl = false, okr = false;
    if (FS == 3) {
        const unsigned plane = (unsigned)(p.oh * p.owp);
        qn = pqu / plane;
        const unsigned qrem = pqu - qn * plane;
        qy = (int)(qrem / (unsigned)p.owp);
        const int qx = (int)(qrem - (unsigned)qy * (unsigned)p.owp);
        // the row's last quad of a width that is no multiple of 4 STARTS at column iw - 4: it overlaps its left neighbour (those pixels are computed
        // twice and stored once) and every quad lies whole inside its row -- no access outside the row, no shifting of loaded columns
        qa = min(qx, p.ow - 4); qskip = qx - qa;                      // pixels q < qskip belong to the quad on the left
        base_pix = qvalid ? qn * p.in_ns + (unsigned)(ST * (qy * p.iw + qa)) : 0u;
        okl = qvalid && qa > 0; okr = ST == 1 && qvalid && qa + 4 < p.iw;
    }
    const int dl = okl ? -1 : 0, dr = okr ? 4 : 0;                    // neighbours: clamped into the row, masked afterwards
    const gfp bsrc = to_global(p.in);

    v4f_x3 acc[MT][4];
#pragma unroll
    for (int t = 0; t < MT; t++)
#pragma unroll
        for (int q = 0; q < 4; q++) acc[t][q] = (v4f_x3){ 0.f, 0.f, 0.f, 0.f };

    // raw input of one group: 8 channels x (left, quad, right).  This lane's k-unit of group gr is u = 4 gr + kq = (block of 8 channels u / 3, tap row u % 3)
    // (units beyond the last one: the last one again -- their weights are zero in the image)
    v4f_x3 rc[8], rd[ST == 2 ? 8 : 1]; float rl_[8], rr[8];      // (ST = 2: a second quad instead of the right neighbour)
    // of a group: off0 = offset of the unit's first channel at this lane's tap row (the quad's own row when that one lies outside the plane),
    // ok = the tap row lies inside the plane.  Channel j of the unit sits j in_cs behind: uniform bases (ic % 8 == 0: every unit is whole)
    gfp bj[8];
#pragma unroll
    for (int j = 0; j < 8; j++) bj[j] = bsrc + (size_t)j * p.in_cs;
    auto unit_of = [&](int gr, unsigned &off0, bool &ok) {
        const unsigned u = (unsigned)min(4 * gr + kq, p.nunits - 1);
        const bool real = 4 * gr + kq < p.nunits;                      // a unit beyond the last re-reads the last one: it counts as ZERO (its weights are zero: no 0 x Inf; round 6)
        if (FS == 3) {
            const unsigned cb8 = __umulhi(u, 0x55555556u);
            const int ky = (int)(u - 3u * cb8);
            ok = real && qvalid && (unsigned)(ST * qy + ky - 1) < (unsigned)p.ih;
            off0 = 8u * cb8 * p.in_cs + (ok ? base_pix + (unsigned)((ky - 1) * p.iw) : base_pix);
        } else {
            ok = real && qvalid;
            off0 = 8u * u * p.in_cs + base_pix;
        }
    };
    auto issue = [&](int j, unsigned off0) {
        rc[j] = gld<v4a4>(bj[j] + off0);
        if (FS == 3) {
            rl_[j] = *(bj[j] + (off0 + (unsigned)dl));
            if (ST == 2) rd[j] = gld<v4a4>(bj[j] + (off0 + 4u));
            else rr[j] = *(bj[j] + (off0 + (unsigned)dr));
        }
    };
    constexpr int NP = (3 * NKX * MT + NW - 1) / NW;                        // pieces of a weight chunk per wave
    auto glds1 = [&](int gr, int i, auto BUF) {                        // piece wid + NW i of group gr's weight chunk -> LDS buffer BUF (LDS-DMA)
        constexpr int buf = decltype(BUF)::value;
        const unsigned *src = p.wpack + ((size_t)mtile * p.ngr + gr) * CH;
        const int pc = wid + NW * i;
        if ((3 * NKX * MT) % NW == 0 || pc < 3 * NKX * MT)
            __builtin_amdgcn_global_load_lds((glb_t)(src + pc * 256 + lane * 4), (lds_t)(&igx_lds[buf * CH + pc * 256]), 16, 0, 0);
    };
    auto glds = [&](int gr, auto BUF) {
#pragma unroll
        for (int i = 0; i < NP; i++) glds1(gr, i, BUF);
    };

    glds(0, std::integral_constant<int, 0>{});
    bool rowok;                                                       // of the group whose raw values sit in rc / rl_ / rr
    {
        unsigned off0;
        unit_of(0, off0, rowok);
#pragma unroll
        for (int j = 0; j < 8; j++) issue(j, off0);
    }
    __builtin_amdgcn_s_waitcnt(0x0f70);                               // vmcnt(0): chunk 0 in LDS (see the barrier of the group body)
    __syncthreads();

    // channel pair d (channels 2 d, 2 d + 1 of the lane's unit) of the raw values -> dword d of every packed operand
    auto convert_pair = [&](auto INF, auto MASK, int d, bool ok, u4_x3 (&pk)[NCOL][3]) {
#pragma unroll
        for (int c = 0; c < NCOL; c++) {                              // (column by column: six temporaries alive, not 36)
            unsigned u[3][2];
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int j = 2 * d + h;
                float x;
                if (FS == 3 && ST == 2) x = c == 0 ? ((okl && ok) ? rl_[j] : 0.f) : (ok ? (c <= 4 ? rc[j][c >= 1 && c <= 4 ? c - 1 : 0] : rd[j][c >= 5 ? c - 5 : 0]) : 0.f);
                else if (FS == 3) x = c == 0 ? ((okl && ok) ? rl_[j] : 0.f) : (c == 5 ? ((okr && ok) ? rr[j] : 0.f) : (ok ? rc[j][c == 0 || c == 5 ? 0 : c - 1] : 0.f));
                else x = (decltype(MASK)::value && !ok) ? 0.f : rc[j][c < 4 ? c : 0];
                const float r = x3_resid_t<decltype(INF)::value>(x);                           // exact (INF: 0 for +-Inf)
                const float r2 = x3_resid2(r);                                                       // exact, <= 8 significant bits
                u[0][h] = __float_as_uint(x); u[1][h] = __float_as_uint(r); u[2][h] = __float_as_uint(r2);
            }
#pragma unroll
            for (int pt = 0; pt < 3; pt++) pk[c][pt][d] = __builtin_amdgcn_perm(u[pt][1], u[pt][0], 0x07060302u);
        }
    };

    // one group: LAST = the K loop's final group (no loads for a next one, no barrier behind it)
    auto group = [&](int gr, auto BUF, auto LAST) {
        constexpr int buf = decltype(BUF)::value;
        constexpr bool last = decltype(LAST)::value;
        unsigned noff0 = 0; bool nrowok = false;
        if (!last) unit_of(gr + 1, noff0, nrowok);
        // ---- this group's 48 values -> three bf16 parts, packed over the lane's 8 channels: pk[j][part] = column x - 1 + j
        u4_x3 pk[NCOL][3];
        // (round 6: a wave whose raw values hold an Inf -- max |x| over the group, half an instruction per value -- splits with the form that zeroes an Inf's
        //  residual parts; every other wave with round 5's instruction stream: ffgpu_irb_wave.inc, x3_resid_t)
        float amax = 0.f;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            amax = x3_amax3(x3_amax3(amax, rc[j][0], rc[j][1]), rc[j][2], rc[j][3]);
            if (FS == 3 && ST == 2) amax = x3_amax3(x3_amax3(x3_amax3(amax, rd[j][0], rd[j][1]), rd[j][2], rd[j][3]), rl_[j], rl_[j]);
            else if (FS == 3) amax = x3_amax3(amax, rl_[j], rr[j]);
        }
#ifndef X3_CONVX3_WAVE
#define X3_CONVX3_WAVE 1
#endif
        // FS = 1, round 6: `ok` = "the pixel quad exists and the k-unit is a real one".  A lane without a pixel quad stores nothing and a pixel column only feeds its own outputs, so its
        // values need no zeroing; a padded k-unit exists in the LAST group only (its weights are zero, its re-read values must count as zero: no 0 x Inf).  The select per value
        // (32 per group) therefore stays in the last group and in the 3x3 forms (rows outside the plane ARE zero padding).
        using MK = std::integral_constant<bool, FS != 1 || last>;
        if (X3_INF_X_CONV && (!X3_CONVX3_WAVE || x3_wave_has_inf(amax))) {
#pragma unroll
            for (int d = 0; d < 4; d++) convert_pair(std::true_type{}, MK{}, d, rowok, pk);
        } else {
#pragma unroll
            for (int d = 0; d < 4; d++) convert_pair(std::false_type{}, MK{}, d, rowok, pk);
        }
        // ---- three k-steps (tap columns) x MT row blocks x six terms (the small ones first) x four pixels
        const unsigned *A = igx_lds + buf * CH + lane * 4;
        u4_x3 a[3], an[3];
#pragma unroll
        for (int pt = 0; pt < 3; pt++) a[pt] = *reinterpret_cast<const u4_x3 *>(A + pt * 256);
#pragma unroll
        for (int kx = 0; kx < NKX; kx++)
#pragma unroll
            for (int t = 0; t < MT; t++) {
                const int nx = kx * MT + t + 1;
                if (!last) {
                    // the next group's loads and weight pieces ride in the issue slots the MFMAs leave free (first blocks: they have the rest of the
                    // group to land) instead of lengthening the vector phase in front of them: 5-13 % on every layer measured (issued in the vector
                    // phase -- the loads behind each converted channel pair, the pieces up front -- 384 -> 256 on 26x26 x 64: 356 us, here: 320 us)
                    constexpr int NB = NKX * MT, PB = (4 + NB - 1) / NB, GB = (NP + NB - 1) / NB;
                    const int b = nx - 1;
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int d = b * PB; d < (b + 1) * PB; d++) if (d < 4) { issue(2 * d, noff0); issue(2 * d + 1, noff0); }
#pragma unroll
                    for (int i = b * GB; i < (b + 1) * GB; i++) if (i < NP) glds1(gr + 1, i, std::integral_constant<int, buf ^ 1>{});
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (nx < NKX * MT) {
#pragma unroll
                    for (int pt = 0; pt < 3; pt++) an[pt] = *reinterpret_cast<const u4_x3 *>(A + (nx * 3 + pt) * 256);
                }
                constexpr int WP[6] = { 0, 1, 2, 0, 1, 0 }, XP[6] = { 2, 1, 0, 1, 0, 0 };
#pragma unroll
                for (int m = 0; m < 6; m++) {
                    const v8bf_x3 Af = __builtin_bit_cast(v8bf_x3, a[WP[m]]);
#pragma unroll
                    for (int q = 0; q < 4; q++)
                        acc[t][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Af, __builtin_bit_cast(v8bf_x3, pk[ST * q + kx][XP[m]]), acc[t][q], 0, 0, 0);
                }
                if (nx < NKX * MT) {
#pragma unroll
                    for (int pt = 0; pt < 3; pt++) a[pt] = an[pt];
                }
            }
        rowok = nrowok;
        __builtin_amdgcn_sched_barrier(0);                            // (nothing of the next group among this group's MFMAs: see below)
        if (!last) {
            // The LDS-DMA pieces of the next chunk must have LANDED before any wave crosses the barrier.  hipcc does not know that global_load_lds writes
            // LDS: it hoists the next group's split (which waits only for the raw loads -- vmcnt(n) with the pieces issued behind them still in flight) above
            // the barrier and emits no vmcnt(0) of its own.  Found as a sporadic wrong detection score (1 forward in ~400) with two half-batch chains
            // running concurrently (tests/test_gpu_round3.py::test_u8_frames_into_the_first_kernel[32-32]); alone the pieces always won the race.
            __builtin_amdgcn_s_waitcnt(0x0f70);                       // vmcnt(0)
            __syncthreads();
        }
    };
    {
        const std::integral_constant<int, 0> B0; const std::integral_constant<int, 1> B1;
        const std::false_type F; const std::true_type T;
        int gr = 0;
        for (; gr + 2 < p.ngr; gr += 2) { group(gr, B0, F); group(gr + 1, B1, F); }
        if (gr + 1 < p.ngr) { group(gr, B0, F); group(gr + 1, B1, T); }
        else group(gr, B0, T);
    }
    // Tried and removed (pointwise form): a software-pipelined body -- two sets of packed operands (2 x 48 registers), the split of group g + 1 placed BETWEEN the
    // MFMAs of group g with sched_group_barrier (1 MFMA : 3 vector instructions, the ISA showed the pattern), loads of group g + 2 behind it.  Parity-green, no
    // spill in the loop -- and config[2] 231 us instead of 167, 120 -> 255 22.5 instead of 15.4: vector instructions between MFMAs cost the matrix pipe more
    // than a separate vector phase does (the guide's "one extra issue slot between two MFMAs" price), so the phases stay apart.

    // ---- epilogue: acc[t][q][r] = Out[16 (rb0 + t) + 4 kq + r][quad pixel q]
    if (!qvalid) return;
    bool sp_hit = false;
    const float slope = p.act == 2 ? 0.1f : (p.act == 1 ? 0.f : 1.f), rslope = p.res_act == 2 ? 0.1f : (p.res_act == 1 ? 0.f : 1.f);
    const long px = FS == 3 ? ((long)qn * p.oh + qy) * p.ow + qa : pq;    // real pixel index of the quad's first pixel
    const bool vec = FS == 1 || (p.owp == p.ow && (p.P & 3) == 0);    // 16-byte stores: every quad 16-byte aligned (uniform)
#pragma unroll
    for (int t = 0; t < MT; t++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int o = x3_sp_chan<SP>(p.sp_classes, 16 * (rb0 + t) + 4 * kq + r);
            if (o >= 0 && o < p.oc) {
                const float sc = sb[2 * (16 * t + 4 * kq + r)], bi = sb[2 * (16 * t + 4 * kq + r) + 1];
                // (four plain v_fma_f32, kept apart: see k_pw_x3)
                v4f_pw v = pw_fma4_apart(acc[t][0][r], acc[t][1][r], acc[t][2][r], acc[t][3][r], sc, bi);
                v = pw_act4(v, slope, p.act == 3);
                const long off = (long)o * p.P + px;
                if (vec) {
                    if (p.residual) {
                        const v4f_pw q4 = *reinterpret_cast<const v4f_pw *>(p.residual + off);
                        v = pw_act4(v + q4, rslope, p.res_act == 3);
                    }
                    *reinterpret_cast<v4f_pw *>(p.out + off) = v;
                } else {
                    if (p.residual) {
                        v4f_pw q4 = { 0.f, 0.f, 0.f, 0.f };
#pragma unroll
                        for (int q = 0; q < 4; q++) if (q >= qskip) q4[q] = p.residual[off + q];
                        v = pw_act4(v + q4, rslope, p.res_act == 3);
                    }
#pragma unroll
                    for (int q = 0; q < 4; q++) if (q >= qskip) p.out[off + q] = v[q];
                }
                // box pass: rows 4, 9, 14 are the anchors' objectness -- k_yolo's test on the values just stored
                if (SP == 1 && (4 * kq + r) % 5 == 4)
                    sp_hit = sp_hit || yolo_obj_pass(v[0], p.sp_thresh) || yolo_obj_pass(v[1], p.sp_thresh) || yolo_obj_pass(v[2], p.sp_thresh) || yolo_obj_pass(v[3], p.sp_thresh);
            }
        }
    if (SP == 1) {
        // lane (kq, n) holds rows 4 kq .. 4 kq + 3 of quad n: the quad is listed when any of its lanes hit.  One ballot and one integer atomic per wave; the
        // append is guarded by the capacity (the counter may run past it: the class pass then takes every quad).  A wave with a live lane has lane 0 live.
        const unsigned long long hit = __ballot(sp_hit);
        const unsigned m16 = (unsigned)((hit | (hit >> 16) | (hit >> 32) | (hit >> 48)) & 0xffffu);
        if (m16) {
            int base = 0;
            if (lane == 0) base = atomicAdd(p.sp_ctr, __popc(m16));
            base = __builtin_amdgcn_readfirstlane(base);
            const int slot = base + __popc(m16 & ((1u << n) - 1u));
            if (kq == 0 && ((m16 >> n) & 1u) && (unsigned)slot < (unsigned)p.sp_cap) p.sp_list[slot] = (int)(pq >> 2);
        }
    }
}
