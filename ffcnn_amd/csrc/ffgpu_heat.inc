// ffgpu_heat.inc -- heat maps: the considered boxes of a stream accumulated into a grid of cells kept on the device, and the grid colour-mapped and
// alpha-blended into the frames (ffgpu_heat_boxes_dev, ffgpu_exec_heat, ffgpu_heat_blend_bgr_dev / _nv12_dev, ffgpu_heat_reset_dev, ffgpu_heat_state_bytes,
// ffgpu_heat_spec_check, ffgpu_heat_blend_spec_check, ffgpu_heat_palette).  The contract is in include/ffcnn_hip.h; the host side (specs, palette and
// argument checks) is ffgpu_heat_host.hpp.
//
// k_heat_accumulate: one workgroup per video stream and launch, as k_zones and k_trails, with their list walk (block_consider).  The stream's grid
// lies in LDS for the whole launch (dynamic, 64 KB at 128 x 128), loaded once and stored once.  Per frame the considered boxes' footprints are
// staged in LDS as integer cell rectangles; then every lane owns cells of one column, four of them in registers at a time, and sums over the boxes:
// one owner per cell, no LDS or global atomic, no order.  Peak and the saturated count are folded by block_fold.  Integer arithmetic but the anchor.
//
// k_heat_blend<NV12>: frame-driven with k_redact's ownership: a workgroup owns a 64 x 64 pixel block of its target anchored at (0, 0) and is the
// only one to read and write the block's bytes.  It first computes the levels of the cells the block can reach into LDS (34 x 34 at most), leaves if
// every one is below max(floor, 1), and then takes the block's rows: a lane owns an ALIGNED 32-bit word of a row, loads and stores it whole where
// all four bytes belong to the block's row segment and byte by byte at the segment's two ends, and stores only what changed.  Four rows are loaded
// before the first is mixed, so a wave waits for memory four times per block and not sixteen.  No barrier between a pixel's load and its store:
// nobody else reads it.
#define HEAT_BLOCK     64                             // the side of a blend block, in pixels
#define HEAT_REACH     34                             // cells per side a block can reach: 64 / 2 + 2
struct HeatArgs {
    StreamEntries<HEAT_ARG_ENTRIES> en;               // the launch's records, grouped by video stream (ffgpu_streams_host.hpp)
    unsigned char classes[256];
    int   nclasses, gw, gh, cell_log2, mode, anchor, spread, gain, decay_shift, ngroups;
    float min_score;
};
struct HeatBlendArgs {
    DrawTarget t[HEAT_ARG_TARGETS];                   // (first: the target's stream)
    unsigned   pal[256];                              // byte 0, 1, 2 of an entry: B G R (BGR targets) or Y U V (NV12 targets)
    int   gw, gh, cell_log2, full_scale, floor, opacity, smooth, ramp;
};
static_assert(sizeof(HeatArgs) + 5 * 8 <= 4096 - 256 && sizeof(HeatBlendArgs) + 1 * 8 <= 4096 - 256,
              "the tables travel as a kernel argument (4 KB at most, the hidden arguments included)");
static_assert(FFGPU_HEAT_DETS == 128 && FFGPU_HEAT_ROW == 8 && HEAT_STATE_HEADER == 16 && FFGPU_HEAT_MAX == 0x7fffffff, "k_heat_accumulate: the layouts of include/ffcnn_hip.h");
static_assert((unsigned long long)FFGPU_HEAT_MAX + (unsigned long long)FFGPU_HEAT_DETS * 65536ull < (1ull << 32),
              "k_heat_accumulate: a clamped cell and 128 gains fit 32 bits, so the 64-bit sum of the contract is held in one register");
static_assert(HEAT_BLOCK / 2 + 2 == HEAT_REACH && WAVE == 64, "k_heat_blend: cells of 2 pixels, one more cell on either side with FFGPU_HEAT_SMOOTH");

struct HeatLds {
    int4  rect[FFGPU_HEAT_DETS];                      // considered box j's footprint, cells x0, y0 .. x1, y1 inclusive, inside the grid (x0 > x1: none)
    int2  centre[FFGPU_HEAT_DETS];                    // FFGPU_HEAT_ANCHOR: the anchor's cell
    int   wsum[4];
    unsigned red[4];
    int4  hdr;                                        // the stream's header as it lies in memory
};

// grid = groups of the launch, 256 lanes, dynamic LDS: the grid's cells (rounded up to 16 bytes), then HeatLds.  Counts are clamped to [0, stride]
// as the draw kernel clamps them.  Total over any state bytes.
__global__ void __launch_bounds__(256) k_heat_accumulate(HeatArgs a, const ffgpu_frame_dets *recs, const BBOX *lists, int stride, unsigned char *state, int *rows)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char s_heat[];
    const int tid = threadIdx.x, g = blockIdx.x;
    const int e0 = a.en.goff[g], e1 = a.en.goff[g + 1], vs = a.en.gstream[g];
    if (vs < 0) {                                                                     // the ignored entries: every output byte zero (uniform)
        for (int e = e0; e < e1; e++)
            if (tid < FFGPU_HEAT_ROW) rows[(long)a.en.rec[e] * FFGPU_HEAT_ROW + tid] = 0;
        return;
    }
    const int gw = a.gw, gh = a.gh, ncell = gw * gh, k = a.cell_log2;
    const size_t cell_bytes = (4 * (size_t)ncell + 15) & ~(size_t)15;
    unsigned *const cell = reinterpret_cast<unsigned *>(s_heat);
    HeatLds &L = *reinterpret_cast<HeatLds *>(s_heat + cell_bytes);
    unsigned char *const gbase = state + (size_t)vs * (((size_t)HEAT_STATE_HEADER + 4 * (size_t)ncell + 15) & ~(size_t)15);
    unsigned *const gcell = reinterpret_cast<unsigned *>(gbase + HEAT_STATE_HEADER);
    if (tid == 0) L.hdr = *reinterpret_cast<const int4 *>(gbase);
    for (int i = tid; i < ncell; i += blockDim.x) cell[i] = gcell[i];
    __syncthreads();
    unsigned frames = (unsigned)L.hdr.x, peak = 0;                                    // (uniform; written back at the end)
    const float min_score = a.min_score;
    const int ext_w = gw << k, ext_h = gh << k, spread = a.spread, gain = a.gain, ds = a.decay_shift;
    const bool by_box = a.mode == FFGPU_HEAT_BOX, bottom = a.anchor != 0;
    // which cells a lane owns: the 256 lanes lie over the grid in rows of P = the power of two from gw up, R = 256 / P rows at a time -- no division
    const int psh = 32 - __clz(gw - 1), cx = tid & ((1 << psh) - 1), cy0 = tid >> psh, R = 256 >> psh;
    const int dmask = by_box ? 0 : 31;                                                // FFGPU_HEAT_BOX: gain >> 0 whatever the distance

    for (int e = e0; e < e1; e++) {
        const long t = a.en.rec[e];
        const ffgpu_frame_dets *rec = recs + t;
        const int n = max(0, min(lists ? rec->nfull : rec->count, stride));
        const BBOX *list = lists ? lists + a.en.first[e] : rec->box;

        // 1. the considered boxes, in list order; each straight into its footprint
        const long nq = block_consider(n, FFGPU_HEAT_DETS, L.wsum,
            [&](int i) { const BBOX &b = list[i]; return b.score >= min_score && (!a.nclasses || ((unsigned)b.type < (unsigned)a.nclasses && a.classes[(unsigned)b.type & 255u])); },
            [&](int ord, int i) {
                const BBOX b = list[i];
                int4 r = make_int4(1, 1, 0, 0);
                int2 c = make_int2(0, 0);
                if (by_box) {
                    const int A = draw_f2i(b.x1), B = draw_f2i(b.y1), C = draw_f2i(b.x2), D = draw_f2i(b.y2);
                    const int X0 = max(A, 0), Y0 = max(B, 0), X1 = min(C, ext_w - 1), Y1 = min(D, ext_h - 1);
                    if (A <= C && B <= D && X0 <= X1 && Y0 <= Y1) r = make_int4(X0 >> k, Y0 >> k, X1 >> k, Y1 >> k);
                } else {
                    const int ax = draw_f2i((b.x1 + b.x2) * 0.5f), ay = draw_f2i(bottom ? b.y2 : (b.y1 + b.y2) * 0.5f);
                    if (ax >= 0 && ax < ext_w && ay >= 0 && ay < ext_h) {
                        c = make_int2(ax >> k, ay >> k);
                        r = make_int4(max(c.x - spread, 0), max(c.y - spread, 0), min(c.x + spread, gw - 1), min(c.y + spread, gh - 1));
                    }
                }
                L.rect[ord] = r; L.centre[ord] = c;
            });
        const int nd = (int)min(nq, (long)FFGPU_HEAT_DETS), dropped = (int)min(nq - nd, 0x7fffffffL);
        const int outside = __syncthreads_count(tid < nd && L.rect[tid].x > L.rect[tid].z);

        // 2. decay, 3. deposit: a lane owns the cells of its column in rows cy0, cy0 + R, .. and takes them four at a time in registers, so a box's
        // footprint is read from LDS once per four cells and the four sums do not wait for each other
        unsigned mx = 0, nsat = 0;
        for (int cyb = cy0; cyb < gh && cx < gw; cyb += 4 * R) {
            unsigned v[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int cy = cyb + u * R;
                v[u] = cy < gh ? min(cell[cy * gw + cx], (unsigned)FFGPU_HEAT_MAX) : 0u;
                if (ds) v[u] -= (unsigned)(((unsigned long long)v[u] + (1u << ds) - 1u) >> ds);
            }
            for (int j = 0; j < nd; j++) {
                const int4 r = L.rect[j];
                const int2 c = L.centre[j];
                const bool xin = cx >= r.x && cx <= r.z;
                const int dx = abs(cx - c.x);
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int cy = cyb + u * R;
                    const unsigned add = (unsigned)gain >> (max(dx, abs(cy - c.y)) & dmask);      // (inside a footprint the distance is at most 4)
                    v[u] += xin && cy >= r.y && cy <= r.w ? add : 0u;
                }
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int cy = cyb + u * R;
                if (cy < gh) {
                    const unsigned w = min(v[u], (unsigned)FFGPU_HEAT_MAX);
                    cell[cy * gw + cx] = w;
                    mx = max(mx, w); nsat += w == (unsigned)FFGPU_HEAT_MAX;
                }
            }
        }
        // 4. peak and the row
        peak = block_fold(mx, L.red, 4, [](unsigned x, unsigned y) { return max(x, y); });
        const unsigned sat = block_fold(nsat, L.red, 4, [](unsigned x, unsigned y) { return x + y; });
        if (tid < FFGPU_HEAT_ROW)
            rows[t * FFGPU_HEAT_ROW + tid] = tid == 0 ? nd : tid == 1 ? dropped : tid == 2 ? outside : tid == 3 ? (int)frames : tid == 4 ? (int)peak : tid == 5 ? (int)sat : 0;
        frames++;
        __syncthreads();                                                              // (the next frame rewrites the footprints)
    }
    if (tid == 0) { L.hdr.x = (int)frames; L.hdr.y = (int)peak; *reinterpret_cast<int4 *>(gbase) = L.hdr; }
    for (int i = tid; i < ncell; i += blockDim.x) gcell[i] = cell[i];
}

// n / 255 for 0 <= n <= 65 152 (tests/test_heat_abi.py checks the identity over the whole range)
__device__ __forceinline__ unsigned heat_div255(unsigned n) { return (n + 1u + (n >> 8)) >> 8; }

// min(255, v 255 / F) for v <= FFGPU_HEAT_MAX, 1 <= F <= FFGPU_HEAT_MAX and rF = 1.0f / F, in the manner of blur_div: below F the quotient is under
// 255, so the float product is off by far less than 1 and its floor by at most one, which the 64-bit remainder shows and the corrections mend: exact.
__device__ __forceinline__ unsigned heat_level(unsigned v, unsigned F, float rF)
{
    if (v >= F) return 255u;
    long long q = (long long)((float)v * 255.0f * rF);
    const long long rem = (long long)v * 255 - q * (long long)F;
    if (rem < 0) q--; else if (rem >= (long long)F) q++;
    return (unsigned)q;
}

// what a lane needs of the block to turn a pixel into a level and an alpha
struct HeatPix {
    const unsigned char *lev;                         // LDS: the levels of cells ci0 .. , cj0 .. , ncx per row
    const unsigned *pal;                              // LDS: the palette
    int ci0, cj0, ncx, gw, gh, k, smooth, thr, opacity, ramp;
    // the level of picture pixel (X, Y), inside the extent
    __device__ __forceinline__ unsigned level(int X, int Y) const
    {
        if (!smooth) return lev[((Y >> k) - cj0) * ncx + (X >> k) - ci0];
        const int c = 1 << k, h = c >> 1;
        const int i0 = (X - h) >> k, j0 = (Y - h) >> k, fx = (X - h) & (c - 1), fy = (Y - h) & (c - 1);
        const int ia = max(i0, 0) - ci0, ib = min(i0 + 1, gw - 1) - ci0, ja = (max(j0, 0) - cj0) * ncx, jb = (min(j0 + 1, gh - 1) - cj0) * ncx;
        const unsigned L00 = lev[ja + ia], L10 = lev[ja + ib], L01 = lev[jb + ia], L11 = lev[jb + ib];
        return (L00 * (unsigned)((c - fx) * (c - fy)) + L10 * (unsigned)(fx * (c - fy)) + L01 * (unsigned)((c - fx) * fy) + L11 * (unsigned)(fx * fy) +
                (unsigned)(c * c / 2)) >> (2 * k);
    }
    // the alpha of a level: 0 = not written
    __device__ __forceinline__ unsigned alpha(unsigned l) const
    {
        if ((int)l < thr) return 0u;
        return ramp ? heat_div255(l * (unsigned)opacity + 127u) : (unsigned)opacity;
    }
};

// One row segment of the block: nb bytes at p, byte o of it channel CH0 + o % BPP of picture pixel (X0 + XSTEP (o / BPP), Y).  Lane l of the row owns
// the aligned word l of the words the segment touches (at most 49: 192 bytes and a misaligned start): o0 is its first byte's offset in the segment
// (-3 .. ), and a lane whose word lies behind the segment loads nothing, changes nothing and stores nothing.
__device__ __forceinline__ int heat_word(const unsigned char *p, int l) { return 4 * l - (int)(reinterpret_cast<uintptr_t>(p) & 3); }
__device__ __forceinline__ unsigned heat_load(const unsigned char *p, int nb, int o0)
{
    if (o0 >= 0 && o0 + 4 <= nb) return *reinterpret_cast<const unsigned *>(p + o0);
    unsigned old = 0;
    for (int j = 0; j < 4; j++) if (o0 + j >= 0 && o0 + j < nb) old |= (unsigned)p[o0 + j] << (8 * j);
    return old;
}
template <int BPP, int XSTEP, int CH0>
__device__ __forceinline__ unsigned heat_mix(const HeatPix &hp, unsigned old, int nb, int o0, int X0, int Y)
{
    unsigned nw = old;
    int qprev = -1;
    unsigned a = 0, colour = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int o = o0 + j;
        if (o < 0 || o >= nb) continue;
        const int q = o / BPP, ch = CH0 + o - q * BPP;
        if (q != qprev) {
            const unsigned lv = hp.level(X0 + XSTEP * q, Y);
            a = hp.alpha(lv); colour = hp.pal[lv]; qprev = q;
        }
        if (a) {
            const unsigned ob = (old >> (8 * j)) & 0xffu;
            const unsigned b = heat_div255(ob * (255u - a) + ((colour >> (8 * ch)) & 0xffu) * a + 127u);
            nw = (nw & ~(0xffu << (8 * j))) | b << (8 * j);
        }
    }
    return nw;
}
__device__ __forceinline__ void heat_store(unsigned char *p, int nb, int o0, unsigned old, unsigned nw)
{
    if (nw == old) return;
    if (o0 >= 0 && o0 + 4 <= nb) { *reinterpret_cast<unsigned *>(p + o0) = nw; return; }
    for (int j = 0; j < 4; j++)
        if (((nw ^ old) >> (8 * j)) & 0xffu) p[o0 + j] = (unsigned char)(nw >> (8 * j));
}
// nrows row segments of nb bytes, row y at p0 + y pitch and on picture row Y0 + YSTEP y: LPR lanes per row, 256 / LPR rows per pass, four passes'
// loads in front of their arithmetic
template <int BPP, int XSTEP, int CH0, int LPR>
__device__ __forceinline__ void heat_rows(const HeatPix &hp, unsigned char *p0, size_t pitch, int nrows, int nb, int X0, int Y0, int YSTEP)
{
    constexpr int RPP = 256 / LPR;
    const int l = threadIdx.x % LPR, r = threadIdx.x / LPR;
    for (int yb = r; yb < nrows; yb += 4 * RPP) {
        unsigned old[4];
        int o0[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int y = yb + u * RPP;
            unsigned char *p = p0 + (size_t)y * pitch;
            o0[u] = y < nrows ? heat_word(p, l) : nb;                                  // (behind the segment: the lane does nothing)
            old[u] = o0[u] < nb ? heat_load(p, nb, o0[u]) : 0u;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int y = yb + u * RPP;
            if (o0[u] < nb) heat_store(p0 + (size_t)y * pitch, nb, o0[u], old[u], heat_mix<BPP, XSTEP, CH0>(hp, old[u], nb, o0[u], X0, Y0 + YSTEP * y));
        }
    }
}

// grid (blocks of the launch's largest target inside the extent, targets of this launch), 256 lanes.  A workgroup beyond its target's own blocks
// leaves.  Every load and store lies inside the block, clipped to the target's w x h and to the extent.
template <bool NV12>
__global__ void __launch_bounds__(256) k_heat_blend(HeatBlendArgs a, const unsigned char *state)
{
    __shared__ unsigned char s_lev[HEAT_REACH * HEAT_REACH + 4];
    __shared__ unsigned s_pal[256];
    const DrawTarget &t = a.t[blockIdx.y];
    if (!t.p0) return;                                                                // a skipped target, or one of stream -1 (uniform)
    const int k = a.cell_log2, gw = a.gw, gh = a.gh;
    const int w = min(t.w, gw << k), h = min(t.h, gh << k);                            // what of the target lies inside the extent
    const int nbx = (w + HEAT_BLOCK - 1) / HEAT_BLOCK, nby = (h + HEAT_BLOCK - 1) / HEAT_BLOCK;
    if ((int)blockIdx.x >= nbx * nby) return;                                         // (uniform)
    const int bx0 = (int)(blockIdx.x % nbx) * HEAT_BLOCK, by0 = (int)(blockIdx.x / nbx) * HEAT_BLOCK, bw = min(HEAT_BLOCK, w - bx0), bh = min(HEAT_BLOCK, h - by0);
    const int tid = threadIdx.x;
    const unsigned char *const sbase = state + (size_t)t.first * (((size_t)HEAT_STATE_HEADER + 4 * (size_t)gw * (size_t)gh + 15) & ~(size_t)15);
    const unsigned F = a.full_scale >= 1 ? (unsigned)a.full_scale : min(reinterpret_cast<const unsigned *>(sbase)[1], (unsigned)FFGPU_HEAT_MAX);
    if (F == 0) return;                                                               // a peak of 0 draws nothing (uniform)
    const float rF = 1.0f / (float)F;

    // ---- the levels of the cells this block can reach
    const int half = a.smooth ? (1 << k) >> 1 : 0, more = a.smooth ? 1 : 0;
    const int ci0 = max((bx0 - half) >> k, 0), ci1 = min(((bx0 + bw - 1 - half) >> k) + more, gw - 1);
    const int cj0 = max((by0 - half) >> k, 0), cj1 = min(((by0 + bh - 1 - half) >> k) + more, gh - 1);
    const int ncx = ci1 - ci0 + 1, ncy = cj1 - cj0 + 1, thr = max(a.floor, 1);
    const unsigned *const gcell = reinterpret_cast<const unsigned *>(sbase + HEAT_STATE_HEADER);
    bool any = false;
    for (int i = tid; i < ncx * ncy; i += blockDim.x) {
        const int cy = i / ncx, cx = i - cy * ncx;
        const unsigned lv = heat_level(min(gcell[(size_t)(cj0 + cy) * gw + ci0 + cx], (unsigned)FFGPU_HEAT_MAX), F, rF);
        s_lev[i] = (unsigned char)lv;
        any |= (int)lv >= thr;
    }
    s_pal[tid] = a.pal[tid];
    if (!__syncthreads_or(any)) return;                                               // nothing to write: no pixel is loaded

    HeatPix hp;
    hp.lev = s_lev; hp.pal = s_pal; hp.ci0 = ci0; hp.cj0 = cj0; hp.ncx = ncx; hp.gw = gw; hp.gh = gh; hp.k = k; hp.smooth = a.smooth; hp.thr = thr;
    hp.opacity = a.opacity; hp.ramp = a.ramp;
    if (!NV12) {                                                                      // a wave per row: 192 bytes, 49 words at most
        heat_rows<3, 1, 0, 64>(hp, t.p0 + (size_t)by0 * (size_t)t.pitch + 3 * (size_t)bx0, (size_t)t.pitch, bh, 3 * bw, bx0, by0, 1);
    } else {                                                                          // half a wave per row: 64 bytes, 17 words at most
        heat_rows<1, 1, 0, 32>(hp, t.p0 + (size_t)by0 * (size_t)t.pitch + (size_t)bx0, (size_t)t.pitch, bh, bw, bx0, by0, 1);
        const int cbw = (bw + 1) >> 1, cbh = (bh + 1) >> 1;                            // chroma sample (i, jj) follows luma pixel (2 i, 2 jj)
        heat_rows<2, 2, 1, 32>(hp, t.p1 + (size_t)(by0 >> 1) * (size_t)t.pitch_uv + (size_t)bx0, (size_t)t.pitch_uv, cbh, 2 * cbw, bx0, by0, 2);
    }
}

// ---- host side
extern "C" size_t ffgpu_heat_state_bytes(int nstreams, int gw, int gh) { return ffgpu_heat_state_bytes_host(nstreams, gw, gh); }
extern "C" int ffgpu_heat_spec_check(const ffgpu_heat_spec *spec)
{
    HeatPlan pl;
    return ffgpu_heat_spec_plan("heat_spec_check", spec, pl);
}
extern "C" int ffgpu_heat_blend_spec_check(const ffgpu_heat_blend_spec *spec)
{
    HeatBlendPlan pl;
    return ffgpu_heat_blend_spec_plan("heat_blend_spec_check", spec, false, pl);
}
extern "C" int ffgpu_heat_palette(int nv12, unsigned char out[1024])
{
    if (!out) { ffgpu_set_error("heat_palette: NULL out"); return -1; }
    ffgpu_heat_palette_host(nv12, out);
    return 0;
}

// everything has been checked
int ffgpu_launch_heat(const DetSource &src, const int *streams, int ntargets, const HeatPlan &pl, void *d_state, void *d_rows, hipStream_t s)
{
    const size_t lds = ((4 * (size_t)pl.gw * (size_t)pl.gh + 15) & ~(size_t)15) + sizeof(HeatLds);
    if (lds_allow((const void *)k_heat_accumulate, lds, "heat_boxes")) return -1;
    for (int t0 = 0; t0 < ntargets; t0 += HEAT_ARG_ENTRIES) {
        const int nt = std::min(HEAT_ARG_ENTRIES, ntargets - t0);
        HeatArgs a;
        memset(&a, 0, sizeof a);
        memcpy(a.classes, pl.classes, sizeof a.classes);
        a.nclasses = pl.nclasses; a.gw = pl.gw; a.gh = pl.gh; a.cell_log2 = pl.cell_log2; a.mode = pl.mode; a.anchor = pl.anchor; a.spread = pl.spread;
        a.gain = pl.gain; a.decay_shift = pl.decay_shift; a.min_score = pl.min_score;
        a.ngroups = ffgpu_stream_entries(src.first, streams, t0, nt, a.en);
        hipLaunchKernelGGL(k_heat_accumulate, dim3((unsigned)a.ngroups), dim3(256), lds, s, a, src.recs, src.lists, src.stride, (unsigned char *)d_state, (int *)d_rows);
        LAUNCH_OK("heat_boxes");
    }
    return 0;
}

extern "C" int ffgpu_heat_reset_dev(void *d_state, int nstreams, int gw, int gh, int which_stream, void *stream)
{
    const char *const what = "heat_reset_dev";
    if (ffgpu_no_device(what)) return -1;
    const size_t all = ffgpu_heat_state_bytes(nstreams, gw, gh);
    if (!all) ffgpu_set_error("%s: %d streams of %d x %d cells (nstreams 1..65536, gw and gh 1..%d)", what, nstreams, gw, gh, HEAT_GRID_MAX);   // (stands unless the state is NULL)
    return ffgpu_state_reset(what, d_state, all, nstreams, which_stream, stream);
}

extern "C" int ffgpu_heat_boxes_dev(const void *d_records, const void *d_lists, int list_stride, const int *list_first, const int *streams, int ntargets,
                                    const ffgpu_heat_spec *spec, void *d_state, int nstreams, void *d_rows, void *stream)
{
    const char *const what = "heat_boxes_dev";
    if (ffgpu_no_device(what)) return -1;
    HeatPlan pl;
    if (ffgpu_heat_args_check(what, streams, ntargets, spec, d_state, nstreams, d_rows, pl)) return -1;
    DetSource src;
    if (ffgpu_source_dev(what, d_records, d_lists, list_stride, list_first, ntargets, src)) return -1;
    return ffgpu_launch_heat(src, streams, ntargets, pl, d_state, d_rows, (hipStream_t)stream);
}

// HEAT_ARG_TARGETS targets per launch, the grid sized by the launch's largest target inside the extent
template <class Frame>
static int heat_blend_dev(const char *what, const void *d_state, int nstreams, const int *streams, const Frame *targets, int ntargets,
                          const ffgpu_heat_blend_spec *spec, void *stream)
{
    const bool nv12 = std::is_same<Frame, ffgpu_nv12_frame>::value;
    if (ffgpu_no_device(what)) return -1;
    HeatBlendPlan pl;
    std::vector<DrawTarget> tab;
    if (ffgpu_heat_blend_args_check(what, d_state, nstreams, streams, targets, ntargets, spec, nv12, pl, tab)) return -1;
    const int ew = pl.gw << pl.cell_log2, eh = pl.gh << pl.cell_log2;
    auto blocks = [&](const DrawTarget &t) {
        return t.p0 ? (long long)((std::min(t.w, ew) + HEAT_BLOCK - 1) / HEAT_BLOCK) * ((std::min(t.h, eh) + HEAT_BLOCK - 1) / HEAT_BLOCK) : 0LL;
    };
    for (int t0 = 0; t0 < ntargets; t0 += HEAT_ARG_TARGETS) {
        const int nt = std::min(HEAT_ARG_TARGETS, ntargets - t0);
        HeatBlendArgs a;
        memset(&a, 0, sizeof a);
        memcpy(a.t, tab.data() + t0, sizeof(DrawTarget) * (size_t)nt);
        long long most = 0;
        for (int i = 0; i < nt; i++) most = std::max(most, blocks(a.t[i]));
        if (most == 0) continue;                                                       // every target of this launch is skipped
        memcpy(a.pal, pl.pal, sizeof a.pal);
        a.gw = pl.gw; a.gh = pl.gh; a.cell_log2 = pl.cell_log2; a.full_scale = pl.full_scale; a.floor = pl.floor; a.opacity = pl.opacity; a.smooth = pl.smooth;
        a.ramp = pl.ramp;
        const dim3 grid((unsigned)most, (unsigned)nt);
        if (nv12) hipLaunchKernelGGL(k_heat_blend<true>, grid, dim3(256), 0, (hipStream_t)stream, a, (const unsigned char *)d_state);
        else      hipLaunchKernelGGL(k_heat_blend<false>, grid, dim3(256), 0, (hipStream_t)stream, a, (const unsigned char *)d_state);
        LAUNCH_OK("heat_blend");
    }
    return 0;
}

extern "C" int ffgpu_heat_blend_bgr_dev(const void *d_state, int nstreams, const int *streams, const ffgpu_bgr_frame *targets, int ntargets,
                                        const ffgpu_heat_blend_spec *spec, void *stream)
{
    return heat_blend_dev("heat_blend_bgr_dev", d_state, nstreams, streams, targets, ntargets, spec, stream);
}

extern "C" int ffgpu_heat_blend_nv12_dev(const void *d_state, int nstreams, const int *streams, const ffgpu_nv12_frame *targets, int ntargets,
                                         const ffgpu_heat_blend_spec *spec, void *stream)
{
    return heat_blend_dev("heat_blend_nv12_dev", d_state, nstreams, streams, targets, ntargets, spec, stream);
}
