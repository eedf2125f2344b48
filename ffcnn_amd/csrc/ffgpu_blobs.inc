// ffgpu_blobs.inc -- motion blobs: the active cells of a stream's motion state labelled into connected components, and the components written as
// boxes in the record layout (ffgpu_blobs_spec_check, ffgpu_blobs_dev).  The contract is in include/ffcnn_hip.h; the host side (spec, LDS layout,
// argument checks) is ffgpu_blobs_host.hpp.  Only reads the state.
//
// k_blobs: one workgroup of 16 waves per target; the whole grid lives in LDS, up to 32768 cells.  A WORD is 64 consecutive cells of one row of the
// grid: a wave takes a word, a lane a cell of it, so the row's bit mask comes from one ballot and every question about runs is bit arithmetic on it.
//   1. masks: the cells read once, coalesced; ballot(count >= min_pixels) -> s_mask[row][word].
//   2. runs: every active cell's label = the raster index of its run's first cell (L, a short per cell; 0xFFFF: inactive).  The label of a run's
//      first cell is the run's PARENT in the union-find forest: a first cell always points at a first cell with a smaller or equal index.
//   3. union: the lane of a run's first cell unites the run with every run of the row above that it overlaps (widened by a cell for connect 8).
//      Lock-free: find walks the parents, the larger root is hooked onto the smaller by an atomic min, the walked path is compressed by atomic
//      mins.  LDS has no 16-bit atomics: blobs_min16 is a compare-and-swap on the dword that holds the short.  Parents only ever decrease, so the
//      forest stays a forest, and the root of a component is its smallest raster index whatever the order.
//   4. flatten, number, table: every active cell's label becomes its root; the roots are ranked in raster order (block_rank), a root's label
//      becomes 0x8000 | its number; the first 2048 get a table entry, accumulated per run SEGMENT (the part of a run inside a word) with integer
//      LDS atomics: cells, area, pixels (a wave prefix sum over the word's cells), the cell bounding box.
//   5. select: the kept entries' 64-bit keys (pixels descending, cells descending, root ascending) sorted by block_bitonic; the first max_boxes
//      are the record's boxes; labels, record and words stored from owning lanes.
// Integer LDS atomics only (sums, minima and maxima: any order gives the same bits); no global atomics; the same bytes on every run.
struct BlobsArgs {
    int stream[BLOBS_ARG_TARGETS];                    // target e of the launch: its video stream, or -1
    int w, h, k, gw, gh, wpr, ncell, ntab, npow2, min_pixels, warmup, connect, min_cells, max_cells, max_boxes, pad, type;
    unsigned mask_off, tab_off, key_off, rank_off;
    unsigned long long cells_off, stream_bytes, label_pitch;
};
static_assert(sizeof(BlobsArgs) + 4 * 8 <= 4096 - 256, "the table travels as a kernel argument (4 KB at most, the hidden arguments included)");
static_assert(FFGPU_BLOBS_WORDS == 8 && BLOBS_LANES == 16 * WAVE && FFGPU_BLOBS_MAX_CELLS <= 0x8000 && FFGPU_MAX_DET <= BLOBS_LANES, "k_blobs: the layouts of include/ffcnn_hip.h");
#define BLOBS_NONE 0xFFFFu                            // the label of an inactive cell
#define BLOBS_ROOT 0x8000u                            // a numbered root's label: BLOBS_ROOT | number (numbers < 16384: at most half the cells are roots)

// min(L[i], v) -> L[i]; returns what L[i] held
__device__ __forceinline__ unsigned blobs_min16(unsigned short *L, unsigned i, unsigned v)
{
    unsigned *const wp = reinterpret_cast<unsigned *>(L) + (i >> 1);
    const unsigned sh = (i & 1u) * 16u;
    unsigned old = *reinterpret_cast<volatile unsigned *>(wp);
    for (;;) {
        const unsigned cur = (old >> sh) & 0xFFFFu;
        if (cur <= v) return cur;
        const unsigned got = atomicCAS(wp, old, (old & ~(0xFFFFu << sh)) | (v << sh));
        if (got == old) return cur;
        old = got;
    }
}
// the root above active cell x
__device__ __forceinline__ unsigned blobs_find(const unsigned short *L, unsigned x)
{
    const volatile unsigned short *const V = L;
    for (unsigned p; (p = V[x]) != x; x = p) {}
    return x;
}
// find, and every cell on the walked path pointed at the root (or at whatever smaller parent it has got meanwhile)
__device__ __forceinline__ unsigned blobs_find_compress(unsigned short *L, unsigned x)
{
    const unsigned r = blobs_find(L, x);
    while (x > r) x = blobs_min16(L, x, r);
    return r;
}
__device__ __forceinline__ void blobs_unite(unsigned short *L, unsigned a, unsigned b)
{
    for (;;) {
        a = blobs_find_compress(L, a); b = blobs_find_compress(L, b);
        if (a == b) return;
        if (a < b) { const unsigned t = a; a = b; b = t; }
        const unsigned old = blobs_min16(L, a, b);    // a was a root when found: hook it onto b
        if (old == a) return;
        a = old;                                      // it has been hooked meanwhile: its other parent and b are one component too
    }
}
// the component number of active cell c once the roots are numbered (every active cell points at its root)
__device__ __forceinline__ unsigned blobs_number(const unsigned short *L, unsigned c)
{
    const unsigned v = L[c];
    return ((v & BLOBS_ROOT) ? v : L[v]) & 0x7FFFu;
}
// the length of the run of set bits of m that starts at bit `lane` (a set bit), cut at the word's end
__device__ __forceinline__ int blobs_runlen(unsigned long long m, int lane)
{
    const unsigned long long z = ~(m >> lane);        // (the bits shifted in are zero: the run ends at the word's end)
    return z ? __builtin_ctzll(z) : 64;
}

// grid = targets of this launch (target t0 + blockIdx.x of the call), BLOBS_LANES lanes, lds bytes of dynamic LDS (ffgpu_blobs_lds).  Every load
// lies inside the stream's header and cells, every store inside the target's words, record and gw * gh labels.
__global__ void __launch_bounds__(BLOBS_LANES) k_blobs(BlobsArgs a, const unsigned char *state, int t0, int *words, ffgpu_frame_dets *out_recs, unsigned short *labels)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_blobs[];
    __shared__ int s_wsum[16], s_red[16];
    unsigned short *const L = reinterpret_cast<unsigned short *>(s_blobs);
    unsigned long long *const s_mask = reinterpret_cast<unsigned long long *>(s_blobs + a.mask_off);
    unsigned *const t_cells = reinterpret_cast<unsigned *>(s_blobs + a.tab_off);
    const int ntab = a.ntab;
    unsigned *const t_area = t_cells + ntab, *const t_pix = t_area + ntab, *const t_i0 = t_pix + ntab, *const t_i1 = t_i0 + ntab, *const t_j1 = t_i1 + ntab;
    unsigned long long *const s_key = reinterpret_cast<unsigned long long *>(s_blobs + a.key_off);
    unsigned short *const s_rank = reinterpret_cast<unsigned short *>(s_blobs + a.rank_off);

    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE, vs = a.stream[blockIdx.x];
    const long t = (long)t0 + blockIdx.x;
    const int gw = a.gw, gh = a.gh, ncell = a.ncell, wpr = a.wpr, k = a.k, nword = wpr * gh;
    int *const row = words + t * FFGPU_BLOBS_WORDS;
    int *const rec = reinterpret_cast<int *>(out_recs + t);
    unsigned short *const lab = labels ? labels + (size_t)t * a.label_pitch : nullptr;
    const unsigned char *const sbase = state + (size_t)max(vs, 0) * a.stream_bytes;
    const unsigned frames = vs < 0 ? 0u : *reinterpret_cast<const unsigned *>(sbase);
    if (vs < 0 || frames <= (unsigned)a.warmup) {                                     // an ignored entry, or a model that still learns: nothing (uniform)
        for (int i = tid; i < (int)(sizeof(ffgpu_frame_dets) / sizeof(int)); i += BLOBS_LANES) rec[i] = 0;
        if (lab) for (int i = tid; i < ncell; i += BLOBS_LANES) lab[i] = 0;
        if (tid < FFGPU_BLOBS_WORDS) row[tid] = tid == 6 ? (int)frames : 0;
        return;
    }
    const unsigned *const cell = reinterpret_cast<const unsigned *>(sbase + a.cells_off);

    // 1. the rows' masks; the table and the ranks cleared
    int nactive = 0;
    for (int w0 = wave; w0 < nword; w0 += 8 * (BLOBS_LANES / WAVE)) {                  // (uniform per wave) eight words' loads in flight
        unsigned v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int wi = w0 + u * (BLOBS_LANES / WAVE), y = wi / wpr, x = 64 * (wi - y * wpr) + lane;
            v[u] = wi < nword && x < gw ? cell[(size_t)y * (size_t)gw + x] : 0u;      // (0 is below every min_pixels)
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int wi = w0 + u * (BLOBS_LANES / WAVE);
            const unsigned long long m = __ballot(v[u] >= (unsigned)a.min_pixels);
            if (lane == 0 && wi < nword) { s_mask[wi] = m; nactive += __popcll(m); }
        }
    }
    for (int n = tid; n < ntab; n += BLOBS_LANES) {
        t_cells[n] = 0; t_area[n] = 0; t_pix[n] = 0; t_i0[n] = 0xFFFFu; t_i1[n] = 0; t_j1[n] = 0;
        s_rank[n] = (unsigned short)0xFFFFu;
    }
    nactive = block_fold(nactive, s_red, BLOBS_LANES / WAVE, [](int x, int y) { return x + y; });      // (barriers: the masks are written)

    // 2. the runs' labels.  carry: the run of the word's bit 0 began in an earlier word of the row, at cell `from`
    for (int wi = wave; wi < nword; wi += BLOBS_LANES / WAVE) {
        const int y = wi / wpr, wd = wi - y * wpr, x = 64 * wd + lane;
        const unsigned long long m = s_mask[wi];
        int from = 64 * wd;
        for (int p = wd - 1; p >= 0 && (m & 1ull); p--) {                             // (uniform)
            const unsigned long long z = ~s_mask[wi - wd + p];
            if (z) { from = 64 * p + 64 - __builtin_clzll(z); break; }
            from = 64 * p;
        }
        const unsigned long long below = ~m & ((1ull << lane) - 1ull);                // the inactive cells of the word in front of this one
        const int start = below ? 64 * wd + 64 - __builtin_clzll(below) : from;
        if (x < gw) L[y * gw + x] = (unsigned short)(((m >> lane) & 1ull) ? (unsigned)(y * gw + start) : BLOBS_NONE);
    }
    __syncthreads();

    // 3. union: a lane per run, at the run's first cell
    const int d8 = a.connect == 8;
    for (int wi = wave; wi < nword; wi += BLOBS_LANES / WAVE) {
        const int y = wi / wpr, wd = wi - y * wpr;
        if (y == 0) continue;
        const unsigned long long m = s_mask[wi], prev = wd ? s_mask[wi - 1] >> 63 : 0ull;
        if (!((m & ~((m << 1) | prev)) >> lane & 1ull)) continue;
        const int x0 = 64 * wd + lane;
        int x1 = x0 + blobs_runlen(m, lane) - 1;
        for (int p = wd + 1; p < wpr && x1 == 64 * p - 1; p++) x1 += blobs_runlen(s_mask[wi - wd + p], 0) * (int)(s_mask[wi - wd + p] & 1ull);
        const int xa = max(x0 - d8, 0), xb = min(x1 + d8, gw - 1);
        const unsigned long long *const up = s_mask + (wi - wd - wpr);
        unsigned long long carry = 0;
        for (int p = xa >> 6; p <= xb >> 6; p++) {
            const int lo = p == xa >> 6 ? xa & 63 : 0, hi = p == xb >> 6 ? xb & 63 : 63;
            const unsigned long long bits = up[p] & (~0ull << lo) & (~0ull >> (63 - hi));
            for (unsigned long long first = bits & ~((bits << 1) | carry); first; first &= first - 1ull)      // one cell of every run above in reach
                blobs_unite(L, (unsigned)(y * gw + x0), (unsigned)((y - 1) * gw + 64 * p + __builtin_ctzll(first)));
            carry = bits >> 63;
        }
    }
    __syncthreads();

    // 4. every active cell at its root; the roots numbered in raster order
    for (int c = tid; c < ncell; c += BLOBS_LANES)
        if (L[c] != BLOBS_NONE) L[c] = (unsigned short)blobs_find(L, (unsigned)c);    // (a race of plain stores and loads: every value met is an ancestor)
    __syncthreads();
    int ncomp = 0;
    for (int c0 = 0; c0 < ncell; c0 += BLOBS_LANES) {                                 // (uniform)
        const int c = c0 + tid;
        const bool root = c < ncell && L[c] == c;
        int tot;
        const int n = ncomp + block_rank(root, s_wsum, BLOBS_LANES / WAVE, tot);
        if (root) {
            L[c] = (unsigned short)(BLOBS_ROOT | (unsigned)n);
            if (n < ntab) s_key[n] = (unsigned long long)c;                           // (the root of entry n, until the keys are built)
        }
        ncomp += tot;
        __syncthreads();
    }

    // the table, a lane per run segment: the cells are read a second time for the pixels
    const int c1 = 1 << k;
    for (int wi = wave; wi < nword; wi += BLOBS_LANES / WAVE) {
        const int y = wi / wpr, wd = wi - y * wpr, x = 64 * wd + lane;
        const unsigned long long m = s_mask[wi];
        if (!m) continue;                                                             // (uniform)
        const bool on = (m >> lane) & 1ull;
        const int ch = min(c1 * (y + 1), a.h) - c1 * y;
        unsigned pix = on ? min(cell[(size_t)y * (size_t)gw + x], (unsigned)((min(c1 * (x + 1), a.w) - c1 * x) * ch)) : 0u;
        const unsigned own = pix;
        for (int o = 1; o < WAVE; o <<= 1) { const unsigned up = __shfl_up(pix, o); if (lane >= o) pix += up; }
        const int len = on ? blobs_runlen(m, lane) : 1;
        const unsigned last = __shfl(pix, lane + len - 1);
        if (!((m & ~(m << 1)) >> lane & 1ull)) continue;
        const unsigned n = blobs_number(L, (unsigned)(y * gw + x));
        if (n >= (unsigned)ntab) continue;
        atomicAdd(&t_cells[n], (unsigned)len);
        atomicAdd(&t_area[n], (unsigned)((min(c1 * (x + len), a.w) - c1 * x) * ch));
        atomicAdd(&t_pix[n], last - pix + own);
        atomicMin(&t_i0[n], (unsigned)x);
        atomicMax(&t_i1[n], (unsigned)(x + len - 1));
        atomicMax(&t_j1[n], (unsigned)y);
    }
    __syncthreads();

    // 5. the kept entries in the contract's order
    const int tabled = min(ncomp, ntab);
    int nkept = 0;
    unsigned long long key[FFGPU_BLOBS_COMPONENTS / BLOBS_LANES];
    bool kept[FFGPU_BLOBS_COMPONENTS / BLOBS_LANES];
#pragma unroll
    for (int u = 0; u < FFGPU_BLOBS_COMPONENTS / BLOBS_LANES; u++) {
        const int n = u * BLOBS_LANES + tid;
        kept[u] = n < tabled && t_cells[n] >= (unsigned)a.min_cells && (!a.max_cells || t_cells[n] <= (unsigned)a.max_cells);
        key[u] = kept[u] ? ((unsigned long long)((1u << 27) - t_pix[n]) << 31) | ((unsigned long long)(FFGPU_BLOBS_MAX_CELLS - t_cells[n]) << 15) | s_key[n] : ~0ull;
    }
    __syncthreads();                                                                  // (the roots in s_key are read)
#pragma unroll
    for (int u = 0; u < FFGPU_BLOBS_COMPONENTS / BLOBS_LANES; u++) {
        int tot;
        const int pos = nkept + block_rank(kept[u], s_wsum, BLOBS_LANES / WAVE, tot);
        if (kept[u]) s_key[pos] = key[u];
        nkept += tot;
        __syncthreads();
    }
    int pow2 = 1;
    while (pow2 < nkept) pow2 <<= 1;                                                  // (<= npow2: nkept <= ntab)
    for (int i = nkept + tid; i < pow2; i += BLOBS_LANES) s_key[i] = ~0ull;
    __syncthreads();
    block_bitonic(pow2, [&](int i, int l) { return s_key[i] < s_key[l]; },
                  [&](int i, int l) { const unsigned long long v = s_key[i]; s_key[i] = s_key[l]; s_key[l] = v; });

    const int written = min(nkept, a.max_boxes), untabled = ncomp - tabled;
    if (tid < FFGPU_MAX_DET) {
        BBOX *const o = out_recs[t].box + tid;
        if (tid < written) {
            const unsigned n = L[(unsigned)s_key[tid] & 0x7FFFu] & 0x7FFFu;
            s_rank[n] = (unsigned short)(tid + 1);
            const int i0 = (int)t_i0[n], i1 = (int)t_i1[n], j0 = (int)((unsigned)s_key[tid] & 0x7FFFu) / gw, j1 = (int)t_j1[n];
            const unsigned q = min(256u, (unsigned)((unsigned long long)t_pix[n] * 256ull / t_area[n]));
            o->type = a.type;
            o->score = (float)q * 0.00390625f;
            o->x1 = (float)max(c1 * i0 - a.pad, 0);
            o->y1 = (float)max(c1 * j0 - a.pad, 0);
            o->x2 = (float)min(min(c1 * (i1 + 1), a.w) - 1 + a.pad, a.w - 1);
            o->y2 = (float)min(min(c1 * (j1 + 1), a.h) - 1 + a.pad, a.h - 1);
        } else track_zero(o);
    }
    if (tid < 4) rec[tid] = tid == 1 ? nkept : tid == 2 ? (int)(nkept > written || untabled > 0) : written;      // count, ncand, overflow, nfull
    if (tid < FFGPU_BLOBS_WORDS)
        row[tid] = tid == 0 ? nactive : tid == 1 ? ncomp : tid == 2 ? nkept : tid == 3 ? written : tid == 4 ? untabled : tid == 5 ? 1 : tid == 6 ? (int)frames : 0;
    if (!lab) return;
    __syncthreads();
    for (int c = tid; c < ncell; c += BLOBS_LANES) {
        unsigned v = 0;
        if (L[c] != BLOBS_NONE) { const unsigned n = blobs_number(L, (unsigned)c); v = n < (unsigned)ntab ? s_rank[n] : 0xFFFFu; }
        lab[c] = (unsigned short)v;
    }
}

// ---- host side
extern "C" int ffgpu_blobs_spec_check(const ffgpu_blobs_spec *spec)
{
    BlobsPlan pl;
    return ffgpu_blobs_spec_plan("blobs_spec_check", spec, pl);
}

extern "C" int ffgpu_blobs_dev(const int *streams, int ntargets, const ffgpu_blobs_spec *spec, const void *d_state, int nstreams, void *d_words, void *d_out_records,
                               void *d_labels, void *stream)
{
    const char *const what = "blobs_dev";
    if (ffgpu_no_device(what)) return -1;
    BlobsPlan pl;
    if (ffgpu_blobs_args_check(what, streams, ntargets, spec, d_state, nstreams, d_words, d_out_records, pl)) return -1;
    if (lds_allow((const void *)k_blobs, pl.lds, "blobs")) return -1;
    BlobsArgs a;
    memset(&a, 0, sizeof a);
    a.w = pl.lay.w; a.h = pl.lay.h; a.k = pl.lay.cell_log2; a.gw = pl.lay.gw; a.gh = pl.lay.gh; a.wpr = pl.wpr; a.ncell = pl.ncell; a.ntab = pl.ntab; a.npow2 = pl.npow2;
    a.min_pixels = pl.min_pixels; a.warmup = pl.warmup; a.connect = pl.connect; a.min_cells = pl.min_cells; a.max_cells = pl.max_cells; a.max_boxes = pl.max_boxes;
    a.pad = pl.pad; a.type = pl.type; a.mask_off = pl.mask_off; a.tab_off = pl.tab_off; a.key_off = pl.key_off; a.rank_off = pl.rank_off;
    a.cells_off = pl.lay.cells_off; a.stream_bytes = pl.lay.stream_bytes; a.label_pitch = pl.label_pitch;
    for (int t0 = 0; t0 < ntargets; t0 += BLOBS_ARG_TARGETS) {
        const int nt = std::min(BLOBS_ARG_TARGETS, ntargets - t0);
        for (int i = 0; i < BLOBS_ARG_TARGETS; i++) a.stream[i] = i < nt ? streams[t0 + i] : -1;
        hipLaunchKernelGGL(k_blobs, dim3((unsigned)nt), dim3(BLOBS_LANES), pl.lds, (hipStream_t)stream, a, (const unsigned char *)d_state, t0, (int *)d_words,
                           (ffgpu_frame_dets *)d_out_records, (unsigned short *)d_labels);
        LAUNCH_OK("blobs");
    }
    return 0;
}
