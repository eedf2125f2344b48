// ffgpu_merge.inc -- tiled detection: the boxes of the tiles of one picture merged on the device (ffgpu_merge_tiles_dev, ffgpu_exec_merge_tiles).
// A batch entry may be a tile of a larger picture (a frame descriptor is an address, a size and a pitch: a crop costs nothing); its survivors
// are in the tile's own pixels.  Per picture: translate every tile's survivors by the tile's origin (one fp32 addition per coordinate), order
// the union by (score desc, position of the tile in the caller's table asc, index in the tile's list asc), run the greedy class-aware
// suppression of ffcnn.c:298-322 with k_nms's arithmetic (block_suppress, ffgpu_block.inc), write the survivors in that order.  Two-stage NMS: per tile by k_nms, across tiles
// here -- not NMS over the union of the raw candidates.
//
// The tile table as the kernel reads it, ints: [0] nimages | off[nimages + 1] | { t, x0, y0 } per selected table entry, the entries of picture g
// at triples off[g] .. off[g + 1] in table order (a CSR built on the host; entries with image == -1 are in no row).  It reaches the device as a
// by-value kernel argument: of the merge launch itself when it fits (MergeTabArg, the operator), or of k_set_ints in front of it (the executor,
// which skips that launch while the table is unchanged; the operator for tables beyond MERGE_ARG_INTS, into the head of its scratch buffer).
#define MERGE_ARG_INTS 896
struct MergeTabPtr { const int *p; __device__ __forceinline__ int at(int i) const { return p[i]; } };
struct MergeTabArg { int v[MERGE_ARG_INTS]; __device__ __forceinline__ int at(int i) const { return v[i]; } };
struct IntsChunk { int v[MERGE_ARG_INTS]; int n; };
static_assert(sizeof(IntsChunk) + sizeof(int *) <= 4096 - 256 && sizeof(MergeTabArg) + 96 <= 4096 - 256, "the table travels as a kernel argument (4 KB at most, the hidden arguments included)");
__global__ void k_set_ints(int *dst, IntsChunk c)
{
    for (int i = threadIdx.x; i < c.n; i += blockDim.x) dst[i] = c.v[i];
}

// Work arrays of one picture, MERGE_SLOT_BYTES per slot: score (the survivors' list once the sort is done), index, the translated box, alive.  In LDS
// when the picture's union has at most FFGPU_MERGE_LDS_SLOTS boxes (the normal case: tens), else in the picture's own region of the global
// scratch buffer: 2 x list_stride slots per tile of the picture (>= the next power of two of any union it can have), regions in picture order.
#define MERGE_SLOT_BYTES 36
struct MergeWork {
    float *score; int *idx; BBOX *box; int *alive;
    __device__ __forceinline__ MergeWork(unsigned char *b, size_t cap)
        : score(reinterpret_cast<float *>(b)), idx(reinterpret_cast<int *>(b + 4 * cap)), box(reinterpret_cast<BBOX *>(b + 8 * cap)), alive(reinterpret_cast<int *>(b + 32 * cap)) {}
};

// sort, suppress, write: steps 2 - 4 of the contract on the m gathered boxes of picture g, with the primitives of ffgpu_block.inc that k_nms uses (the
// gather slot is the tie-breaking key: slots are filled tile by tile in table order).  Unlike k_nms, a box of score 0 starts alive.
__device__ __forceinline__ void merge_sorted_out(MergeWork w, int m, float thresh, int use_min, int ncand, int ovf0,
                                                 ffgpu_frame_dets *out, BBOX *out_list)
{
    const int tid = threadIdx.x;
    int pow2 = 1;
    while (pow2 < m) pow2 <<= 1;
    for (int i = m + tid; i < pow2; i += blockDim.x) { w.score[i] = -1.f; w.idx[i] = 0x7fffffff; }
    __syncthreads();
    block_bitonic(pow2, [&](int i, int l) { return w.score[i] > w.score[l] || (w.score[i] == w.score[l] && w.idx[i] < w.idx[l]); },
                  [&](int i, int l) {
                      const float ts = w.score[i]; w.score[i] = w.score[l]; w.score[l] = ts;
                      const int ti = w.idx[i]; w.idx[i] = w.idx[l]; w.idx[l] = ti;
                  });
    for (int i = tid; i < m; i += blockDim.x) w.alive[i] = 1;
    __syncthreads();
    block_suppress(m, w.alive, [&](int i) { return w.box[w.idx[i]]; }, thresh, use_min);
    // survivors in order (the score array has served its purpose and becomes the list), every thread then writes slots
    int *const keep = reinterpret_cast<int *>(w.score);
    const int nfull = block_compact(m, w.alive, w.idx, keep), nrec = min(nfull, FFGPU_MAX_DET);
    if (out_list) for (int i = tid; i < nfull; i += blockDim.x) out_list[i] = w.box[keep[i]];
    for (int i = tid; i < FFGPU_MAX_DET; i += blockDim.x) {
        BBOX r = { 0, 0.f, 0.f, 0.f, 0.f, 0.f };
        if (i < nrec) r = w.box[keep[i]];
        out->box[i] = r;                                  // (the caller's buffer may hold anything: every slot is written)
    }
    if (tid == 0) {
        out->count = nrec; out->ncand = ncand; out->nfull = nfull;
        out->overflow = (ovf0 ? 1 : 0) | (nfull > FFGPU_MAX_DET ? 4 : 0);
    }
}

// One workgroup per picture.  lists == NULL: a tile's boxes are its record's own box[0 .. count), stride == FFGPU_MAX_DET; else list t holds
// the tile's nfull boxes at lists + t * stride.  Counts are clamped to [0, stride]: whatever the records hold, nothing is read or written
// outside the buffers the host has sized.
template <class Tab>
__global__ void __launch_bounds__(256) k_merge_tiles(Tab tab, const ffgpu_frame_dets *recs, const BBOX *lists, int stride, float thresh, int use_min,
                                                     ffgpu_frame_dets *out_recs, BBOX *out_lists, unsigned char *scratch)
{
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) unsigned char s_work[MERGE_SLOT_BYTES * FFGPU_MERGE_LDS_SLOTS];
    __shared__ int s_cnt[256], s_start[256], s_t[256], s_x0[256], s_y0[256], s_wsum[4], s_red[3];
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nimages = tab.at(0), o0 = tab.at(1 + g), ng = tab.at(2 + g) - o0, trip = 2 + nimages + 3 * o0;      // trip: this picture's first triple
    auto count_of = [&](int t) { return max(0, min(lists ? recs[t].nfull : recs[t].count, stride)); };
    // the union's size (LDS or scratch?), the candidate sum and the overflow bit
    if (tid < 3) s_red[tid] = 0;
    __syncthreads();
    {
        int m_ = 0, nc_ = 0, ov_ = 0;
        for (int j = tid; j < ng; j += blockDim.x) {
            const int t = tab.at(trip + 3 * j);
            m_ += count_of(t); nc_ += recs[t].ncand; ov_ |= recs[t].overflow & 1;
        }
        if (m_) atomicAdd(&s_red[0], m_);
        if (nc_) atomicAdd(&s_red[1], nc_);
        if (ov_) atomicOr(&s_red[2], 1);
    }
    __syncthreads();
    const int m = s_red[0], ncand = s_red[1], ovf0 = s_red[2];
    const bool glb = m > FFGPU_MERGE_LDS_SLOTS;                                       // uniform
    const size_t cap = glb ? (size_t)2 * stride * ng : FFGPU_MERGE_LDS_SLOTS;
    const MergeWork w(glb ? scratch + (size_t)MERGE_SLOT_BYTES * 2 * stride * o0 : s_work, cap);
    // gather: 256 tiles at a time -- their counts scanned into first slots, then every thread takes slots and finds each one's tile by bisection
    int base = 0;
    for (int c0 = 0; c0 < ng; c0 += 256) {
        const int nn = min(256, ng - c0);
        int v = 0;
        if (tid < nn) {
            const int t = tab.at(trip + 3 * (c0 + tid));
            v = count_of(t);
            s_t[tid] = t; s_x0[tid] = tab.at(trip + 3 * (c0 + tid) + 1); s_y0[tid] = tab.at(trip + 3 * (c0 + tid) + 2); s_cnt[tid] = v;
        }
        int incl = v;
        for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(incl, o); if (lane >= o) incl += u; }
        if (lane == 63) s_wsum[wave] = incl;
        __syncthreads();
        int woff = 0;
        for (int k = 0; k < wave; k++) woff += s_wsum[k];
        s_start[tid] = base + woff + incl - v;
        const int chunk = s_wsum[0] + s_wsum[1] + s_wsum[2] + s_wsum[3];
        __syncthreads();
        for (int i = base + tid; i < base + chunk; i += blockDim.x) {
            int lo = 0, hi = nn - 1;                                                  // the last tile whose first slot is <= i (empty tiles share their successor's)
            while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (s_start[mid] <= i) lo = mid; else hi = mid - 1; }
            const int t = s_t[lo], k = i - s_start[lo];
            BBOX b = lists ? lists[(size_t)t * stride + k] : recs[t].box[k];
            const float fx = (float)s_x0[lo], fy = (float)s_y0[lo];
            b.x1 += fx; b.x2 += fx; b.y1 += fy; b.y2 += fy;
            w.box[i] = b; w.score[i] = b.score; w.idx[i] = i;
        }
        base += chunk;
        __syncthreads();                                                              // (the chunk's tables are rewritten by the next trip)
    }
    BBOX *const ol = out_lists ? out_lists + (size_t)stride * o0 : nullptr;
    merge_sorted_out(w, m, thresh, use_min, ncand, ovf0, out_recs + g, ol);
}

int ffgpu_launch_set_ints(int *d_dst, const int *h_src, int n, hipStream_t s)
{
    for (int i0 = 0; i0 < n; i0 += MERGE_ARG_INTS) {
        IntsChunk c;
        memset(&c, 0, sizeof c);
        c.n = std::min(MERGE_ARG_INTS, n - i0);
        memcpy(c.v, h_src + i0, sizeof(int) * c.n);
        hipLaunchKernelGGL(k_set_ints, dim3(1), dim3(256), 0, s, d_dst + i0, c);
        LAUNCH_OK("set_ints");
    }
    return 0;
}

size_t ffgpu_merge_tab_bytes(int ntiles) { return (((size_t)4 * ntiles + 2) * sizeof(int) + 15) & ~(size_t)15; }

// The caller's table -> the CSR above (2 + nimages + 3 x selected ints); off (may be NULL) receives off[0 .. nimages].  Every entry is checked
// here, once, for both entry points; -1 with the entry's index in the message.
int ffgpu_merge_build_tab(const char *what, const ffgpu_tile *tiles, int ntiles, int nimages, std::vector<int> &tab, std::vector<int> *off)
{
    if (!tiles) { ffgpu_set_error("%s: NULL tile table", what); return -1; }
    if (ntiles < 1 || nimages < 1 || nimages > ntiles) { ffgpu_set_error("%s: %d pictures for %d tiles (1 <= nimages <= ntiles)", what, nimages, ntiles); return -1; }
    if (ntiles > (1 << 24)) { ffgpu_set_error("%s: %d tiles is too many", what, ntiles); return -1; }
    tab.assign((size_t)2 + nimages, 0);
    tab[0] = nimages;
    for (int t = 0; t < ntiles; t++) {
        const ffgpu_tile &e = tiles[t];
        if (e.image < -1 || e.image >= nimages) { ffgpu_set_error("%s: tile %d: image %d is outside -1 .. %d", what, t, e.image, nimages - 1); return -1; }
        if (e.x0 < 0 || e.y0 < 0) { ffgpu_set_error("%s: tile %d: negative origin (%d, %d)", what, t, e.x0, e.y0); return -1; }
        if (e.reserved != 0) { ffgpu_set_error("%s: tile %d: reserved must be 0", what, t); return -1; }
        if (e.image >= 0) tab[(size_t)2 + e.image]++;                                 // counts, one place to the right: the scan below makes them offsets
    }
    for (int g = 0, run = 0; g < nimages; g++) { const int c = tab[(size_t)2 + g]; tab[(size_t)1 + g] = run; run += c; tab[(size_t)2 + g] = run; }
    const int nsel = tab[(size_t)1 + nimages];
    std::vector<int> fill(tab.begin() + 1, tab.begin() + 1 + nimages);
    tab.resize((size_t)2 + nimages + (size_t)3 * nsel);
    for (int t = 0; t < ntiles; t++) {
        const ffgpu_tile &e = tiles[t];
        if (e.image < 0) continue;
        int *trip = &tab[(size_t)2 + nimages + (size_t)3 * fill[e.image]++];
        trip[0] = t; trip[1] = e.x0; trip[2] = e.y0;
    }
    if (off) off->assign(tab.begin() + 1, tab.begin() + 2 + nimages);
    return 0;
}

// d_tab: the table on the device (in stream order), or NULL: `tab` travels with this launch (at most MERGE_ARG_INTS ints)
int ffgpu_launch_merge_tiles(const int *d_tab, const std::vector<int> &tab, const ffgpu_frame_dets *recs, const BBOX *lists, int stride,
                             float thresh, int use_min, ffgpu_frame_dets *out_recs, BBOX *out_lists, void *scratch, hipStream_t s)
{
    const int nimages = tab[0];
    if (d_tab) {
        MergeTabPtr t; t.p = d_tab;
        hipLaunchKernelGGL(k_merge_tiles<MergeTabPtr>, dim3(nimages), dim3(256), 0, s, t, recs, lists, stride, thresh, use_min, out_recs, out_lists, (unsigned char *)scratch);
    } else {
        if (tab.size() > MERGE_ARG_INTS) { ffgpu_set_error("merge_tiles: a table of %zu ints does not fit a kernel argument", tab.size()); return -1; }
        MergeTabArg t;
        memset(&t, 0, sizeof t);
        memcpy(t.v, tab.data(), sizeof(int) * tab.size());
        hipLaunchKernelGGL(k_merge_tiles<MergeTabArg>, dim3(nimages), dim3(256), 0, s, t, recs, lists, stride, thresh, use_min, out_recs, out_lists, (unsigned char *)scratch);
    }
    LAUNCH_OK("merge_tiles");
    return 0;
}

extern "C" size_t ffgpu_merge_tiles_scratch_bytes(int ntiles, int list_stride)
{
    if (ntiles < 1 || list_stride < 1) return 0;
    return ffgpu_merge_tab_bytes(ntiles) + (size_t)MERGE_SLOT_BYTES * 2 * (size_t)list_stride * (size_t)ntiles;
}

extern "C" int ffgpu_merge_tiles_dev(const void *d_records, const void *d_lists, int list_stride, const ffgpu_tile *tiles, int ntiles, int nimages,
                                     float thresh, int use_min, void *d_out_records, void *d_out_lists, void *d_scratch, size_t scratch_bytes, void *stream)
{
    if (ffgpu_no_device("merge_tiles_dev")) return -1;
    if (!d_records || !d_out_records) { ffgpu_set_error("merge_tiles_dev: NULL records"); return -1; }
    const int stride = ffgpu_list_stride("merge_tiles_dev", d_lists, list_stride);
    if (stride < 0) return -1;
    std::vector<int> tab, off;
    if (ffgpu_merge_build_tab("merge_tiles_dev", tiles, ntiles, nimages, tab, &off)) return -1;
    // the scratch buffer is needed when a picture's union CAN exceed the LDS slots (the kernel then uses it for the pictures whose union does),
    // and for a table too long for a kernel argument
    int most = 0;
    for (int g = 0; g < nimages; g++) most = std::max(most, off[g + 1] - off[g]);
    const bool need_work = (long)most * stride > FFGPU_MERGE_LDS_SLOTS, need_tab = tab.size() > MERGE_ARG_INTS;
    if (need_work || need_tab) {
        const size_t need = ffgpu_merge_tiles_scratch_bytes(ntiles, stride);
        if (!d_scratch || scratch_bytes < need) {
            if (need_work) ffgpu_set_error("merge_tiles_dev: a picture of %d tiles x %d boxes can exceed the %d LDS slots: a scratch buffer of ffgpu_merge_tiles_scratch_bytes() = %zu bytes is needed (given: %zu)",
                                           most, stride, FFGPU_MERGE_LDS_SLOTS, need, d_scratch ? scratch_bytes : (size_t)0);
            else ffgpu_set_error("merge_tiles_dev: a table of %d tiles needs a scratch buffer of ffgpu_merge_tiles_scratch_bytes() = %zu bytes (given: %zu)", ntiles, need, d_scratch ? scratch_bytes : (size_t)0);
            return -1;
        }
        if (reinterpret_cast<uintptr_t>(d_scratch) & 15) { ffgpu_set_error("merge_tiles_dev: the scratch buffer must be 16-byte aligned"); return -1; }
    }
    const hipStream_t s = (hipStream_t)stream;
    int *d_tab = nullptr;
    if (need_tab) {
        d_tab = reinterpret_cast<int *>(d_scratch);
        if (ffgpu_launch_set_ints(d_tab, tab.data(), (int)tab.size(), s)) return -1;
    }
    unsigned char *work = d_scratch ? (unsigned char *)d_scratch + ffgpu_merge_tab_bytes(ntiles) : nullptr;
    return ffgpu_launch_merge_tiles(d_tab, tab, (const ffgpu_frame_dets *)d_records, (const BBOX *)d_lists, stride, thresh, use_min,
                                    (ffgpu_frame_dets *)d_out_records, (BBOX *)d_out_lists, need_work ? work : nullptr, s);
}
