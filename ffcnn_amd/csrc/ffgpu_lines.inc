// ffgpu_lines.inc -- outlines: segments rasterised into the frames on the device, and the composer that writes them from the zones' scenes, events and
// state (ffgpu_draw_segments_bgr_dev / _nv12_dev, ffgpu_outline_scene_dev, ffgpu_outline_spec_check).  The contract is in include/ffcnn_hip.h; the
// host side (spec and argument checks) is ffgpu_lines_host.hpp.
//
// The rasteriser follows k_draw_text: items run in parallel, so the LAST WRITER of every byte is computed instead of raced for.  An item's pixel set is
// a closed form (seg_hit: two 64-bit products and four compares), so the lane that owns pixel P of item k stores it only if no item j > k of the
// target contains P, and the chroma pair only if no later item contains any luma pixel of the sample.  Every byte is stored with one value per launch,
// whichever lanes store it.  A target's items are staged in LDS in canonical form (S, D, g: 8 KB at 512, with colour and thickness 12 KB) beside one
// clipped bounding box each (8 KB), thickness included and empty for an item that draws nothing: a later item is dismissed by four compares -- once
// per item against the item's own box (the survivors are the item's candidates, 10 KB), then per pixel among the candidates.  An
// item's major range is clipped to the target before the lanes stride over it, so a segment from -2^20 to 2^20 costs what its visible part costs.  A
// lane owns a major step: one column (an fp64 estimate of the quotient, corrected by the inequality), then its T pixels.  Byte stores and one aligned
// 2-byte store per (U, V) pair.
#define SEG_GROUPS 16             // workgroups per target: workgroup g draws items g, g + 16, ...
struct SegArgs {
    DrawTarget t[SEG_ARG_TARGETS];
    int t0, stride, pad_[2];      // target blockIdx.y of the launch is target t0 + blockIdx.y of the call; items_stride
};
static_assert(sizeof(SegArgs) + 1 * 8 <= 4096 - 256, "the tables travel as a kernel argument (4 KB at most, the hidden arguments included)");
static_assert(FFGPU_SEG_ITEMS == 512 && FFGPU_SEG_LIMIT == (1 << 20) && offsetof(ffgpu_seg_item, color) == 16 && offsetof(ffgpu_seg_item, thickness) == 20 &&
              offsetof(ffgpu_seg_item, dash) == 21, "k_draw_segments: a lane stages an item's geometry; the layout of include/ffcnn_hip.h");

struct SegLds {
    int4     geo[FFGPU_SEG_ITEMS];                    // item j in canonical form: S's major and minor coordinate, D, g
    int4     box[FFGPU_SEG_ITEMS];                    // the pixels it can write inside the target: x from .x to .z, y from .y to .w; empty: .x > .z
    unsigned aux[FFGPU_SEG_ITEMS];                    // T | d << 8 | y-major << 16
    unsigned col[FFGPU_SEG_ITEMS];
    int4     cbox[FFGPU_SEG_ITEMS];                   // the item being drawn: the boxes of the later items that meet its own, in slot order
    int      cidx[FFGPU_SEG_ITEMS];                   //                       and their slots
    int      wmax[4], wsum[4];
};

// pixel (px, py) belongs to item (g, aux): the contract's inequality, word for word.  |coordinates| <= 2^20 and 0 <= px, py < 2^31: every product is
// below 2^55.
__device__ __forceinline__ bool seg_hit(const int4 g, unsigned aux, int px, int py)
{
    const int T = (int)(aux & 0xffu), d = (int)((aux >> 8) & 0xffu);
    const bool ym = (aux >> 16) & 1u;
    const long long m = (long long)(ym ? py : px) - g.x, r = (long long)(ym ? px : py) - g.y, D = g.z;
    if (m < 0 || m > D) return false;
    if (d && ((m >> d) & 1)) return false;
    const long long lo = (T - 1) >> 1, hi = T >> 1;
    if (D == 0) return -lo <= r && r <= hi;
    const long long e = 2 * m * g.w + D;
    return 2 * D * (r - hi) <= e && e < 2 * D * (r + lo + 1);
}

// floor((2 m g + D) / (2 D)), D > 0: |2 m g + D| < 2^44 is exact in fp64 and the quotient's estimate is off by one at most; the inequality decides
__device__ __forceinline__ long long seg_column(long long m, long long D, long long g)
{
    const long long e = 2 * m * g + D, dd = 2 * D;
    long long q = (long long)floor((double)e / (double)dd);
    while (q * dd > e) q--;
    while ((q + 1) * dd <= e) q++;
    return q;
}

// grid (SEG_GROUPS, targets of this launch), 256 lanes.  Whatever the items hold, nothing is read outside them, and every store lies inside the
// target's w x h.
template <bool NV12>
__global__ void __launch_bounds__(256) k_draw_segments(SegArgs a, const unsigned *items)
{
    __shared__ __attribute__((aligned(16))) unsigned char s_seg[sizeof(SegLds)];
    SegLds &L = *reinterpret_cast<SegLds *>(s_seg);
    const DrawTarget &t = a.t[blockIdx.y];
    if (!t.p0) return;                                                                // a skipped target (uniform)
    const int tid = threadIdx.x, stride = a.stride, w = t.w, h = t.h;
    const unsigned *src = items + ((size_t)a.t0 + blockIdx.y) * (size_t)stride * 8u;
    int last = 0;                                                                     // behind the last of this lane's items that draws anything
    for (int j = tid; j < stride; j += blockDim.x) {
        const long long x0 = (int)src[j * 8], y0 = (int)src[j * 8 + 1], x1 = (int)src[j * 8 + 2], y1 = (int)src[j * 8 + 3];
        const unsigned m5 = src[j * 8 + 5];
        const int T = min((int)(m5 & 0xffu), 8), d = min((int)((m5 >> 8) & 0xffu), 6);
        const long long lim = FFGPU_SEG_LIMIT;
        const bool ok = T > 0 && x0 >= -lim && x0 <= lim && y0 >= -lim && y0 <= lim && x1 >= -lim && x1 <= lim && y1 >= -lim && y1 <= lim;
        int4 geo = make_int4(0, 0, 0, 0), box = make_int4(1, 1, 0, 0);
        unsigned aux = 0;
        if (ok) {
            const long long dx = x1 - x0, dy = y1 - y0;
            const bool ym = (dx < 0 ? -dx : dx) < (dy < 0 ? -dy : dy);
            long long a0 = ym ? y0 : x0, b0 = ym ? x0 : y0, a1 = ym ? y1 : x1, b1 = ym ? x1 : y1;
            if (a1 < a0) { const long long ta = a0, tb = b0; a0 = a1; b0 = b1; a1 = ta; b1 = tb; }
            const long long D = a1 - a0, g = b1 - b0, Wm = ym ? h : w, Wn = ym ? w : h, lo = (T - 1) >> 1, hi = T >> 1;
            geo = make_int4((int)a0, (int)b0, (int)D, (int)g);
            aux = (unsigned)T | (unsigned)d << 8 | (ym ? 1u << 16 : 0u);
            const long long mlo = max(0LL, -a0), mhi = min(D, Wm - 1 - a0);              // the major steps inside the target
            if (mlo <= mhi) {
                const long long c0 = D ? seg_column(mlo, D, g) : 0, c1 = D ? seg_column(mhi, D, g) : 0;      // (the column is monotone in m)
                const long long nlo = max(b0 + min(c0, c1) - lo, 0LL), nhi = min(b0 + max(c0, c1) + hi, Wn - 1);
                if (nlo <= nhi) {
                    box = ym ? make_int4((int)nlo, (int)(a0 + mlo), (int)nhi, (int)(a0 + mhi)) : make_int4((int)(a0 + mlo), (int)nlo, (int)(a0 + mhi), (int)nhi);
                    last = j + 1;
                }
            }
        }
        L.geo[j] = geo; L.box[j] = box; L.aux[j] = aux; L.col[j] = src[j * 8 + 4];
    }
    last = wave_max(last);
    if ((tid & (WAVE - 1)) == 0) L.wmax[tid / WAVE] = last;
    __syncthreads();
    const int n = max(max(L.wmax[0], L.wmax[1]), max(L.wmax[2], L.wmax[3]));          // behind the last item that draws anything
    for (int k = blockIdx.x; k < n; k += gridDim.x) {
        const int4 bx = L.box[k];
        if (bx.x > bx.z) continue;                                                    // draws nothing, or clipped away
        const int4 g = L.geo[k];
        const unsigned aux = L.aux[k], col = L.col[k];
        const int T = (int)(aux & 0xffu), d = (int)((aux >> 8) & 0xffu), lo = (T - 1) >> 1, hi = T >> 1;
        const bool ym = (aux >> 16) & 1u;
        const int M0 = ym ? bx.y : bx.x, M1 = ym ? bx.w : bx.z, Wn = ym ? w : h;
        // the candidates: only a later item whose box meets this item's (NV12: widened to whole chroma samples) can own one of its pixels or samples.
        // Found by all lanes at once, compacted by ranks; the pixels then ask the candidates alone.  (k, n and the box are uniform: so are the barriers)
        const int bxl = NV12 ? bx.x & ~1 : bx.x, bxh = NV12 ? bx.z | 1 : bx.z, byl = NV12 ? bx.y & ~1 : bx.y, byh = NV12 ? bx.w | 1 : bx.w;
        int nc = 0;
        __syncthreads();                                                              // (the previous item's candidates are read no more)
        for (int j0 = k + 1; j0 < n; j0 += blockDim.x) {
            const int j = j0 + tid;
            int4 q = make_int4(1, 1, 0, 0);
            if (j < n) q = L.box[j];
            const bool meets = !(bxh < q.x || bxl > q.z || byh < q.y || byl > q.w || q.x > q.z);
            int tot;
            const int r = nc + block_rank(meets, L.wsum, 4, tot);
            if (meets) { L.cbox[r] = q; L.cidx[r] = j; }
            nc += tot;
            __syncthreads();
        }
        for (int M = M0 + tid; M <= M1; M += blockDim.x) {
            const long long m = (long long)M - g.x;
            if (d && ((m >> d) & 1)) continue;
            const long long c = g.y + (g.z ? seg_column(m, g.z, g.w) : 0);
            for (int o = -lo; o <= hi; o++) {
                const long long N = c + o;
                if (N < 0 || N >= Wn) continue;
                const int x = ym ? (int)N : M, y = ym ? M : (int)N;
                // the last writer: a later item that contains this pixel owns it (and, NV12, its chroma sample); a later item on another luma pixel
                // of the sample owns the sample alone
                const int x1 = x ^ 1, y1 = y ^ 1, xl = NV12 ? x & ~1 : x, xh = NV12 ? x | 1 : x, yl = NV12 ? y & ~1 : y, yh = NV12 ? y | 1 : y;
                bool later = false, later_uv = false;
                for (int ci = 0; ci < nc; ci++) {
                    const int4 q = L.cbox[ci];
                    if (xh < q.x || xl > q.z || yh < q.y || yl > q.w) continue;
                    const int j = L.cidx[ci];
                    const int4 gj = L.geo[j];
                    const unsigned aj = L.aux[j];
                    if (seg_hit(gj, aj, x, y)) { later = true; break; }
                    if (NV12 && !later_uv)
                        later_uv = (x1 < w && seg_hit(gj, aj, x1, y)) || (y1 < h && (seg_hit(gj, aj, x, y1) || (x1 < w && seg_hit(gj, aj, x1, y1))));
                }
                if (later) continue;
                if (NV12) {
                    t.p0[(size_t)y * (size_t)t.pitch + (size_t)x] = (unsigned char)col;
                    if (!later_uv)
                        *reinterpret_cast<unsigned short *>(t.p1 + (size_t)(y >> 1) * (size_t)t.pitch_uv + 2 * (size_t)(x >> 1)) = (unsigned short)(col >> 8);
                } else {
                    unsigned char *px = t.p0 + (size_t)y * (size_t)t.pitch + 3 * (size_t)x;
                    px[0] = (unsigned char)col; px[1] = (unsigned char)(col >> 8); px[2] = (unsigned char)(col >> 16);
                }
            }
        }
    }
}

// ---- the scene composer.  An item is composed by one lane in its 32 bytes of LDS and leaves the workgroup as words.
struct OutlineArgs {
    int      stream[OUTLINE_ARG_TARGETS];             // target blockIdx.x of the launch: its video stream, or -1
    unsigned pal[256];
    int      npal, flags, thickness, line_dash, marker, t0, items_stride, capacity, events_stride;
    unsigned alarm;
    int      pad_[2];
};
static_assert(sizeof(OutlineArgs) + 4 * 8 <= 4096 - 256, "the tables travel as a kernel argument (4 KB at most, the hidden arguments included)");
static_assert(FFGPU_SCENE_ZONES == 8 && FFGPU_ZONE_VERTS == 8 && FFGPU_SCENE_LINES == 8 && FFGPU_OUTLINE_FIXED == 80 && FFGPU_ZONES_DETS <= 256 &&
              CAPTION_STATE_HEADER == ZONES_STATE_HEADER, "k_outline_scene: lanes 0..63 the zones' edges, 64..79 the lines' shafts and ticks; a lane owns a slot of the state");

__device__ __forceinline__ int seg_sat(long long v) { return (int)min(max(v, -2147483648LL), 2147483647LL); }
__device__ __forceinline__ void seg_put(unsigned *row, long long x0, long long y0, long long x1, long long y1, unsigned col, int T, int d)
{
    row[0] = (unsigned)seg_sat(x0); row[1] = (unsigned)seg_sat(y0); row[2] = (unsigned)seg_sat(x1); row[3] = (unsigned)seg_sat(y1);
    row[4] = col; row[5] = (unsigned)T | (unsigned)d << 8;
}

// grid = targets of the launch, 256 lanes: lanes 0..79 compose the fixed slots, lanes 0..capacity - 1 the markers, all copy.  Total over any scene and
// state bytes, as k_zones.
__global__ void __launch_bounds__(256) k_outline_scene(OutlineArgs a, const unsigned char *scenes, const unsigned char *state, const unsigned *events, unsigned *items)
{
    __shared__ unsigned s_row[FFGPU_SEG_ITEMS * 8];
    __shared__ int s_wsum[4];
    const int tid = threadIdx.x, nwords = a.items_stride * 8, vs = a.stream[blockIdx.x];
    const size_t T = (size_t)a.t0 + blockIdx.x;
    for (int i = tid; i < nwords; i += blockDim.x) s_row[i] = 0;
    __syncthreads();
    if (vs >= 0) {                                                                    // (uniform)
        const ffgpu_scene &S = *reinterpret_cast<const ffgpu_scene *>(scenes + (size_t)vs * sizeof(ffgpu_scene));
        if (tid < FFGPU_SCENE_ZONES * FFGPU_ZONE_VERTS) {
            const int z = tid >> 3, i = tid & 7;
            const ffgpu_zone &zn = S.zone[z];
            const int nv = zn.nverts;
            bool ok = (a.flags & FFGPU_OUTLINE_ZONES) && z < max(0, min(S.nzones, FFGPU_SCENE_ZONES)) && nv >= 3 && nv <= FFGPU_ZONE_VERTS && i < nv;
            for (int v = 0; ok && v < nv; v++) ok = zn.x[v] == zn.x[v] && zn.y[v] == zn.y[v];
            if (ok) {
                const int j = i + 1 == nv ? 0 : i + 1;
                const bool alarm = (a.flags & FFGPU_OUTLINE_ALARM) && events[T * (size_t)a.events_stride + 19u + 4u * (unsigned)z] != 0;
                seg_put(s_row + tid * 8, draw_f2i(zn.x[i]), draw_f2i(zn.y[i]), draw_f2i(zn.x[j]), draw_f2i(zn.y[j]),
                        alarm ? a.alarm : a.pal[draw_colour_index(z, a.npal)], a.thickness, 0);
            }
        } else if (tid < FFGPU_OUTLINE_FIXED) {
            const int l = (tid - 64) >> 1;
            const bool tick = tid & 1;
            if ((a.flags & (tick ? FFGPU_OUTLINE_TICKS : FFGPU_OUTLINE_LINES)) && l < max(0, min(S.nlines, FFGPU_SCENE_LINES))) {
                const ffgpu_line &ln = S.line[l];
                const long long ax = draw_f2i(ln.ax), ay = draw_f2i(ln.ay), bx = draw_f2i(ln.bx), by = draw_f2i(ln.by);
                const unsigned col = a.pal[draw_colour_index(8 + l, a.npal)];
                if (tick) {
                    const long long mx = (ax + bx) >> 1, my = (ay + by) >> 1;
                    seg_put(s_row + tid * 8, mx, my, mx + (-(by - ay)) / 8, my + (bx - ax) / 8, col, 1, 0);
                } else seg_put(s_row + tid * 8, ax, ay, bx, by, col, a.thickness, a.line_dash);
            }
        }
        if (a.flags & FFGPU_OUTLINE_MARKERS) {                                        // (uniform: block_rank has a barrier)
            const unsigned char *st = state + (size_t)vs * (CAPTION_STATE_HEADER + sizeof(ffgpu_zone_slot) * (size_t)a.capacity);
            const unsigned frames = *reinterpret_cast<const unsigned *>(st);
            const ffgpu_zone_slot *slot = reinterpret_cast<const ffgpu_zone_slot *>(st + CAPTION_STATE_HEADER);
            const bool seen = tid < a.capacity && slot[tid].id != 0 && (unsigned)slot[tid].last == frames - 1u;
            const int k = block_rank(seen, s_wsum, 4);
            if (seen && FFGPU_OUTLINE_FIXED + 2 * k + 1 < a.items_stride) {
                const long long cx = draw_f2i(slot[tid].px), cy = draw_f2i(slot[tid].py), r = a.marker;
                const unsigned col = a.pal[draw_colour_index(slot[tid].id, a.npal)];
                unsigned *row = s_row + (FFGPU_OUTLINE_FIXED + 2 * k) * 8;
                seg_put(row, cx - r, cy, cx + r, cy, col, 1, 0);
                seg_put(row + 8, cx, cy - r, cx, cy + r, col, 1, 0);
            }
        }
    }
    __syncthreads();
    unsigned *dst = items + T * (size_t)nwords;
    for (int i = tid; i < nwords; i += blockDim.x) dst[i] = s_row[i];
}

// ---- host side
extern "C" int ffgpu_outline_spec_check(const ffgpu_outline_spec *spec)
{
    OutlinePlan pl;
    return ffgpu_outline_spec_plan("outline_spec_check", spec, pl);
}

// everything has been checked; targets[t] draws items t * items_stride ...
int ffgpu_launch_draw_segments(bool nv12, const void *d_items, int items_stride, const std::vector<DrawTarget> &targets, hipStream_t s)
{
    const int n = (int)targets.size();
    for (int t0 = 0; t0 < n; t0 += SEG_ARG_TARGETS) {
        const int nt = std::min(SEG_ARG_TARGETS, n - t0);
        SegArgs a;
        memset(&a, 0, sizeof a);
        memcpy(a.t, targets.data() + t0, sizeof(DrawTarget) * (size_t)nt);
        a.t0 = t0; a.stride = items_stride;
        const dim3 grid((unsigned)std::min(items_stride, SEG_GROUPS), (unsigned)nt);
        if (nv12) hipLaunchKernelGGL(k_draw_segments<true>, grid, dim3(256), 0, s, a, (const unsigned *)d_items);
        else      hipLaunchKernelGGL(k_draw_segments<false>, grid, dim3(256), 0, s, a, (const unsigned *)d_items);
        LAUNCH_OK("draw_segments");
    }
    return 0;
}

template <class Frame>
static int draw_segments_dev(const char *what, const void *d_items, int items_stride, const Frame *targets, int ntargets, void *stream)
{
    if (ffgpu_no_device(what)) return -1;
    if (ffgpu_draw_segments_args_check(what, d_items, items_stride, targets, ntargets)) return -1;
    std::vector<DrawTarget> tab;
    if (ffgpu_frame_table(what, FRAME_DRAW, targets, ntargets, tab)) return -1;
    return ffgpu_launch_draw_segments(std::is_same<Frame, ffgpu_nv12_frame>::value, d_items, items_stride, tab, (hipStream_t)stream);
}

extern "C" int ffgpu_draw_segments_bgr_dev(const void *d_items, int items_stride, const ffgpu_bgr_frame *targets, int ntargets, void *stream)
{
    return draw_segments_dev("draw_segments_bgr_dev", d_items, items_stride, targets, ntargets, stream);
}

extern "C" int ffgpu_draw_segments_nv12_dev(const void *d_items, int items_stride, const ffgpu_nv12_frame *targets, int ntargets, void *stream)
{
    return draw_segments_dev("draw_segments_nv12_dev", d_items, items_stride, targets, ntargets, stream);
}

extern "C" int ffgpu_outline_scene_dev(const void *d_scenes, const void *d_state, int nstreams, int capacity, const void *d_events, int events_stride,
                                       const int *streams, int ntargets, const ffgpu_outline_spec *spec, void *d_items, int items_stride, void *stream)
{
    const char *const what = "outline_scene_dev";
    if (ffgpu_no_device(what)) return -1;
    OutlinePlan pl;
    if (ffgpu_outline_scene_args_check(what, d_scenes, d_state, nstreams, capacity, d_events, events_stride, streams, ntargets, spec, d_items, items_stride, pl)) return -1;
    for (int t0 = 0; t0 < ntargets; t0 += OUTLINE_ARG_TARGETS) {
        const int nt = std::min(OUTLINE_ARG_TARGETS, ntargets - t0);
        OutlineArgs a;
        memset(&a, 0, sizeof a);
        memcpy(a.stream, streams + t0, sizeof(int) * (size_t)nt);
        memcpy(a.pal, pl.pal, sizeof a.pal);
        a.npal = pl.npal; a.flags = pl.flags; a.thickness = pl.thickness; a.line_dash = pl.line_dash; a.marker = pl.marker; a.t0 = t0;
        a.items_stride = items_stride; a.capacity = capacity; a.events_stride = events_stride; a.alarm = pl.alarm;
        hipLaunchKernelGGL(k_outline_scene, dim3((unsigned)nt), dim3(256), 0, (hipStream_t)stream, a, (const unsigned char *)d_scenes, (const unsigned char *)d_state,
                           (const unsigned *)d_events, (unsigned *)d_items);
        LAUNCH_OK("outline_scene");
    }
    return 0;
}
