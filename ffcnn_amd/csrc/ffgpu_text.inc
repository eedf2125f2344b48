// ffgpu_text.inc -- captions: text rasterised into the frames on the device, and the composers that write it from the boxes and from the zones' counters
// (ffgpu_draw_text_bgr_dev / _nv12_dev, ffgpu_caption_boxes_dev, ffgpu_caption_scene_dev, ffgpu_exec_caption_bgr / _nv12, ffgpu_font_builtin).  The
// contract is in include/ffcnn_hip.h; the host side (font table, spec and argument checks) is ffgpu_text_host.hpp.
//
// The rasteriser follows k_draw_boxes: items run in parallel, so the LAST WRITER of every byte is computed instead of raced for.  The lane that owns
// pixel (x, y) of item k stores it only if no item j > k of the target writes that pixel -- a rectangle check, plus one glyph bit for an item that is not
// opaque -- and a chroma sample is owned the same way: by the last item that writes any of its luma pixels.  Every byte is stored with one value per
// launch, whichever lanes store it.  A target's items (16 KB at most) and the font (2 KB) are staged in LDS; an item's rectangle is clipped to the
// target before the lanes stride over it, so an item at +-2^31 costs nothing.  Byte stores and one aligned 2-byte store per (U, V) pair; no atomics.
#define TEXT_GROUPS 16            // workgroups per target: workgroup g draws items g, g + 16, ...
struct TextArgs {
    DrawTarget t[TEXT_ARG_TARGETS];
    int t0, stride, pad_[2];      // target blockIdx.y of the launch is target t0 + blockIdx.y of the call; items_stride
};
static_assert(sizeof(TextArgs) + 2 * 8 <= 4096 - 256, "the tables travel as a kernel argument (4 KB at most, the hidden arguments included)");
static_assert(FFGPU_TEXT_ITEMS == 256 && FFGPU_TEXT_MAX == 44 && offsetof(ffgpu_text_item, text) == 20 && offsetof(ffgpu_text_item, scale) == 16,
              "k_draw_text: a lane stages an item's geometry; the layout of include/ffcnn_hip.h");

__constant__ unsigned char c_font8[FONT8_GLYPHS * 8] = {
#include "ffgpu_font8.inc"
};

struct TextLds {
    unsigned raw[FFGPU_TEXT_ITEMS * 16];              // the target's items as they lie in memory
    int4     geo[FFGPU_TEXT_ITEMS];                   // item j: x, y, 8 s n (0: draws nothing), s | opaque << 8
    unsigned char font[2048];
    int      wmax[4];
};

// what item (g, txt) does to pixel (px, py): 0 nothing, 1 writes paper, 2 writes ink.  dx < 8 * 4 * 44 and s <= 4: dx / s is a multiplication.
__device__ __forceinline__ int text_hit(const int4 g, const unsigned char *txt, const unsigned char *font, int px, int py)
{
    const int s = g.w & 0xff;
    const long long dx = (long long)px - g.x, dy = (long long)py - g.y;
    if (dx < 0 || dx >= g.z || dy < 0 || dy >= 8 * s) return 0;
    const unsigned inv = s == 3 ? 21846u : 65536u >> (s >> 1);
    const unsigned qx = ((unsigned)dx * inv) >> 16, qy = ((unsigned)dy * inv) >> 16;
    const unsigned bits = font[txt[qx >> 3] * 8u + qy];
    return ((bits >> (7u - (qx & 7u))) & 1u) ? 2 : (g.w >> 8) & 1;
}

// grid (TEXT_GROUPS, targets of this launch), 256 lanes.  Whatever the items hold, nothing is read outside them and the font, and every store lies
// inside the target's w x h.
template <bool NV12>
__global__ void __launch_bounds__(256) k_draw_text(TextArgs a, const unsigned *items, const unsigned char *font)
{
    __shared__ __attribute__((aligned(16))) unsigned char s_text[sizeof(TextLds)];
    TextLds &L = *reinterpret_cast<TextLds *>(s_text);
    const DrawTarget &t = a.t[blockIdx.y];
    if (!t.p0) return;                                                                // a skipped target (uniform)
    const int tid = threadIdx.x, stride = a.stride, w = t.w, h = t.h;
    const unsigned *src = items + ((size_t)a.t0 + blockIdx.y) * (size_t)stride * 16u;
    for (int i = tid; i < stride * 16; i += blockDim.x) L.raw[i] = src[i];
    for (int i = tid; i < 2048; i += blockDim.x) {
        const int g = i >> 3;
        L.font[i] = font ? font[i] : c_font8[(g >= 32 && g <= 126 ? g - 32 : FONT8_GLYPHS - 1) * 8 + (i & 7)];
    }
    __syncthreads();
    bool used = false;
    if (tid < stride) {
        const unsigned m = L.raw[tid * 16 + 4];
        const int s = min(max((int)(m & 0xffu), 1), 4), n = min((int)((m >> 16) & 0xffu), FFGPU_TEXT_MAX);
        L.geo[tid] = make_int4((int)L.raw[tid * 16], (int)L.raw[tid * 16 + 1], 8 * s * n, s | (int)((m >> 8) & 1u) << 8);
        used = n > 0;
    }
    {
        const unsigned long long m = __ballot(used);
        if ((tid & (WAVE - 1)) == 0) L.wmax[tid / WAVE] = m ? (tid / WAVE) * WAVE + 64 - __clzll((long long)m) : 0;
    }
    __syncthreads();
    const int n = max(max(L.wmax[0], L.wmax[1]), max(L.wmax[2], L.wmax[3]));          // behind the last item that draws anything
    for (int k = blockIdx.x; k < n; k += gridDim.x) {
        const int4 g = L.geo[k];
        if (g.z <= 0) continue;
        const long long X0 = max((long long)g.x, 0LL), X1 = min((long long)g.x + g.z, (long long)w);
        const long long Y0 = max((long long)g.y, 0LL), Y1 = min((long long)g.y + 8 * (g.w & 0xff), (long long)h);
        if (X1 <= X0 || Y1 <= Y0) continue;                                           // clipped away
        const unsigned fg = L.raw[k * 16 + 2], bg = L.raw[k * 16 + 3];
        const unsigned char *txt = reinterpret_cast<const unsigned char *>(&L.raw[k * 16 + 5]);
        for (int y = (int)Y0 + (tid >> 6); y < (int)Y1; y += 4)
            for (int x = (int)X0 + (tid & 63); x < (int)X1; x += 64) {
                const int me = text_hit(g, txt, L.font, x, y);
                if (!me) continue;
                // the last writer: a later item that writes this pixel owns it (and, NV12, its chroma sample); a later item on another luma pixel of
                // the sample owns the sample alone
                const int x1 = x ^ 1, y1 = y ^ 1, xl = NV12 ? x & ~1 : x, xh = NV12 ? x | 1 : x, yl = NV12 ? y & ~1 : y, yh = NV12 ? y | 1 : y;
                bool later = false, later_uv = false;
                for (int j = k + 1; j < n; j++) {
                    const int4 q = L.geo[j];
                    if (xh < q.x || (long long)xl - q.x >= q.z || yh < q.y || (long long)yl - q.y >= 8 * (q.w & 0xff)) continue;
                    const unsigned char *tj = reinterpret_cast<const unsigned char *>(&L.raw[j * 16 + 5]);
                    if (text_hit(q, tj, L.font, x, y)) { later = true; break; }
                    if (NV12 && !later_uv)
                        later_uv = (x1 < w && text_hit(q, tj, L.font, x1, y)) || (y1 < h && (text_hit(q, tj, L.font, x, y1) || (x1 < w && text_hit(q, tj, L.font, x1, y1))));
                }
                if (later) continue;
                const unsigned col = me == 2 ? fg : bg;
                if (NV12) {
                    t.p0[(size_t)y * (size_t)t.pitch + (size_t)x] = (unsigned char)col;
                    if (!later_uv) {
                        const bool ink = me == 2 || (x1 < w && text_hit(g, txt, L.font, x1, y) == 2) ||
                                         (y1 < h && (text_hit(g, txt, L.font, x, y1) == 2 || (x1 < w && text_hit(g, txt, L.font, x1, y1) == 2)));
                        *reinterpret_cast<unsigned short *>(t.p1 + (size_t)(y >> 1) * (size_t)t.pitch_uv + 2 * (size_t)(x >> 1)) = (unsigned short)((ink ? fg : bg) >> 8);
                    }
                } else {
                    unsigned char *px = t.p0 + (size_t)y * (size_t)t.pitch + 3 * (size_t)x;
                    px[0] = (unsigned char)col; px[1] = (unsigned char)(col >> 8); px[2] = (unsigned char)(col >> 16);
                }
            }
    }
}

// ---- the composers.  An item is composed by one lane in its 64 bytes of LDS and leaves the workgroup as words; decimal digits are taken in registers,
// least significant first into a packed word (a division by the constant 10), and written most significant first.
struct TextPen { unsigned char *txt; int pos; };
__device__ __forceinline__ void pen_put(TextPen &p, unsigned c) { if (p.pos < FFGPU_TEXT_MAX) p.txt[p.pos] = (unsigned char)c; p.pos++; }
__device__ __forceinline__ void pen_dec(TextPen &p, unsigned v)
{
    unsigned long long bcd = 0;
    int nd = 0;
    do { const unsigned q = v / 10u; bcd = bcd << 4 | (v - q * 10u); v = q; nd++; } while (v);
    for (int i = 0; i < nd; i++) { pen_put(p, '0' + (unsigned)(bcd & 15u)); bcd >>= 4; }
}
__device__ __forceinline__ void pen_gap(TextPen &p) { if (p.pos > 0) pen_put(p, ' '); }
// the item's words 0..4 and its pen
__device__ __forceinline__ TextPen pen_open(unsigned *row, int x, int y, unsigned fg, unsigned bg)
{
    row[0] = (unsigned)x; row[1] = (unsigned)y; row[2] = fg; row[3] = bg;
    return TextPen{ reinterpret_cast<unsigned char *>(row) + offsetof(ffgpu_text_item, text), 0 };
}
__device__ __forceinline__ void pen_close(const TextPen &p, unsigned *row, int scale, bool opaque)
{
    row[4] = (unsigned)scale | (opaque ? (unsigned)FFGPU_TEXT_OPAQUE << 8 : 0u) | (unsigned)min(p.pos, FFGPU_TEXT_MAX) << 16;
}

struct CaptionArgs {
    long long first[CAPTION_ARG_TARGETS];             // target blockIdx.x of the launch: its list's first box in `lists`
    unsigned  pal[256];
    float     min_score;
    int       flags, identity, scale, nnames, npal, t0, items_stride;
    unsigned  fg;
    int       pad_;
};
static_assert(sizeof(CaptionArgs) + 6 * 8 <= 4096 - 256, "the tables travel as a kernel argument (4 KB at most, the hidden arguments included)");
static_assert(FFGPU_CAPTION_DETS <= 256 && FFGPU_TEXT_ITEMS <= 256, "k_caption_boxes: a lane composes an item");

// grid = targets of the launch, 256 lanes.  Counts are clamped to [0, stride] as the draw kernel clamps them.
__global__ void __launch_bounds__(256) k_caption_boxes(CaptionArgs a, const ffgpu_frame_dets *recs, const BBOX *lists, int stride, const unsigned char *names,
                                                       const int *ids, unsigned *items)
{
#pragma clang fp contract(off)
    __shared__ unsigned s_row[FFGPU_TEXT_ITEMS * 16];
    __shared__ int s_idx[FFGPU_CAPTION_DETS], s_wsum[4];
    const int tid = threadIdx.x, nwords = a.items_stride * 16;
    const size_t T = (size_t)a.t0 + blockIdx.x;
    const ffgpu_frame_dets *rec = recs + T;
    const int n = max(0, min(lists ? rec->nfull : rec->count, stride)), cap = min(FFGPU_CAPTION_DETS, a.items_stride);
    const BBOX *list = lists ? lists + a.first[blockIdx.x] : rec->box;
    for (int i = tid; i < nwords; i += blockDim.x) s_row[i] = 0;
    int nq = 0;                                                                       // qualifying boxes so far (uniform)
    for (long long k0 = 0; k0 < n && nq < cap; k0 += 256) {
        const int k = (int)min(k0 + tid, (long long)n);
        const bool q = k < n && list[k].score >= a.min_score;
        int tot;
        const int ord = nq + block_rank(q, s_wsum, 4, tot);
        if (q && ord < cap) s_idx[ord] = k;
        nq += tot;
        __syncthreads();
    }
    __syncthreads();
    if (tid < min(nq, cap)) {
        const int k = s_idx[tid];
        const BBOX b = list[k];
        const int s8 = 8 * a.scale, bx = draw_f2i(b.x1), by = draw_f2i(b.y1);
        unsigned *row = s_row + tid * 16;
        TextPen p = pen_open(row, bx, by >= s8 ? by - s8 : by, a.fg, a.pal[draw_colour_index(b.type, a.npal)]);
        if ((a.flags & FFGPU_CAPTION_NAME) && a.identity != FFGPU_ZONES_TYPE) {
            if (b.type >= 0 && b.type < a.nnames) {
                const unsigned char *nm = names + (size_t)b.type * 16u;
                for (int i = 0; i < 16 && nm[i]; i++) pen_put(p, nm[i]);
            } else {
                if (b.type < 0) pen_put(p, '-');
                pen_dec(p, b.type < 0 ? 0u - (unsigned)b.type : (unsigned)b.type);
            }
        }
        if (a.flags & FFGPU_CAPTION_SCORE) {
            const float pf = b.score * 100.0f;
            pen_gap(p);
            pen_dec(p, (unsigned)min(max(draw_f2i(pf + 0.5f), 0), 999));
            pen_put(p, '%');
        }
        if (a.flags & FFGPU_CAPTION_ID) {
            const int v = a.identity == FFGPU_ZONES_TYPE ? b.type : a.identity == FFGPU_ZONES_IDS ? ids[T * (8u + (size_t)stride) + 8u + (size_t)k] : 0;
            if (v != 0) {
                pen_gap(p);
                pen_put(p, '#');
                pen_dec(p, v < 0 ? 0u - (unsigned)v : (unsigned)v);
                if (v < 0) pen_put(p, '?');
            }
        }
        pen_close(p, row, a.scale, (a.flags & FFGPU_CAPTION_OPAQUE) != 0);
    }
    __syncthreads();
    unsigned *dst = items + T * (size_t)nwords;
    for (int i = tid; i < nwords; i += blockDim.x) dst[i] = s_row[i];
}

struct SceneCapArgs {
    int      stream[SCENE_ARG_TARGETS];               // target blockIdx.x of the launch: its video stream, or -1
    unsigned pal[256];
    int      npal, scale, opaque, t0, items_stride, capacity, events_stride, pad_;
    unsigned fg;
    int      pad2_;
};
static_assert(sizeof(SceneCapArgs) + 4 * 8 <= 4096 - 256, "the tables travel as a kernel argument (4 KB at most, the hidden arguments included)");
static_assert(FFGPU_SCENE_ZONES == 8 && FFGPU_SCENE_LINES == 8 && CAPTION_STATE_HEADER == ZONES_STATE_HEADER, "k_caption_scene: lanes 0..7 the zones, 8..15 the lines");

// grid = targets of the launch, 256 lanes: lanes 0..15 compose, all copy.  Total over any scene bytes, as k_zones.
__global__ void __launch_bounds__(256) k_caption_scene(SceneCapArgs a, const unsigned char *scenes, const unsigned char *state, const unsigned *events, unsigned *items)
{
    __shared__ unsigned s_row[FFGPU_TEXT_ITEMS * 16];
    const int tid = threadIdx.x, nwords = a.items_stride * 16, vs = a.stream[blockIdx.x];
    const size_t T = (size_t)a.t0 + blockIdx.x;
    for (int i = tid; i < nwords; i += blockDim.x) s_row[i] = 0;
    __syncthreads();
    if (vs >= 0 && tid < FFGPU_SCENE_ZONES + FFGPU_SCENE_LINES) {
        const ffgpu_scene &S = *reinterpret_cast<const ffgpu_scene *>(scenes + (size_t)vs * sizeof(ffgpu_scene));
        const unsigned bg = a.pal[draw_colour_index(tid, a.npal)];
        unsigned *row = s_row + tid * 16;
        if (tid < FFGPU_SCENE_ZONES) {
            const ffgpu_zone &z = S.zone[tid];
            if (tid < max(0, min(S.nzones, FFGPU_SCENE_ZONES)) && z.nverts >= 3 && z.nverts <= FFGPU_ZONE_VERTS) {
                TextPen p = pen_open(row, draw_f2i(z.x[0]), draw_f2i(z.y[0]), a.fg, bg);
                pen_put(p, 'Z'); pen_put(p, '0' + (unsigned)tid); pen_put(p, ' ');
                pen_dec(p, events[T * (size_t)a.events_stride + 16u + 4u * (unsigned)tid]);
                pen_close(p, row, a.scale, a.opaque != 0);
            }
        } else {
            const int l = tid - FFGPU_SCENE_ZONES;
            if (l < max(0, min(S.nlines, FFGPU_SCENE_LINES))) {
                const unsigned *hdr = reinterpret_cast<const unsigned *>(state + (size_t)vs * (CAPTION_STATE_HEADER + sizeof(ffgpu_zone_slot) * (size_t)a.capacity));
                TextPen p = pen_open(row, draw_f2i(S.line[l].ax), draw_f2i(S.line[l].ay), a.fg, bg);
                pen_put(p, 'L'); pen_put(p, '0' + (unsigned)l); pen_put(p, ' ');
                pen_dec(p, hdr[20 + l]);
                pen_put(p, '/');
                pen_dec(p, hdr[28 + l]);
                pen_close(p, row, a.scale, a.opaque != 0);
            }
        }
    }
    __syncthreads();
    unsigned *dst = items + T * (size_t)nwords;
    for (int i = tid; i < nwords; i += blockDim.x) dst[i] = s_row[i];
}

// ---- host side
extern "C" void ffgpu_font_builtin(unsigned char out[2048]) { if (out) ffgpu_font_builtin_host(out); }

// everything has been checked; targets[t] draws items t * items_stride ...
int ffgpu_launch_draw_text(bool nv12, const void *d_items, int items_stride, const void *d_font, const std::vector<DrawTarget> &targets, hipStream_t s)
{
    const int n = (int)targets.size();
    for (int t0 = 0; t0 < n; t0 += TEXT_ARG_TARGETS) {
        const int nt = std::min(TEXT_ARG_TARGETS, n - t0);
        TextArgs a;
        memset(&a, 0, sizeof a);
        memcpy(a.t, targets.data() + t0, sizeof(DrawTarget) * (size_t)nt);
        a.t0 = t0; a.stride = items_stride;
        const dim3 grid((unsigned)std::min(items_stride, TEXT_GROUPS), (unsigned)nt);
        if (nv12) hipLaunchKernelGGL(k_draw_text<true>, grid, dim3(256), 0, s, a, (const unsigned *)d_items, (const unsigned char *)d_font);
        else      hipLaunchKernelGGL(k_draw_text<false>, grid, dim3(256), 0, s, a, (const unsigned *)d_items, (const unsigned char *)d_font);
        LAUNCH_OK("draw_text");
    }
    return 0;
}

int ffgpu_launch_caption_boxes(const DetSource &src, int ntargets, const CaptionPlan &pl, const void *d_ids, void *d_items, int items_stride, hipStream_t s)
{
    for (int t0 = 0; t0 < ntargets; t0 += CAPTION_ARG_TARGETS) {
        const int nt = std::min(CAPTION_ARG_TARGETS, ntargets - t0);
        CaptionArgs a;
        memset(&a, 0, sizeof a);
        for (int i = 0; i < nt; i++) a.first[i] = src.first[t0 + i];
        memcpy(a.pal, pl.pal, sizeof a.pal);
        a.min_score = pl.min_score; a.flags = pl.flags; a.identity = pl.identity; a.scale = pl.scale; a.nnames = pl.nnames; a.npal = pl.npal;
        a.t0 = t0; a.items_stride = items_stride; a.fg = pl.fg;
        hipLaunchKernelGGL(k_caption_boxes, dim3((unsigned)nt), dim3(256), 0, s, a, src.recs, src.lists, src.stride, (const unsigned char *)pl.d_names,
                           (const int *)d_ids, (unsigned *)d_items);
        LAUNCH_OK("caption_boxes");
    }
    return 0;
}

template <class Frame>
static int draw_text_dev(const char *what, const void *d_items, int items_stride, const void *d_font, const Frame *targets, int ntargets, void *stream)
{
    if (ffgpu_no_device(what)) return -1;
    if (ffgpu_draw_text_args_check(what, d_items, items_stride, targets, ntargets)) return -1;
    std::vector<DrawTarget> tab;
    if (ffgpu_frame_table(what, FRAME_DRAW, targets, ntargets, tab)) return -1;
    return ffgpu_launch_draw_text(std::is_same<Frame, ffgpu_nv12_frame>::value, d_items, items_stride, d_font, tab, (hipStream_t)stream);
}

extern "C" int ffgpu_draw_text_bgr_dev(const void *d_items, int items_stride, const void *d_font, const ffgpu_bgr_frame *targets, int ntargets, void *stream)
{
    return draw_text_dev("draw_text_bgr_dev", d_items, items_stride, d_font, targets, ntargets, stream);
}

extern "C" int ffgpu_draw_text_nv12_dev(const void *d_items, int items_stride, const void *d_font, const ffgpu_nv12_frame *targets, int ntargets, void *stream)
{
    return draw_text_dev("draw_text_nv12_dev", d_items, items_stride, d_font, targets, ntargets, stream);
}

extern "C" int ffgpu_caption_boxes_dev(const void *d_records, const void *d_lists, int list_stride, const int *list_first, int ntargets,
                                       const ffgpu_caption_spec *spec, const void *d_ids, void *d_items, int items_stride, void *stream)
{
    const char *const what = "caption_boxes_dev";
    if (ffgpu_no_device(what)) return -1;
    CaptionPlan pl;
    if (ffgpu_caption_boxes_args_check(what, spec, d_ids, d_items, items_stride, pl) || ffgpu_ntargets_check(what, ntargets)) return -1;
    DetSource src;
    if (ffgpu_source_dev(what, d_records, d_lists, list_stride, list_first, ntargets, src)) return -1;
    return ffgpu_launch_caption_boxes(src, ntargets, pl, d_ids, d_items, items_stride, (hipStream_t)stream);
}

extern "C" int ffgpu_caption_scene_dev(const void *d_scenes, const void *d_state, int nstreams, int capacity, const void *d_events, int events_stride,
                                       const int *streams, int ntargets, const ffgpu_caption_spec *spec, void *d_items, int items_stride, void *stream)
{
    const char *const what = "caption_scene_dev";
    if (ffgpu_no_device(what)) return -1;
    CaptionPlan pl;
    if (ffgpu_caption_scene_args_check(what, d_scenes, d_state, nstreams, capacity, d_events, events_stride, streams, ntargets, spec, d_items, items_stride, pl)) return -1;
    for (int t0 = 0; t0 < ntargets; t0 += SCENE_ARG_TARGETS) {
        const int nt = std::min(SCENE_ARG_TARGETS, ntargets - t0);
        SceneCapArgs a;
        memset(&a, 0, sizeof a);
        memcpy(a.stream, streams + t0, sizeof(int) * (size_t)nt);
        memcpy(a.pal, pl.pal, sizeof a.pal);
        a.npal = pl.npal; a.scale = pl.scale; a.opaque = (pl.flags & FFGPU_CAPTION_OPAQUE) != 0; a.t0 = t0; a.items_stride = items_stride;
        a.capacity = capacity; a.events_stride = events_stride; a.fg = pl.fg;
        hipLaunchKernelGGL(k_caption_scene, dim3((unsigned)nt), dim3(256), 0, (hipStream_t)stream, a, (const unsigned char *)d_scenes, (const unsigned char *)d_state,
                           (const unsigned *)d_events, (unsigned *)d_items);
        LAUNCH_OK("caption_scene");
    }
    return 0;
}
