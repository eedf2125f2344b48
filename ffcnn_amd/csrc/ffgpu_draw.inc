// ffgpu_draw.inc -- the detections outlined in the frames on the device (ffgpu_draw_boxes_bgr_dev / _nv12_dev, ffgpu_exec_draw_bgr / _nv12): the
// last step of the reference's program (ffcnn.c:583-589, bmp_rectangle of bmpfile.c:145-156) without a host round trip.  The contract is in
// include/ffcnn_hip.h.
//
// Serial order without relying on memory order: a target's result is what drawing its boxes one after the other would leave.  Boxes run in
// parallel here, so the LAST WRITER of every byte is computed instead of raced for: the lane that owns outline pixel (x, y) of box k stores it
// only if no box j > k of the same target has that pixel in its set (NV12 chroma: only if no later box touches any luma pixel of the sample).
// Every byte of a target is then stored with one value per launch -- several lanes may store it (the corners of one box, its rectangles where
// they meet), all with the same value -- and the result is the same byte for byte on every run.
//
// The frame table, the list starts and the palette travel as ONE by-value kernel argument (DrawArgs, DRAW_ARG_TARGETS targets per launch; more
// targets: more launches): nothing is copied from pageable host memory on the stream.
#define DRAW_ARG_TARGETS 64
#define DRAW_LDS_BOXES   256      // a target's list up to this length is staged in LDS (the normal case: tens); a longer one is read where it lies
#define DRAW_GROUPS      16       // workgroups per target: workgroup g draws boxes g, g + 16, ...
struct DrawArgs {
    DrawTarget t[DRAW_ARG_TARGETS];
    unsigned   pal[256];          // byte 0, 1, 2 of an entry: B G R (BGR targets) or Y U V (NV12 targets)
    int        npal, thickness, rec0, pad_;
};
static_assert(sizeof(DrawTarget) == 40 && sizeof(DrawArgs) + 3 * 8 <= 4096 - 256, "the tables travel as a kernel argument (4 KB at most, the hidden arguments included)");

// (int)v as v_cvt_i32_f32 does it -- toward zero, saturating, NaN -> 0 -- spelled out: the C cast is undefined outside int
__device__ __forceinline__ int draw_f2i(float v)
{
    if (!(v == v)) return 0;
    if (v >= 2147483648.f) return 0x7fffffff;
    if (v <= -2147483648.f) return (int)0x80000000;
    return (int)v;
}

// A box's integer corners, each clamped to [-9, size + 8].  For every pixel inside the target and every i < 8 the tests "x == a + i", "a + i <= x",
// "x == c - i" and "x <= c - i" give the same answer with the clamped corner as with the exact one computed in 64 bits, so a +-1e30 box costs
// nothing and a + i never wraps.
__device__ __forceinline__ int4 draw_corners(const BBOX &b, int w, int h)
{
    int4 r;
    r.x = min(max(draw_f2i(b.x1), -9), w + 8); r.y = min(max(draw_f2i(b.y1), -9), h + 8);
    r.z = min(max(draw_f2i(b.x2), -9), w + 8); r.w = min(max(draw_f2i(b.y2), -9), h + 8);
    return r;
}

// pixel (x, y), inside the target, is in the set of the T rectangles of r.  While no rectangle of the T is inverted (c - a and d - b >= 2 (T - 1): every
// box but a sliver) their outlines tile the ring between rectangle 0 and the inside of rectangle T - 1: eight comparisons, no loop; a sliver
// takes the rectangles one by one.  (The clamp of draw_corners moves no corner that lies within 8 pixels of the target, so a clamped box is a
// sliver only where both of its edges are outside, and there both forms agree on every pixel inside.)
__device__ __forceinline__ bool draw_hits(int4 r, int T, int x, int y)
{
    const int e = T - 1;
    if (r.z - r.x >= 2 * e && r.w - r.y >= 2 * e)
        return ((r.x <= x) & (x <= r.z) & (r.y <= y) & (y <= r.w)) && !((r.x + e < x) & (x < r.z - e) & (r.y + e < y) & (y < r.w - e));
    for (int i = 0; i < T; i++) {
        const int A = r.x + i, B = r.y + i, C = r.z - i, D = r.w - i;
        if (((y == B) | (y == D)) & (A <= x) & (x <= C)) return true;
        if (((x == A) | (x == C)) & (B <= y) & (y <= D)) return true;
    }
    return false;
}

__device__ __forceinline__ int draw_colour_index(int type, int npal) { const int m = type % npal; return m < 0 ? m + npal : m; }

// grid (DRAW_GROUPS, targets of this launch), 256 lanes.  Target blockIdx.y draws record rec0 + blockIdx.y: lists == NULL its own box[0 .. count),
// else nfull boxes from lists + first.  Counts are clamped to [0, stride]: whatever the records hold, nothing is read outside the buffers the host
// has sized, and every store lies inside the target's w x h.
template <bool NV12>
__global__ void __launch_bounds__(256) k_draw_boxes(DrawArgs a, const ffgpu_frame_dets *recs, const BBOX *lists, int stride)
{
    __shared__ int4 s_rc[DRAW_LDS_BOXES];
    __shared__ int  s_ci[DRAW_LDS_BOXES];
    const DrawTarget &t = a.t[blockIdx.y];
    if (!t.p0) return;                                                                // a skipped target (uniform)
    const ffgpu_frame_dets *rec = recs + a.rec0 + blockIdx.y;
    const int n = max(0, min(lists ? rec->nfull : rec->count, stride));
    if ((int)blockIdx.x >= n) return;                                                 // (uniform: in front of the barrier)
    const BBOX *list = lists ? lists + t.first : rec->box;
    const int tid = threadIdx.x, w = t.w, h = t.h, T = a.thickness, npal = a.npal;
    const bool in_lds = n <= DRAW_LDS_BOXES;                                          // uniform
    if (in_lds) {
        for (int j = tid; j < n; j += blockDim.x) { const BBOX b = list[j]; s_rc[j] = draw_corners(b, w, h); s_ci[j] = draw_colour_index(b.type, npal); }
        __syncthreads();
    }
    auto corners = [&](int j) { return in_lds ? s_rc[j] : draw_corners(list[j], w, h); };
    for (int k = blockIdx.x; k < n; k += gridDim.x) {
        const int4 r = corners(k);
        const unsigned col = a.pal[in_lds ? s_ci[k] : draw_colour_index(list[k].type, npal)];
        for (int i = 0; i < T; i++) {
            // rectangle i clipped to the target: two rows of lh pixels from xa, two columns of lv pixels from ya, each only where it lies inside
            const int A = r.x + i, B = r.y + i, C = r.z - i, D = r.w - i;
            const int xa = max(A, 0), xb = min(C, w - 1), ya = max(B, 0), yb = min(D, h - 1);
            const long long lh = xb >= xa ? (long long)xb - xa + 1 : 0, lv = yb >= ya ? (long long)yb - ya + 1 : 0;
            const long long n0 = (unsigned)B < (unsigned)h ? lh : 0, n1 = n0 + ((unsigned)D < (unsigned)h ? lh : 0);
            const long long n2 = n1 + ((unsigned)A < (unsigned)w ? lv : 0), n3 = n2 + ((unsigned)C < (unsigned)w ? lv : 0);
            for (long long p = tid; p < n3; p += blockDim.x) {
                int x, y;
                if (p < n0)      { x = xa + (int)p;        y = B; }
                else if (p < n1) { x = xa + (int)(p - n0); y = D; }
                else if (p < n2) { x = A;                  y = ya + (int)(p - n1); }
                else             { x = C;                  y = ya + (int)(p - n2); }
                // the last writer: a later box that has this pixel owns it (and, NV12, its chroma sample); a later box on another luma pixel of the
                // sample owns the sample alone
                bool later = false, later_uv = false;
                for (int j = k + 1; j < n; j++) {
                    const int4 q = corners(j);
                    if (draw_hits(q, T, x, y)) { later = true; break; }
                    if (NV12 && !later_uv) {
                        const int x1 = x ^ 1, y1 = y ^ 1;
                        later_uv = (x1 < w && draw_hits(q, T, x1, y)) || (y1 < h && (draw_hits(q, T, x, y1) || (x1 < w && draw_hits(q, T, x1, y1))));
                    }
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

// ---- host side: the caller's style checked once for the operators and the executor forms (the descriptors: ffgpu_frame_table, role FRAME_DRAW)
int ffgpu_draw_style_check(const char *what, const ffgpu_draw_style *st, unsigned pal[256], int *npal)
{
    if (!st) { ffgpu_set_error("%s: NULL style", what); return -1; }
    if (st->thickness < 1 || st->thickness > 8) { ffgpu_set_error("%s: thickness %d is outside 1..8", what, st->thickness); return -1; }
    return ffgpu_palette_plan(what, st->palette, st->npalette, st->color, pal, npal);
}

// targets[t] draws record t of `src`; DRAW_ARG_TARGETS targets per launch
int ffgpu_launch_draw(bool nv12, const DetSource &src, const std::vector<DrawTarget> &targets, const unsigned pal[256], int npal, int thickness, hipStream_t s)
{
    const int n = (int)targets.size();
    for (int t0 = 0; t0 < n; t0 += DRAW_ARG_TARGETS) {
        const int nt = std::min(DRAW_ARG_TARGETS, n - t0);
        DrawArgs a;
        memset(&a, 0, sizeof a);
        memcpy(a.t, targets.data() + t0, sizeof(DrawTarget) * (size_t)nt);
        for (int i = 0; i < nt; i++) a.t[i].first = src.first[t0 + i];
        memcpy(a.pal, pal, sizeof a.pal);
        a.npal = npal; a.thickness = thickness; a.rec0 = t0;
        const dim3 grid((unsigned)std::min(src.stride, DRAW_GROUPS), (unsigned)nt);
        if (nv12) hipLaunchKernelGGL(k_draw_boxes<true>, grid, dim3(256), 0, s, a, src.recs, src.lists, src.stride);
        else      hipLaunchKernelGGL(k_draw_boxes<false>, grid, dim3(256), 0, s, a, src.recs, src.lists, src.stride);
        LAUNCH_OK("draw_boxes");
    }
    return 0;
}

template <class Frame>
static int draw_boxes_dev(const char *what, const void *d_records, const void *d_lists, int list_stride, const int *list_first,
                          const Frame *targets, int ntargets, const ffgpu_draw_style *style, void *stream)
{
    if (ffgpu_no_device(what)) return -1;
    if (!targets) { ffgpu_set_error("%s: NULL targets", what); return -1; }
    unsigned pal[256];
    int npal = 0;
    if (ffgpu_draw_style_check(what, style, pal, &npal)) return -1;
    if (ntargets < 1 || ntargets > (1 << 24)) { ffgpu_set_error("%s: %d targets (ntargets >= 1)", what, ntargets); return -1; }
    DetSource src;
    if (ffgpu_source_dev(what, d_records, d_lists, list_stride, list_first, ntargets, src)) return -1;
    std::vector<DrawTarget> tab;
    if (ffgpu_frame_table(what, FRAME_DRAW, targets, ntargets, tab)) return -1;
    return ffgpu_launch_draw(std::is_same<Frame, ffgpu_nv12_frame>::value, src, tab, pal, npal, style->thickness, (hipStream_t)stream);
}

extern "C" int ffgpu_draw_boxes_bgr_dev(const void *d_records, const void *d_lists, int list_stride, const int *list_first,
                                        const ffgpu_bgr_frame *targets, int ntargets, const ffgpu_draw_style *style, void *stream)
{
    return draw_boxes_dev("draw_boxes_bgr_dev", d_records, d_lists, list_stride, list_first, targets, ntargets, style, stream);
}

extern "C" int ffgpu_draw_boxes_nv12_dev(const void *d_records, const void *d_lists, int list_stride, const int *list_first,
                                         const ffgpu_nv12_frame *targets, int ntargets, const ffgpu_draw_style *style, void *stream)
{
    return draw_boxes_dev("draw_boxes_nv12_dev", d_records, d_lists, list_stride, list_first, targets, ntargets, style, stream);
}
