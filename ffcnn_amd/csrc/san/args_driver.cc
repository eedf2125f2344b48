// args_driver.cc -- ffgpu_args.hpp on the CPU under AddressSanitizer + UBSan (`make args`; tests/test_args_host.py): a fixed table of cases, one line
// each: id, return value, message -- and for an accepted descriptor the fields it resolves to.  Nothing of HIP: the addresses are made up and
// never followed.
#include <cstdarg>
#include <cstdio>
#include "../ffgpu_args.hpp"

static char g_err[512];
extern "C" void ffgpu_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

static const unsigned char *at(uintptr_t a) { return reinterpret_cast<const unsigned char *>(a); }
static const uintptr_t BASE = 0x10000000;

template <class Frame> static void frame(const char *id, const FrameRole &role, int k, const Frame &f)
{
    FrameArgs a;
    g_err[0] = 0;
    const int rc = ffgpu_frame_check("op", role, k, f, a);
    printf("%s %d %s", id, rc, g_err);
    if (!rc) printf("p0=%llx p1=%llx w=%d h=%d pitch=%d pitch_uv=%d fmt=%d", (unsigned long long)(uintptr_t)a.p0, (unsigned long long)(uintptr_t)a.p1, a.w, a.h, a.pitch, a.pitch_uv, a.fmt);
    printf("\n");
}

static ffgpu_bgr_frame bgr(uintptr_t p, int w, int h, int pitch = 0, int reserved = 0)
{
    ffgpu_bgr_frame f = { at(p), w, h, pitch, reserved };
    return f;
}
static ffgpu_nv12_frame nv12(uintptr_t y, uintptr_t uv, int w, int h, int pitch_y = 0, int pitch_uv = 0, int matrix = 0, int reserved = 0)
{
    ffgpu_nv12_frame f = { at(y), at(uv), w, h, pitch_y, pitch_uv, matrix, reserved };
    return f;
}

static void source(const char *id, int rc, const DetSource &s)
{
    printf("%s %d %s", id, rc, rc ? g_err : "");
    if (!rc) {
        printf("lists=%d stride=%d longest=%lld first=", s.lists != nullptr, s.stride, s.longest);
        for (size_t t = 0; t < s.first.size(); t++) printf("%s%lld", t ? "," : "", s.first[t]);
    }
    printf("\n");
}
static void dev(const char *id, bool lists, int list_stride, const int *list_first, int ntargets, bool recs = true)
{
    DetSource s;
    g_err[0] = 0;
    source(id, ffgpu_source_dev("op", recs ? at(BASE) : nullptr, lists ? at(2 * BASE) : nullptr, list_stride, list_first, ntargets, s), s);
}
static void exec(const char *id, const char *family, int which, int ntargets, int N, int cand_cap, const std::vector<int> *off)
{
    DetSource s;
    g_err[0] = 0;
    source(id, ffgpu_source_exec("op", family, which, ntargets, N, cand_cap, off, s), s);
}

int main()
{
    const FrameRole *roles[2] = { &FRAME_FORWARD, &FRAME_DRAW };
    const char *rn[2] = { "fwd", "draw" };
    char id[64];
    for (int r = 0; r < 2; r++) {
        const FrameRole &R = *roles[r];
#define ID(name) (snprintf(id, sizeof id, "%s.%s", rn[r], name), id)
        // BGR: rejections, defaults, both sides of the bounds
        frame(ID("bgr.null"), R, 0, bgr(0, 64, 48));
        frame(ID("bgr.null_badsize"), R, 1, bgr(0, 0, 48));
        frame(ID("bgr.w0"), R, 2, bgr(BASE, 0, 48));
        frame(ID("bgr.hneg"), R, 3, bgr(BASE, 64, -1));
        frame(ID("bgr.reserved"), R, 4, bgr(BASE, 64, 48, 0, 7));
        frame(ID("bgr.pitch_default"), R, 5, bgr(BASE, 63, 48));
        frame(ID("bgr.pitch_3w"), R, 6, bgr(BASE, 63, 48, 189));
        frame(ID("bgr.pitch_3w_less_1"), R, 7, bgr(BASE, 63, 48, 188));
        frame(ID("bgr.pitch_negative"), R, 8, bgr(BASE, 63, 48, -4));
        frame(ID("bgr.w_max"), R, 9, bgr(BASE, 0x2aaaaaaa, 1, 0x7ffffffe));
        frame(ID("bgr.w_max_plus_1"), R, 10, bgr(BASE, 0x2aaaaaab, 1, 0x7fffffff));
        frame(ID("bgr.w_max_pitch_default"), R, 10, bgr(BASE, 0x2aaaaaaa, 1));
        frame(ID("bgr.h_3fffffff"), R, 11, bgr(BASE, 1, 0x3fffffff));
        frame(ID("bgr.h_40000000"), R, 12, bgr(BASE, 1, 0x40000000));
        frame(ID("bgr.h_7fffffff"), R, 13, bgr(BASE, 1, 0x7fffffff));
        // NV12
        frame(ID("nv12.null"), R, 0, nv12(0, 0, 64, 48));
        frame(ID("nv12.null_badmatrix"), R, 1, nv12(0, 0, 64, 48, 0, 0, 4));
        frame(ID("nv12.w0"), R, 2, nv12(BASE, 0, 0, 48));
        frame(ID("nv12.w_40000000"), R, 3, nv12(BASE, 0, 0x40000000, 2));
        frame(ID("nv12.h_40000000"), R, 4, nv12(BASE, BASE, 2, 0x40000000));
        frame(ID("nv12.reserved"), R, 5, nv12(BASE, 0, 64, 48, 0, 0, 0, 1));
        frame(ID("nv12.matrix_neg"), R, 6, nv12(BASE, 0, 64, 48, 0, 0, -1));
        frame(ID("nv12.matrix_4"), R, 7, nv12(BASE, 0, 64, 48, 0, 0, 4));
        frame(ID("nv12.pitch_y_low"), R, 8, nv12(BASE, 0, 64, 48, 63));
        frame(ID("nv12.pitch_uv_low"), R, 9, nv12(BASE, 0, 63, 48, 0, 62));
        frame(ID("nv12.pitch_uv_odd"), R, 10, nv12(BASE, 0, 63, 48, 0, 65));
        frame(ID("nv12.pitch_uv_even"), R, 11, nv12(BASE, 0, 63, 48, 0, 66, 3));
        frame(ID("nv12.defaults"), R, 12, nv12(BASE, 0, 63, 48, 0, 0, 2));
        frame(ID("nv12.pitches_given"), R, 13, nv12(BASE, 0, 64, 48, 80, 96, 1));
        frame(ID("nv12.uv_given"), R, 14, nv12(BASE, 3 * BASE, 64, 48));
        frame(ID("nv12.uv_odd"), R, 15, nv12(BASE, BASE + 0x1001, 64, 48));
        frame(ID("nv12.uv_default_odd"), R, 16, nv12(BASE, 0, 63, 47, 65));
        frame(ID("nv12.w_3fffffff"), R, 17, nv12(BASE, BASE, 0x3fffffff, 1));
#undef ID
    }

    // the operator forms' source
    const int first[4] = { 7, 0, 300, 12 }, neg[4] = { 7, 0, -5, -6 };
    dev("dev.null_records", true, 100, nullptr, 4, false);
    dev("dev.first_null", true, 100, nullptr, 4);
    dev("dev.first_given", true, 100, first, 4);
    dev("dev.first_negative", true, 100, neg, 4);
    dev("dev.no_lists", false, 0, neg, 4);
    dev("dev.stride_0", true, 0, nullptr, 4);
    dev("dev.stride_2p24", true, 1 << 24, nullptr, 2);
    dev("dev.stride_2p24_plus_1", true, (1 << 24) + 1, nullptr, 2);
    g_err[0] = 0;
    printf("stride.no_lists %d %s\n", ffgpu_list_stride("op", nullptr, -3), g_err);
    printf("stride.lists %d %s\n", ffgpu_list_stride("op", at(BASE), 1500), g_err);
    printf("stride.bad %d %s\n", ffgpu_list_stride("op", at(BASE), -3), g_err);

    // the executor forms' source
    const std::vector<int> off = { 0, 2, 2, 5 }, none, big = { 0, 1, 3 };
    exec("exec.entries", "DRAW", 0, 3, 3, 1500, nullptr);
    exec("exec.merged", "DRAW", 1, 3, 5, 1500, &off);
    const char *fam[4] = { "DRAW", "CROP", "TRACK", "RELABEL" };
    for (int i = 0; i < 4; i++) { snprintf(id, sizeof id, "exec.which_2.%s", fam[i]); exec(id, fam[i], 2, 3, 3, 1500, &off); }
    exec("exec.which_neg", "TRACK", -1, 3, 3, 1500, &off);
    exec("exec.merged_no_merge", "CROP", 1, 3, 3, 1500, nullptr);
    exec("exec.merged_empty", "CROP", 1, 3, 3, 1500, &none);
    exec("exec.count_entries", "TRACK", 0, 4, 3, 1500, &off);
    exec("exec.count_merged", "RELABEL", 1, 5, 5, 1500, &off);
    exec("exec.past_2p31", "DRAW", 1, 2, 3, 0x7fffffff, &big);
    return 0;
}
