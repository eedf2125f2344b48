// heat_driver.cc -- ffgpu_heat_host.hpp on the CPU under AddressSanitizer + UBSan (`make heat`; tests/test_heat_abi.py): the state's size, the two heat
// specs resolved into their plans, the built-in palette, and the argument checks of the accumulate operator and of the blend, on good and hostile
// arguments.  One line per case: id, return value, message.  The last line is "heat_driver: N cases, 0 wrong".  Nothing of HIP: the addresses are
// made up and never followed.  `heat_driver palette` prints the two built-in palettes as hex instead (2 x 1024 bytes).
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <limits>
#include "../ffgpu_heat_host.hpp"

static char g_err[512];
extern "C" void ffgpu_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

static int g_cases, g_wrong;
static void line(const char *id, int rc, int want_rc, const char *want_msg)
{
    const bool ok = rc == want_rc && (rc == 0 || strstr(g_err, want_msg));
    g_cases++;
    g_wrong += !ok;
    printf("%s %d %s%s\n", id, rc, rc ? g_err : "", ok ? "" : "   <-- WRONG");
}
static void fact(const char *id, bool ok)
{
    g_cases++;
    g_wrong += !ok;
    printf("%s %s\n", id, ok ? "holds" : "fails   <-- WRONG");
}

static const void *at(uintptr_t a) { return reinterpret_cast<const void *>(a); }
static const unsigned char g_classes[3] = { 1, 0, 1 };
static unsigned char g_palette[1024];

static ffgpu_heat_spec good_spec()
{
    ffgpu_heat_spec sp;
    memset(&sp, 0, sizeof sp);
    sp.gw = 40; sp.gh = 23; sp.cell_log2 = 4; sp.mode = FFGPU_HEAT_ANCHOR; sp.anchor = 1; sp.spread = 2; sp.gain = 64; sp.decay_shift = 5; sp.min_score = 0.25f;
    return sp;
}
static ffgpu_heat_blend_spec good_blend()
{
    ffgpu_heat_blend_spec sp;
    memset(&sp, 0, sizeof sp);
    sp.gw = 40; sp.gh = 23; sp.cell_log2 = 4; sp.full_scale = 1000; sp.floor = 8; sp.opacity = 160; sp.sampling = FFGPU_HEAT_SMOOTH; sp.flags = FFGPU_HEAT_RAMP_ALPHA;
    return sp;
}

template <class Fn> static void spec(const char *id, int want_rc, const char *want_msg, Fn change)
{
    ffgpu_heat_spec sp = good_spec();
    change(sp);
    g_err[0] = 0;
    HeatPlan pl;
    line(id, ffgpu_heat_spec_plan("op", &sp, pl), want_rc, want_msg);
}
template <class Fn> static void blend(const char *id, int want_rc, const char *want_msg, Fn change)
{
    ffgpu_heat_blend_spec sp = good_blend();
    change(sp);
    g_err[0] = 0;
    HeatBlendPlan pl;
    line(id, ffgpu_heat_blend_spec_plan("op", &sp, false, pl), want_rc, want_msg);
}

struct Args {
    std::vector<int> streams{ 0, 2, -1, 1, 0 };
    bool have_streams = true, have_spec = true;
    ffgpu_heat_spec spec = good_spec();
    uintptr_t state = 0x2000, rows = 0x4000;
    int nstreams = 3, ntargets = 5;
};
template <class Fn> static void args(const char *id, int want_rc, const char *want_msg, Fn change)
{
    Args a;
    change(a);
    g_err[0] = 0;
    HeatPlan pl;
    line(id, ffgpu_heat_args_check("op", a.have_streams ? a.streams.data() : nullptr, a.ntargets, a.have_spec ? &a.spec : nullptr, at(a.state), a.nstreams, at(a.rows), pl),
         want_rc, want_msg);
}

struct BArgs {
    std::vector<int> streams{ 0, -1, 1 };
    std::vector<ffgpu_bgr_frame> bgr;
    std::vector<ffgpu_nv12_frame> nv;
    bool have_streams = true, have_spec = true, have_targets = true;
    ffgpu_heat_blend_spec spec = good_blend();
    uintptr_t state = 0x2000;
    int nstreams = 2, ntargets = 3;
    BArgs()
    {
        bgr.resize(3); nv.resize(3);
        for (int k = 0; k < 3; k++) {
            memset(&bgr[k], 0, sizeof bgr[k]); memset(&nv[k], 0, sizeof nv[k]);
            bgr[k].bgr = (const unsigned char *)at(0x10001 + 0x10000 * k); bgr[k].w = 65; bgr[k].h = 33; bgr[k].pitch = 200;
            nv[k].y = (const unsigned char *)at(0x10001 + 0x10000 * k); nv[k].uv = (const unsigned char *)at(0x18000 + 0x10000 * k); nv[k].w = 65; nv[k].h = 33;
        }
        bgr[2].bgr = nullptr; nv[2].y = nullptr;                                   // a skipped target
    }
};
template <class Fn> static void bargs(const char *id, bool nv12, int want_rc, const char *want_msg, Fn change)
{
    BArgs a;
    change(a);
    g_err[0] = 0;
    HeatBlendPlan pl;
    std::vector<DrawTarget> tab;
    int rc;
    const int *st = a.have_streams ? a.streams.data() : nullptr;
    const ffgpu_heat_blend_spec *sp = a.have_spec ? &a.spec : nullptr;
    if (nv12) rc = ffgpu_heat_blend_args_check("op", at(a.state), a.nstreams, st, a.have_targets ? a.nv.data() : nullptr, a.ntargets, sp, true, pl, tab);
    else      rc = ffgpu_heat_blend_args_check("op", at(a.state), a.nstreams, st, a.have_targets ? a.bgr.data() : nullptr, a.ntargets, sp, false, pl, tab);
    line(id, rc, want_rc, want_msg);
    if (rc == 0 && want_rc == 0)
        fact(id, tab.size() == 3 && tab[0].p0 && tab[0].first == 0 && !tab[1].p0 && tab[1].first == -1 && !tab[2].p0 && tab[2].first == 1 && tab[0].w == 65 && tab[0].h == 33 &&
                 tab[0].pitch == (nv12 ? 65 : 200) && (nv12 ? tab[0].p1 != nullptr && tab[0].pitch_uv == 66 : tab[0].p1 == nullptr));
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "palette")) {
        for (int nv12 = 0; nv12 < 2; nv12++) {
            unsigned char pal[1024];
            ffgpu_heat_palette_host(nv12, pal);
            for (int i = 0; i < 1024; i++) printf("%02x", pal[i]);
            printf("\n");
        }
        return 0;
    }
    const int imin = std::numeric_limits<int>::min(), imax = std::numeric_limits<int>::max();
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();

    // the state's size: per stream a 16-byte header and 4 bytes per cell, rounded up to 16; 0 outside the ranges
    fact("bytes.1x1x1", ffgpu_heat_state_bytes_host(1, 1, 1) == 32);
    fact("bytes.3x3x2", ffgpu_heat_state_bytes_host(3, 3, 2) == 3u * 48u);
    fact("bytes.2x17x5", ffgpu_heat_state_bytes_host(2, 17, 5) == 2u * 368u);
    fact("bytes.65536x128x128", ffgpu_heat_state_bytes_host(65536, 128, 128) == (size_t)65536 * (16u + 65536u));
    fact("bytes.outside", ffgpu_heat_state_bytes_host(0, 1, 1) == 0 && ffgpu_heat_state_bytes_host(65537, 1, 1) == 0 && ffgpu_heat_state_bytes_host(1, 0, 1) == 0 &&
                          ffgpu_heat_state_bytes_host(1, 129, 1) == 0 && ffgpu_heat_state_bytes_host(1, 1, 0) == 0 && ffgpu_heat_state_bytes_host(1, 1, 129) == 0 &&
                          ffgpu_heat_state_bytes_host(imin, imin, imin) == 0 && ffgpu_heat_state_bytes_host(imax, imax, imax) == 0);
    fact("bytes.sixteen", ffgpu_heat_state_bytes_host(7, 5, 3) % 16 == 0 && ffgpu_heat_stream_bytes(5, 3) == 80);

    // the built-in palette: the anchors, a midpoint, byte 3, the NV12 conversion's ends
    {
        unsigned char b[1024], y[1024];
        ffgpu_heat_palette_host(0, b);
        ffgpu_heat_palette_host(1, y);
        auto is = [](const unsigned char *p, int v, int c0, int c1, int c2) { return p[4 * v] == c0 && p[4 * v + 1] == c1 && p[4 * v + 2] == c2 && p[4 * v + 3] == 0; };
        fact("palette.anchors", is(b, 0, 255, 0, 0) && is(b, 64, 255, 255, 0) && is(b, 128, 0, 255, 0) && is(b, 192, 0, 255, 255) && is(b, 255, 0, 0, 255));
        fact("palette.between", is(b, 32, 255, 128, 0) && is(b, 1, 255, 4, 0) && is(b, 254, 0, 4, 255) && is(b, 96, 128, 255, 0));
        fact("palette.nv12", is(y, 0, 29, 255, 107) && is(y, 255, 77, 85, 255) && is(y, 128, 149, 43, 21));
    }

    // the plans of good specs
    {
        ffgpu_heat_spec sp = good_spec();
        HeatPlan pl;
        g_err[0] = 0;
        line("plan.spec", ffgpu_heat_spec_plan("op", &sp, pl), 0, "");
        fact("plan.spec_values", pl.gw == 40 && pl.gh == 23 && pl.cell_log2 == 4 && pl.mode == 0 && pl.anchor == 1 && pl.spread == 2 && pl.gain == 64 && pl.decay_shift == 5 &&
                                 pl.min_score == 0.25f && pl.nclasses == 0);
        sp.classes = g_classes; sp.nclasses = 3;
        line("plan.classes", ffgpu_heat_spec_plan("op", &sp, pl), 0, "");
        fact("plan.classes_values", pl.nclasses == 3 && pl.classes[0] == 1 && pl.classes[1] == 0 && pl.classes[2] == 1 && pl.classes[3] == 0);
        line("plan.null_spec", ffgpu_heat_spec_plan("op", nullptr, pl), -1, "NULL spec");
        ffgpu_heat_blend_spec bs = good_blend();
        HeatBlendPlan bp;
        line("plan.blend", ffgpu_heat_blend_spec_plan("op", &bs, false, bp), 0, "");
        fact("plan.blend_values", bp.gw == 40 && bp.gh == 23 && bp.cell_log2 == 4 && bp.full_scale == 1000 && bp.floor == 8 && bp.opacity == 160 && bp.smooth == 1 && bp.ramp == 1 &&
                                  bp.pal[0] == 0x0000ffu && bp.pal[64] == 0x00ffffu && bp.pal[255] == 0xff0000u);
        line("plan.blend_nv12", ffgpu_heat_blend_spec_plan("op", &bs, true, bp), 0, "");
        fact("plan.blend_nv12_values", bp.pal[0] == (29u | 255u << 8 | 107u << 16));
        for (int i = 0; i < 1024; i++) g_palette[i] = (unsigned char)(i * 7);
        bs.palette = g_palette;
        line("plan.blend_palette", ffgpu_heat_blend_spec_plan("op", &bs, true, bp), 0, "");
        fact("plan.blend_palette_values", bp.pal[1] == ((4u * 7u) | (5u * 7u) << 8 | (6u * 7u) << 16) && bp.pal[255] == ((1020u * 7u & 255u) | (1021u * 7u & 255u) << 8 | (1022u * 7u & 255u) << 16));
        line("plan.null_blend", ffgpu_heat_blend_spec_plan("op", nullptr, false, bp), -1, "NULL spec");
    }

    spec("spec.good", 0, "", [](ffgpu_heat_spec &) {});
    spec("spec.box", 0, "", [](ffgpu_heat_spec &s) { s.mode = FFGPU_HEAT_BOX; s.spread = 0; });
    spec("spec.smallest", 0, "", [](ffgpu_heat_spec &s) { s.gw = s.gh = 1; s.cell_log2 = 1; s.anchor = 0; s.spread = 0; s.gain = 1; s.decay_shift = 0; s.min_score = 0.f; });
    spec("spec.largest", 0, "", [](ffgpu_heat_spec &s) { s.gw = s.gh = 128; s.cell_log2 = 8; s.spread = 4; s.gain = 65536; s.decay_shift = 16; s.min_score = 1.f; });
    spec("spec.min_score_nan", 0, "", [&](ffgpu_heat_spec &s) { s.min_score = nan; });
    spec("spec.min_score_inf", 0, "", [&](ffgpu_heat_spec &s) { s.min_score = -inf; });
    spec("spec.classes_256", 0, "", [](ffgpu_heat_spec &s) { static unsigned char big[256]; s.classes = big; s.nclasses = 256; });
    spec("spec.gw_0", -1, "a grid of 0 x 23 cells (1..128 each)", [](ffgpu_heat_spec &s) { s.gw = 0; });
    spec("spec.gw_129", -1, "a grid of 129 x 23 cells", [](ffgpu_heat_spec &s) { s.gw = 129; });
    spec("spec.gh_0", -1, "a grid of 40 x 0 cells", [](ffgpu_heat_spec &s) { s.gh = 0; });
    spec("spec.gh_129", -1, "a grid of 40 x 129 cells", [](ffgpu_heat_spec &s) { s.gh = 129; });
    spec("spec.gw_min", -1, "a grid of", [&](ffgpu_heat_spec &s) { s.gw = imin; });
    spec("spec.cell_0", -1, "cell_log2 0 is outside 1..8", [](ffgpu_heat_spec &s) { s.cell_log2 = 0; });
    spec("spec.cell_9", -1, "cell_log2 9 is outside 1..8", [](ffgpu_heat_spec &s) { s.cell_log2 = 9; });
    spec("spec.mode_2", -1, "mode 2 is neither FFGPU_HEAT_ANCHOR nor FFGPU_HEAT_BOX", [](ffgpu_heat_spec &s) { s.mode = 2; });
    spec("spec.mode_neg", -1, "mode -1", [](ffgpu_heat_spec &s) { s.mode = -1; });
    spec("spec.flags_1", -1, "unknown flags 0x1", [](ffgpu_heat_spec &s) { s.flags = 1; });
    spec("spec.flags_min", -1, "unknown flags 0x80000000", [&](ffgpu_heat_spec &s) { s.flags = imin; });
    spec("spec.anchor_2", -1, "anchor 2 is neither 0 nor 1", [](ffgpu_heat_spec &s) { s.anchor = 2; });
    spec("spec.anchor_neg", -1, "anchor -1", [](ffgpu_heat_spec &s) { s.anchor = -1; });
    spec("spec.spread_neg", -1, "spread -1 is outside 0..4", [](ffgpu_heat_spec &s) { s.spread = -1; });
    spec("spec.spread_5", -1, "spread 5 is outside 0..4", [](ffgpu_heat_spec &s) { s.spread = 5; });
    spec("spec.spread_box", -1, "spread 2 with FFGPU_HEAT_BOX (0 then)", [](ffgpu_heat_spec &s) { s.mode = FFGPU_HEAT_BOX; });
    spec("spec.gain_0", -1, "gain 0 is outside 1..65536", [](ffgpu_heat_spec &s) { s.gain = 0; });
    spec("spec.gain_65537", -1, "gain 65537 is outside 1..65536", [](ffgpu_heat_spec &s) { s.gain = 65537; });
    spec("spec.gain_max", -1, "gain", [&](ffgpu_heat_spec &s) { s.gain = imax; });
    spec("spec.decay_neg", -1, "decay_shift -1 is outside 0..16", [](ffgpu_heat_spec &s) { s.decay_shift = -1; });
    spec("spec.decay_17", -1, "decay_shift 17 is outside 0..16", [](ffgpu_heat_spec &s) { s.decay_shift = 17; });
    spec("spec.nclasses_without_classes", -1, "nclasses 3 (0 with NULL classes, else 1..256)", [](ffgpu_heat_spec &s) { s.nclasses = 3; });
    spec("spec.classes_without_nclasses", -1, "nclasses 0", [](ffgpu_heat_spec &s) { s.classes = g_classes; });
    spec("spec.nclasses_257", -1, "nclasses 257", [](ffgpu_heat_spec &s) { s.classes = g_classes; s.nclasses = 257; });
    spec("spec.nclasses_neg", -1, "nclasses -1", [](ffgpu_heat_spec &s) { s.classes = g_classes; s.nclasses = -1; });
    spec("spec.reserved", -1, "reserved must be 0", [](ffgpu_heat_spec &s) { s.reserved = 1; });

    blend("blend.good", 0, "", [](ffgpu_heat_blend_spec &) {});
    blend("blend.smallest", 0, "", [](ffgpu_heat_blend_spec &s) { s.gw = s.gh = 1; s.cell_log2 = 1; s.full_scale = 0; s.floor = 0; s.opacity = 1; s.sampling = 0; s.flags = 0; });
    blend("blend.largest", 0, "", [&](ffgpu_heat_blend_spec &s) { s.gw = s.gh = 128; s.cell_log2 = 8; s.full_scale = imax; s.floor = 255; s.opacity = 255; });
    blend("blend.gw_0", -1, "a grid of 0 x 23 cells (1..128 each)", [](ffgpu_heat_blend_spec &s) { s.gw = 0; });
    blend("blend.gh_129", -1, "a grid of 40 x 129 cells", [](ffgpu_heat_blend_spec &s) { s.gh = 129; });
    blend("blend.cell_0", -1, "cell_log2 0 is outside 1..8", [](ffgpu_heat_blend_spec &s) { s.cell_log2 = 0; });
    blend("blend.cell_9", -1, "cell_log2 9 is outside 1..8", [](ffgpu_heat_blend_spec &s) { s.cell_log2 = 9; });
    blend("blend.full_scale_neg", -1, "negative full_scale -1", [](ffgpu_heat_blend_spec &s) { s.full_scale = -1; });
    blend("blend.full_scale_min", -1, "negative full_scale", [&](ffgpu_heat_blend_spec &s) { s.full_scale = imin; });
    blend("blend.floor_neg", -1, "floor -1 is outside 0..255", [](ffgpu_heat_blend_spec &s) { s.floor = -1; });
    blend("blend.floor_256", -1, "floor 256 is outside 0..255", [](ffgpu_heat_blend_spec &s) { s.floor = 256; });
    blend("blend.opacity_0", -1, "opacity 0 is outside 1..255", [](ffgpu_heat_blend_spec &s) { s.opacity = 0; });
    blend("blend.opacity_256", -1, "opacity 256 is outside 1..255", [](ffgpu_heat_blend_spec &s) { s.opacity = 256; });
    blend("blend.sampling_2", -1, "sampling 2 is neither FFGPU_HEAT_NEAREST nor FFGPU_HEAT_SMOOTH", [](ffgpu_heat_blend_spec &s) { s.sampling = 2; });
    blend("blend.sampling_neg", -1, "sampling -1", [](ffgpu_heat_blend_spec &s) { s.sampling = -1; });
    blend("blend.flags_2", -1, "unknown flags 0x2", [](ffgpu_heat_blend_spec &s) { s.flags = 2; });
    blend("blend.flags_min", -1, "unknown flags", [&](ffgpu_heat_blend_spec &s) { s.flags = imin; });
    blend("blend.reserved0", -1, "reserved must be 0", [](ffgpu_heat_blend_spec &s) { s.reserved[0] = 1; });
    blend("blend.reserved1", -1, "reserved must be 0", [](ffgpu_heat_blend_spec &s) { s.reserved[1] = -1; });

    args("args.good", 0, "", [](Args &) {});
    args("args.null_streams", -1, "NULL streams", [](Args &a) { a.have_streams = false; });
    args("args.null_spec", -1, "NULL spec", [](Args &a) { a.have_spec = false; });
    args("args.null_state", -1, "NULL state", [](Args &a) { a.state = 0; });
    args("args.null_rows", -1, "NULL rows", [](Args &a) { a.rows = 0; });
    args("args.gain_0", -1, "gain 0", [](Args &a) { a.spec.gain = 0; });
    args("args.ntargets_0", -1, "0 targets", [](Args &a) { a.ntargets = 0; });
    args("args.ntargets_neg", -1, "-1 targets", [](Args &a) { a.ntargets = -1; });
    args("args.nstreams_0", -1, "nstreams 0", [](Args &a) { a.nstreams = 0; });
    args("args.nstreams_65537", -1, "nstreams 65537", [](Args &a) { a.nstreams = 65537; });
    args("args.state_unaligned", -1, "the state must be 16-byte aligned", [](Args &a) { a.state += 8; });
    args("args.stream_high", -1, "target 1: stream 2 is outside -1 .. 1", [](Args &a) { a.nstreams = 2; });
    args("args.stream_low", -1, "target 3: stream -2", [](Args &a) { a.streams[3] = -2; });

    for (int nv12 = 0; nv12 < 2; nv12++) {
        const bool n = nv12 != 0;
        bargs(n ? "nv12.good" : "bgr.good", n, 0, "", [](BArgs &) {});
        bargs(n ? "nv12.null_state" : "bgr.null_state", n, -1, "NULL state", [](BArgs &a) { a.state = 0; });
        bargs(n ? "nv12.null_streams" : "bgr.null_streams", n, -1, "NULL streams", [](BArgs &a) { a.have_streams = false; });
        bargs(n ? "nv12.null_targets" : "bgr.null_targets", n, -1, "NULL targets", [](BArgs &a) { a.have_targets = false; });
        bargs(n ? "nv12.null_spec" : "bgr.null_spec", n, -1, "NULL spec", [](BArgs &a) { a.have_spec = false; });
        bargs(n ? "nv12.opacity_0" : "bgr.opacity_0", n, -1, "opacity 0", [](BArgs &a) { a.spec.opacity = 0; });
        bargs(n ? "nv12.ntargets_0" : "bgr.ntargets_0", n, -1, "0 targets", [](BArgs &a) { a.ntargets = 0; });
        bargs(n ? "nv12.nstreams_0" : "bgr.nstreams_0", n, -1, "nstreams 0", [](BArgs &a) { a.nstreams = 0; });
        bargs(n ? "nv12.nstreams_65537" : "bgr.nstreams_65537", n, -1, "nstreams 65537", [](BArgs &a) { a.nstreams = 65537; });
        bargs(n ? "nv12.state_unaligned" : "bgr.state_unaligned", n, -1, "the state must be 16-byte aligned", [](BArgs &a) { a.state += 4; });
        bargs(n ? "nv12.stream_high" : "bgr.stream_high", n, -1, "target 2: stream 1 is outside -1 .. 0", [](BArgs &a) { a.nstreams = 1; });
        bargs(n ? "nv12.stream_low" : "bgr.stream_low", n, -1, "target 0: stream -2", [](BArgs &a) { a.streams[0] = -2; });
        bargs(n ? "nv12.bad_size" : "bgr.bad_size", n, -1, "target 1: bad size 0 x 33", [](BArgs &a) { a.bgr[1].w = 0; a.nv[1].w = 0; });
        bargs(n ? "nv12.target_reserved" : "bgr.target_reserved", n, -1, "target 0: reserved must be 0", [](BArgs &a) { a.bgr[0].reserved = 1; a.nv[0].reserved = 1; });
    }
    bargs("bgr.pitch", false, -1, "target 0: pitch 100 is below 3 w = 195", [](BArgs &a) { a.bgr[0].pitch = 100; });
    bargs("nv12.pitch_y", true, -1, "target 0: pitch_y 10 is below w = 65", [](BArgs &a) { a.nv[0].pitch_y = 10; });
    bargs("nv12.pitch_uv", true, -1, "target 0: pitch_uv 65 is odd", [](BArgs &a) { a.nv[0].pitch_uv = 65; });
    bargs("nv12.uv_odd", true, -1, "is odd (U V pairs are written", [](BArgs &a) { a.nv[0].uv = (const unsigned char *)at(0x18001); });
    bargs("nv12.matrix", true, -1, "target 1: matrix 4", [](BArgs &a) { a.nv[1].matrix = 4; });

    printf("heat_driver: %d cases, %d wrong\n", g_cases, g_wrong);
    return g_wrong ? 1 : 0;
}
