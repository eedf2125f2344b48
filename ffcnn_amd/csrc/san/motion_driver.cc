// motion_driver.cc -- ffgpu_motion_host.hpp on the CPU under AddressSanitizer + UBSan (`make motion`; tests/test_motion_abi.py): the state's layout and
// size, the motion spec resolved into its plan, the argument checks of the update and of the gate, and the rounds of an update call, on good and
// hostile arguments.  One line per case: id, return value, message.  The last line is "motion_driver: N cases, 0 wrong".  Nothing of HIP: the
// addresses are made up and never followed.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <limits>
#include "../ffgpu_motion_host.hpp"

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
    const bool ok = (want_rc < 0 ? rc == want_rc : rc >= 0) && (rc >= 0 || strstr(g_err, want_msg));
    g_cases++;
    g_wrong += !ok;
    printf("%s %d %s%s\n", id, rc, rc < 0 ? g_err : "", ok ? "" : "   <-- WRONG");
}
static void fact(const char *id, bool ok)
{
    g_cases++;
    g_wrong += !ok;
    printf("%s %s\n", id, ok ? "holds" : "fails   <-- WRONG");
}

static const void *at(uintptr_t a) { return reinterpret_cast<const void *>(a); }
static const unsigned char g_classes[3] = { 1, 0, 1 };

static ffgpu_motion_spec good_spec()
{
    ffgpu_motion_spec sp;
    memset(&sp, 0, sizeof sp);
    sp.w = 65; sp.h = 33; sp.cell_log2 = 4; sp.threshold = 20; sp.learn_shift = 4; sp.learn_shift_changed = 8; sp.min_pixels = 16; sp.cover = 64; sp.warmup = 30;
    sp.flags = FFGPU_MOTION_GATE_INVERT; sp.min_score = 0.25f;
    return sp;
}

template <class Fn> static void spec(const char *id, int want_rc, const char *want_msg, Fn change)
{
    ffgpu_motion_spec sp = good_spec();
    change(sp);
    g_err[0] = 0;
    MotionPlan pl;
    line(id, ffgpu_motion_spec_plan("op", &sp, pl), want_rc, want_msg);
}

struct UArgs {
    std::vector<int> streams{ 0, 2, -1, 0, 1, 0 };
    std::vector<ffgpu_bgr_frame> bgr;
    std::vector<ffgpu_nv12_frame> nv;
    bool have_streams = true, have_spec = true, have_targets = true;
    ffgpu_motion_spec spec = good_spec();
    uintptr_t state = 0x2000, rows = 0x4000;
    int nstreams = 3, ntargets = 6;
    UArgs()
    {
        bgr.resize(6); nv.resize(6);
        for (int k = 0; k < 6; k++) {
            memset(&bgr[k], 0, sizeof bgr[k]); memset(&nv[k], 0, sizeof nv[k]);
            bgr[k].bgr = (const unsigned char *)at(0x10001 + 0x10000 * k); bgr[k].w = 65; bgr[k].h = 33; bgr[k].pitch = 200;
            nv[k].y = (const unsigned char *)at(0x10001 + 0x10000 * k); nv[k].uv = (const unsigned char *)at(0x18000 + 0x10000 * k); nv[k].w = 65; nv[k].h = 33;
        }
        bgr[4].bgr = nullptr; nv[4].y = nullptr;                                   // a skipped target
    }
};
template <class Fn> static void uargs(const char *id, bool nv12, int want_rc, const char *want_msg, Fn change)
{
    UArgs a;
    change(a);
    g_err[0] = 0;
    MotionPlan pl;
    std::vector<DrawTarget> tab;
    std::vector<int> round;
    int rc;
    const int *st = a.have_streams ? a.streams.data() : nullptr;
    const ffgpu_motion_spec *sp = a.have_spec ? &a.spec : nullptr;
    if (nv12) rc = ffgpu_motion_update_args_check("op", a.have_targets ? a.nv.data() : nullptr, a.ntargets, st, sp, at(a.state), a.nstreams, at(a.rows), pl, tab, round);
    else      rc = ffgpu_motion_update_args_check("op", a.have_targets ? a.bgr.data() : nullptr, a.ntargets, st, sp, at(a.state), a.nstreams, at(a.rows), pl, tab, round);
    line(id, rc, want_rc, want_msg);
    if (rc >= 0 && want_rc >= 0)                                                   // streams 0 2 -1 0 (1, skipped) 0: three rounds, the skipped ones in round 0
        fact(id, rc == 3 && tab.size() == 6 && round == std::vector<int>({ 0, 0, 0, 1, 0, 2 }) && tab[0].p0 && tab[0].first == 0 && !tab[2].p0 && tab[2].first == -1 &&
                 !tab[4].p0 && tab[4].first == 1 && tab[5].first == 0 && tab[0].w == 65 && tab[0].h == 33 && tab[5].w == 65 && tab[0].pitch == (nv12 ? 65 : 200));
}

struct GArgs {
    std::vector<int> streams{ 0, 2, -1, 1, 0 };
    bool have_streams = true, have_spec = true;
    ffgpu_motion_spec spec = good_spec();
    uintptr_t state = 0x2000, words = 0x4000, out_recs = 0x8000, out_lists = 0xc000;
    int nstreams = 3, ntargets = 5;
};
template <class Fn> static void gargs(const char *id, int want_rc, const char *want_msg, Fn change)
{
    GArgs a;
    change(a);
    g_err[0] = 0;
    MotionPlan pl;
    line(id, ffgpu_motion_gate_args_check("op", a.have_streams ? a.streams.data() : nullptr, a.ntargets, a.have_spec ? &a.spec : nullptr, at(a.state), a.nstreams, at(a.words),
                                          at(a.out_recs), at(a.out_lists), pl), want_rc, want_msg);
}

int main()
{
    const int imin = std::numeric_limits<int>::min(), imax = std::numeric_limits<int>::max();
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();

    // the state's size: per stream a 16-byte header, h rows of ALIGN(w, 8) shorts and 4 bytes per cell rounded up to 16; 0 outside the ranges
    fact("bytes.1x1x1", ffgpu_motion_state_bytes_host(1, 1, 1, 2) == 16 + 16 + 16);
    fact("bytes.3x7x5", ffgpu_motion_state_bytes_host(3, 7, 5, 3) == 3u * (16 + 5 * 16 + 16));
    fact("bytes.2x17x9", ffgpu_motion_state_bytes_host(2, 17, 9, 2) == 2u * (16 + 9 * 48 + 64));                // 5 x 3 cells = 60 bytes -> 64
    fact("bytes.1080p", ffgpu_motion_state_bytes_host(1, 1920, 1080, 4) == 16 + 2u * 1920 * 1080 + 4u * 120 * 68);
    fact("bytes.largest", ffgpu_motion_state_bytes_host(65536, 8192, 8192, 2) == (size_t)65536 * (16 + (size_t)2 * 8192 * 8192 + (size_t)4 * 2048 * 2048));
    fact("bytes.outside", ffgpu_motion_state_bytes_host(0, 1, 1, 2) == 0 && ffgpu_motion_state_bytes_host(65537, 1, 1, 2) == 0 && ffgpu_motion_state_bytes_host(1, 0, 1, 2) == 0 &&
                          ffgpu_motion_state_bytes_host(1, 8193, 1, 2) == 0 && ffgpu_motion_state_bytes_host(1, 1, 0, 2) == 0 && ffgpu_motion_state_bytes_host(1, 1, 8193, 2) == 0 &&
                          ffgpu_motion_state_bytes_host(1, 1, 1, 1) == 0 && ffgpu_motion_state_bytes_host(1, 1, 1, 7) == 0 &&
                          ffgpu_motion_state_bytes_host(imin, imin, imin, imin) == 0 && ffgpu_motion_state_bytes_host(imax, imax, imax, imax) == 0);
    {
        MotionLayout l;
        fact("layout.67x35", ffgpu_motion_layout(67, 35, 3, l) && l.gw == 9 && l.gh == 5 && l.pitch == 72 && l.cells_off == 16 + 2u * 72 * 35 && l.stream_bytes == l.cells_off + 192 &&
                             l.stream_bytes % 16 == 0);
    }

    // the plan of a good spec
    {
        ffgpu_motion_spec sp = good_spec();
        MotionPlan pl;
        g_err[0] = 0;
        line("plan.spec", ffgpu_motion_spec_plan("op", &sp, pl), 0, "");
        fact("plan.spec_values", pl.lay.w == 65 && pl.lay.h == 33 && pl.lay.cell_log2 == 4 && pl.lay.gw == 5 && pl.lay.gh == 3 && pl.lay.pitch == 72 && pl.threshold == 20 &&
                                 pl.learn_shift == 4 && pl.learn_shift_changed == 8 && pl.min_pixels == 16 && pl.cover == 64 && pl.warmup == 30 && pl.invert == 1 &&
                                 pl.min_score == 0.25f && pl.nclasses == 0);
        sp.classes = g_classes; sp.nclasses = 3;
        line("plan.classes", ffgpu_motion_spec_plan("op", &sp, pl), 0, "");
        fact("plan.classes_values", pl.nclasses == 3 && pl.classes[0] == 1 && pl.classes[1] == 0 && pl.classes[2] == 1 && pl.classes[3] == 0);
        line("plan.null_spec", ffgpu_motion_spec_plan("op", nullptr, pl), -1, "NULL spec");
    }

    spec("spec.good", 0, "", [](ffgpu_motion_spec &) {});
    spec("spec.smallest", 0, "", [](ffgpu_motion_spec &s) { s.w = s.h = 1; s.cell_log2 = 2; s.threshold = 1; s.learn_shift = s.learn_shift_changed = 0; s.min_pixels = 1; s.cover = 1; s.warmup = 0; s.flags = 0; });
    spec("spec.largest", 0, "", [](ffgpu_motion_spec &s) { s.w = s.h = 8192; s.cell_log2 = 6; s.threshold = 255; s.learn_shift = s.learn_shift_changed = 16; s.min_pixels = 4096; s.cover = 256; s.warmup = 65535; });
    spec("spec.min_score_nan", 0, "", [&](ffgpu_motion_spec &s) { s.min_score = nan; });
    spec("spec.min_score_inf", 0, "", [&](ffgpu_motion_spec &s) { s.min_score = -inf; });
    spec("spec.classes_256", 0, "", [](ffgpu_motion_spec &s) { static unsigned char big[256]; s.classes = big; s.nclasses = 256; });
    spec("spec.w_0", -1, "a model of 0 x 33 pixels (1..8192 each)", [](ffgpu_motion_spec &s) { s.w = 0; });
    spec("spec.w_8193", -1, "a model of 8193 x 33 pixels", [](ffgpu_motion_spec &s) { s.w = 8193; });
    spec("spec.h_0", -1, "a model of 65 x 0 pixels", [](ffgpu_motion_spec &s) { s.h = 0; });
    spec("spec.h_8193", -1, "a model of 65 x 8193 pixels", [](ffgpu_motion_spec &s) { s.h = 8193; });
    spec("spec.w_min", -1, "a model of", [&](ffgpu_motion_spec &s) { s.w = imin; });
    spec("spec.cell_1", -1, "cell_log2 1 is outside 2..6", [](ffgpu_motion_spec &s) { s.cell_log2 = 1; });
    spec("spec.cell_7", -1, "cell_log2 7 is outside 2..6", [](ffgpu_motion_spec &s) { s.cell_log2 = 7; });
    spec("spec.cell_max", -1, "cell_log2", [&](ffgpu_motion_spec &s) { s.cell_log2 = imax; });
    spec("spec.threshold_0", -1, "threshold 0 is outside 1..255", [](ffgpu_motion_spec &s) { s.threshold = 0; });
    spec("spec.threshold_256", -1, "threshold 256 is outside 1..255", [](ffgpu_motion_spec &s) { s.threshold = 256; });
    spec("spec.learn_neg", -1, "learn_shift -1 is outside 0..16", [](ffgpu_motion_spec &s) { s.learn_shift = -1; });
    spec("spec.learn_17", -1, "learn_shift 17 is outside 0..16", [](ffgpu_motion_spec &s) { s.learn_shift = 17; });
    spec("spec.learn_changed_neg", -1, "learn_shift_changed -1 is outside 0..16", [](ffgpu_motion_spec &s) { s.learn_shift_changed = -1; });
    spec("spec.learn_changed_17", -1, "learn_shift_changed 17 is outside 0..16", [](ffgpu_motion_spec &s) { s.learn_shift_changed = 17; });
    spec("spec.min_pixels_0", -1, "min_pixels 0 is outside 1..256", [](ffgpu_motion_spec &s) { s.min_pixels = 0; });
    spec("spec.min_pixels_257", -1, "min_pixels 257 is outside 1..256", [](ffgpu_motion_spec &s) { s.min_pixels = 257; });
    spec("spec.min_pixels_cell", -1, "min_pixels 17 is outside 1..16", [](ffgpu_motion_spec &s) { s.cell_log2 = 2; s.min_pixels = 17; });
    spec("spec.cover_0", -1, "cover 0 is outside 1..256", [](ffgpu_motion_spec &s) { s.cover = 0; });
    spec("spec.cover_257", -1, "cover 257 is outside 1..256", [](ffgpu_motion_spec &s) { s.cover = 257; });
    spec("spec.warmup_neg", -1, "warmup -1 is outside 0..65535", [](ffgpu_motion_spec &s) { s.warmup = -1; });
    spec("spec.warmup_65536", -1, "warmup 65536 is outside 0..65535", [](ffgpu_motion_spec &s) { s.warmup = 65536; });
    spec("spec.flags_2", -1, "unknown flags 0x2", [](ffgpu_motion_spec &s) { s.flags = 2; });
    spec("spec.flags_min", -1, "unknown flags 0x80000000", [&](ffgpu_motion_spec &s) { s.flags = imin; });
    spec("spec.nclasses_without_classes", -1, "nclasses 3 (0 with NULL classes, else 1..256)", [](ffgpu_motion_spec &s) { s.nclasses = 3; });
    spec("spec.classes_without_nclasses", -1, "nclasses 0", [](ffgpu_motion_spec &s) { s.classes = g_classes; });
    spec("spec.nclasses_257", -1, "nclasses 257", [](ffgpu_motion_spec &s) { s.classes = g_classes; s.nclasses = 257; });
    spec("spec.nclasses_neg", -1, "nclasses -1", [](ffgpu_motion_spec &s) { s.classes = g_classes; s.nclasses = -1; });
    spec("spec.reserved0", -1, "reserved must be 0", [](ffgpu_motion_spec &s) { s.reserved[0] = 1; });
    spec("spec.reserved1", -1, "reserved must be 0", [](ffgpu_motion_spec &s) { s.reserved[1] = -1; });

    for (int nv12 = 0; nv12 < 2; nv12++) {
        const bool n = nv12 != 0;
        uargs(n ? "nv12.good" : "bgr.good", n, 3, "", [](UArgs &) {});
        uargs(n ? "nv12.null_targets" : "bgr.null_targets", n, -1, "NULL targets", [](UArgs &a) { a.have_targets = false; });
        uargs(n ? "nv12.null_streams" : "bgr.null_streams", n, -1, "NULL streams", [](UArgs &a) { a.have_streams = false; });
        uargs(n ? "nv12.null_spec" : "bgr.null_spec", n, -1, "NULL spec", [](UArgs &a) { a.have_spec = false; });
        uargs(n ? "nv12.null_state" : "bgr.null_state", n, -1, "NULL state", [](UArgs &a) { a.state = 0; });
        uargs(n ? "nv12.null_rows" : "bgr.null_rows", n, -1, "NULL rows", [](UArgs &a) { a.rows = 0; });
        uargs(n ? "nv12.threshold_0" : "bgr.threshold_0", n, -1, "threshold 0", [](UArgs &a) { a.spec.threshold = 0; });
        uargs(n ? "nv12.ntargets_0" : "bgr.ntargets_0", n, -1, "0 targets", [](UArgs &a) { a.ntargets = 0; });
        uargs(n ? "nv12.ntargets_neg" : "bgr.ntargets_neg", n, -1, "-1 targets", [](UArgs &a) { a.ntargets = -1; });
        uargs(n ? "nv12.nstreams_0" : "bgr.nstreams_0", n, -1, "nstreams 0", [](UArgs &a) { a.nstreams = 0; });
        uargs(n ? "nv12.nstreams_65537" : "bgr.nstreams_65537", n, -1, "nstreams 65537", [](UArgs &a) { a.nstreams = 65537; });
        uargs(n ? "nv12.state_unaligned" : "bgr.state_unaligned", n, -1, "the state must be 16-byte aligned", [](UArgs &a) { a.state += 8; });
        uargs(n ? "nv12.stream_high" : "bgr.stream_high", n, -1, "target 1: stream 2 is outside -1 .. 1", [](UArgs &a) { a.nstreams = 2; });
        uargs(n ? "nv12.stream_low" : "bgr.stream_low", n, -1, "target 3: stream -2", [](UArgs &a) { a.streams[3] = -2; });
        uargs(n ? "nv12.bad_size" : "bgr.bad_size", n, -1, "target 1: bad size 0 x 33", [](UArgs &a) { a.bgr[1].w = 0; a.nv[1].w = 0; });
        uargs(n ? "nv12.other_w" : "bgr.other_w", n, -1, "target 3: 64 x 33 pixels, the spec's model is 65 x 33", [](UArgs &a) { a.bgr[3].w = 64; a.nv[3].w = 64; });
        uargs(n ? "nv12.other_h" : "bgr.other_h", n, -1, "target 5: 65 x 34 pixels, the spec's model is 65 x 33", [](UArgs &a) { a.bgr[5].h = 34; a.nv[5].h = 34; });
        uargs(n ? "nv12.skipped_other" : "bgr.skipped_other", n, 3, "", [](UArgs &a) { a.bgr[4].h = 1; a.nv[4].h = 1; a.bgr[2].w = 7; a.nv[2].w = 7; });
        uargs(n ? "nv12.target_reserved" : "bgr.target_reserved", n, -1, "target 0: reserved must be 0", [](UArgs &a) { a.bgr[0].reserved = 1; a.nv[0].reserved = 1; });
    }
    uargs("bgr.pitch", false, -1, "target 0: pitch 100 is below 3 w = 195", [](UArgs &a) { a.bgr[0].pitch = 100; });
    uargs("nv12.pitch_y", true, -1, "target 0: pitch_y 10 is below w = 65", [](UArgs &a) { a.nv[0].pitch_y = 10; });
    uargs("nv12.uv_odd", true, -1, "is odd (U V pairs are written", [](UArgs &a) { a.nv[0].uv = (const unsigned char *)at(0x18001); });
    uargs("nv12.matrix", true, -1, "target 1: matrix 4", [](UArgs &a) { a.nv[1].matrix = 4; });

    gargs("gate.good", 0, "", [](GArgs &) {});
    gargs("gate.no_outputs", 0, "", [](GArgs &a) { a.out_recs = 0; a.out_lists = 0; });
    gargs("gate.records_only", 0, "", [](GArgs &a) { a.out_lists = 0; });
    gargs("gate.null_streams", -1, "NULL streams", [](GArgs &a) { a.have_streams = false; });
    gargs("gate.null_spec", -1, "NULL spec", [](GArgs &a) { a.have_spec = false; });
    gargs("gate.null_state", -1, "NULL state", [](GArgs &a) { a.state = 0; });
    gargs("gate.null_words", -1, "NULL words", [](GArgs &a) { a.words = 0; });
    gargs("gate.cover_0", -1, "cover 0", [](GArgs &a) { a.spec.cover = 0; });
    gargs("gate.ntargets_0", -1, "0 targets", [](GArgs &a) { a.ntargets = 0; });
    gargs("gate.nstreams_0", -1, "nstreams 0", [](GArgs &a) { a.nstreams = 0; });
    gargs("gate.nstreams_65537", -1, "nstreams 65537", [](GArgs &a) { a.nstreams = 65537; });
    gargs("gate.state_unaligned", -1, "the state must be 16-byte aligned", [](GArgs &a) { a.state += 4; });
    gargs("gate.stream_high", -1, "target 1: stream 2 is outside -1 .. 1", [](GArgs &a) { a.nstreams = 2; });
    gargs("gate.stream_low", -1, "target 3: stream -2", [](GArgs &a) { a.streams[3] = -2; });
    gargs("gate.lists_without_records", -1, "d_out_lists without d_out_records", [](GArgs &a) { a.out_recs = 0; });

    printf("motion_driver: %d cases, %d wrong\n", g_cases, g_wrong);
    return g_wrong ? 1 : 0;
}
