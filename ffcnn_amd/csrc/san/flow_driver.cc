// flow_driver.cc -- ffgpu_flow_host.hpp on the CPU under AddressSanitizer + UBSan (`make flow`; tests/test_flow_abi.py): the state's layout, the flow
// spec resolved into its plan, the argument checks of the update and of the box operator, and the rounds of an update call, on good and hostile
// arguments.  One line per case: id, return value, message.  The last line is "flow_driver: N cases, 0 wrong".  Nothing of HIP: the addresses are
// made up and never followed.
#include <limits>
#include <string>
#include <vector>
#include "../ffgpu_flow_host.hpp"
#include "driver.hpp"

static const unsigned char g_classes[3] = { 1, 0, 1 };

struct Args {
    std::vector<int> streams{ 0, 2, -1, 0, 1, 0 };
    std::vector<ffgpu_bgr_frame> bgr;
    std::vector<ffgpu_nv12_frame> nv;
    bool have_streams = true, have_spec = true, have_targets = true;
    ffgpu_flow_spec spec;
    uintptr_t state = 0x2000, out = 0x4000;
    int nstreams = 3, ntargets = 6;
    Args() : bgr(6), nv(6)
    {
        memset(&spec, 0, sizeof spec);
        spec.w = 65; spec.h = 33; spec.block_log2 = 4; spec.range = 8; spec.min_spread = 64; spec.min_score = 0.25f;
        for (int k = 0; k < 6; k++) {
            memset(&bgr[k], 0, sizeof bgr[k]); memset(&nv[k], 0, sizeof nv[k]);
            bgr[k].bgr = bytes_at(0x10001 + 0x10000 * k); bgr[k].w = 65; bgr[k].h = 33; bgr[k].pitch = 200;
            nv[k].y = bytes_at(0x10001 + 0x10000 * k); nv[k].uv = bytes_at(0x18000 + 0x10000 * k); nv[k].w = 65; nv[k].h = 33;
        }
        bgr[4].bgr = nullptr; nv[4].y = nullptr;                                   // a skipped target
    }
};
// form 0: the BGR update, 1: the NV12 update, 2: the box operator, 3: the spec alone
template <class Fn> static void run(const char *id, int form, int want_rc, const char *want_msg, Fn change)
{
    Args a;
    change(a);
    g_err[0] = 0;
    FlowPlan pl;
    std::vector<DrawTarget> tab;
    std::vector<int> round;
    const int *st = a.have_streams ? a.streams.data() : nullptr;
    const ffgpu_flow_spec *sp = a.have_spec ? &a.spec : nullptr;
    int rc;
    if (form == 0)      rc = ffgpu_flow_update_args_check("op", a.have_targets ? a.bgr.data() : nullptr, a.ntargets, st, sp, at(a.state), a.nstreams, at(a.out), pl, tab, round);
    else if (form == 1) rc = ffgpu_flow_update_args_check("op", a.have_targets ? a.nv.data() : nullptr, a.ntargets, st, sp, at(a.state), a.nstreams, at(a.out), pl, tab, round);
    else if (form == 2) rc = ffgpu_flow_boxes_args_check("op", st, a.ntargets, sp, at(a.state), a.nstreams, at(a.out), pl);
    else                rc = ffgpu_flow_spec_plan("op", sp, pl);
    line_nonneg(id, rc, want_rc, want_msg);
    if (rc >= 0 && form < 2)                                                       // streams 0 2 -1 0 (1, skipped) 0: three rounds, the skipped ones in round 0
        fact(id, rc == 3 && round == std::vector<int>({ 0, 0, 0, 1, 0, 2 }) && tab[0].p0 && tab[0].first == 0 && !tab[2].p0 && !tab[4].p0 && tab[4].first == 1 &&
                 pl.lay.gw == 5 && pl.lay.gh == 3 && pl.lay.pitch == 80 && pl.range == 8 && pl.min_spread == 64 && pl.min_score == 0.25f);
}

int main()
{
    const int imin = std::numeric_limits<int>::min(), imax = std::numeric_limits<int>::max();
    // the state's size: per stream a 16-byte header, two planes of h rows of ALIGN(w, 16) bytes and 8 bytes per block rounded up to 16; 0 outside the ranges
    fact("bytes.5x3", ffgpu_flow_state_bytes_host(1, 5, 3, 4) == 16 + 2 * 48 + 16);
    fact("bytes.71x37", ffgpu_flow_state_bytes_host(3, 71, 37, 3) == 3u * (16 + 2 * 80 * 37 + 368));        // 9 x 5 blocks = 360 bytes -> 368
    fact("bytes.1080p", ffgpu_flow_state_bytes_host(1, 1920, 1080, 3) == 16 + 2u * 1920 * 1080 + 8u * 240 * 135);
    fact("bytes.largest", ffgpu_flow_state_bytes_host(65536, 8192, 8192, 3) == (size_t)65536 * (16 + (size_t)2 * 8192 * 8192 + (size_t)8 * 1024 * 1024));
    fact("bytes.outside", !ffgpu_flow_state_bytes_host(0, 1, 1, 3) && !ffgpu_flow_state_bytes_host(65537, 1, 1, 3) && !ffgpu_flow_state_bytes_host(1, 0, 1, 3) &&
                          !ffgpu_flow_state_bytes_host(1, 8193, 1, 3) && !ffgpu_flow_state_bytes_host(1, 1, 0, 3) && !ffgpu_flow_state_bytes_host(1, 1, 8193, 3) &&
                          !ffgpu_flow_state_bytes_host(1, 1, 1, 2) && !ffgpu_flow_state_bytes_host(1, 1, 1, 5) && !ffgpu_flow_state_bytes_host(imin, imin, imin, imin) &&
                          !ffgpu_flow_state_bytes_host(imax, imax, imax, imax));

    run("spec.good", 3, 0, "", [](Args &) {});
    run("spec.classes", 3, 0, "", [](Args &a) { a.spec.classes = g_classes; a.spec.nclasses = 3; });
    run("spec.largest", 3, 0, "", [](Args &a) { a.spec.w = a.spec.h = 8192; a.spec.range = 16; a.spec.min_spread = 65535; });
    run("spec.null", 3, -1, "NULL spec", [](Args &a) { a.have_spec = false; });
    run("spec.w_0", 3, -1, "a model of 0 x 33 pixels (1..8192 each)", [](Args &a) { a.spec.w = 0; });
    run("spec.h_8193", 3, -1, "a model of 65 x 8193 pixels", [](Args &a) { a.spec.h = 8193; });
    run("spec.w_min", 3, -1, "a model of", [&](Args &a) { a.spec.w = imin; });
    run("spec.block_2", 3, -1, "block_log2 2 is outside 3..4", [](Args &a) { a.spec.block_log2 = 2; });
    run("spec.block_5", 3, -1, "block_log2 5 is outside 3..4", [](Args &a) { a.spec.block_log2 = 5; });
    run("spec.range_0", 3, -1, "range 0 is outside 1..16", [](Args &a) { a.spec.range = 0; });
    run("spec.range_17", 3, -1, "range 17 is outside 1..16", [](Args &a) { a.spec.range = 17; });
    run("spec.range_max", 3, -1, "range", [&](Args &a) { a.spec.range = imax; });
    run("spec.spread_neg", 3, -1, "min_spread -1 is outside 0..65535", [](Args &a) { a.spec.min_spread = -1; });
    run("spec.spread_65536", 3, -1, "min_spread 65536 is outside 0..65535", [](Args &a) { a.spec.min_spread = 65536; });
    run("spec.flags_1", 3, -1, "unknown flags 0x1", [](Args &a) { a.spec.flags = 1; });
    run("spec.flags_min", 3, -1, "unknown flags 0x80000000", [&](Args &a) { a.spec.flags = imin; });
    run("spec.nclasses_without_classes", 3, -1, "nclasses 3 (0 with NULL classes, else 1..256)", [](Args &a) { a.spec.nclasses = 3; });
    run("spec.nclasses_257", 3, -1, "nclasses 257", [](Args &a) { a.spec.classes = g_classes; a.spec.nclasses = 257; });
    run("spec.reserved0", 3, -1, "reserved must be 0", [](Args &a) { a.spec.reserved[0] = 1; });
    run("spec.reserved5", 3, -1, "reserved must be 0", [](Args &a) { a.spec.reserved[5] = -1; });

    for (int form = 0; form < 3; form++) {
        const std::string f = form == 0 ? "bgr." : form == 1 ? "nv12." : "boxes.";
        auto id = [&](const char *n) { static std::string s; s = f + n; return s.c_str(); };
        run(id("good"), form, form < 2 ? 3 : 0, "", [](Args &) {});
        run(id("null_streams"), form, -1, "NULL streams", [](Args &a) { a.have_streams = false; });
        run(id("null_spec"), form, -1, "NULL spec", [](Args &a) { a.have_spec = false; });
        run(id("null_state"), form, -1, "NULL state", [](Args &a) { a.state = 0; });
        run(id("null_out"), form, -1, form < 2 ? "NULL rows" : "NULL words", [](Args &a) { a.out = 0; });
        run(id("range_0"), form, -1, "range 0", [](Args &a) { a.spec.range = 0; });
        run(id("ntargets_0"), form, -1, "0 targets", [](Args &a) { a.ntargets = 0; });
        run(id("nstreams_65537"), form, -1, "nstreams 65537", [](Args &a) { a.nstreams = 65537; });
        run(id("unaligned"), form, -1, "the state must be 16-byte aligned", [](Args &a) { a.state += 8; });
        run(id("stream_high"), form, -1, "target 1: stream 2 is outside -1 .. 1", [](Args &a) { a.nstreams = 2; });
    }
    run("bgr.null_targets", 0, -1, "NULL targets", [](Args &a) { a.have_targets = false; });
    run("nv12.stream_low", 1, -1, "target 3: stream -2", [](Args &a) { a.streams[3] = -2; });
    run("bgr.bad_size", 0, -1, "target 1: bad size 0 x 33", [](Args &a) { a.bgr[1].w = 0; });
    run("bgr.other_w", 0, -1, "target 3: 64 x 33 pixels, the spec's model is 65 x 33", [](Args &a) { a.bgr[3].w = 64; });
    run("nv12.other_h", 1, -1, "target 5: 65 x 34 pixels, the spec's model is 65 x 33", [](Args &a) { a.nv[5].h = 34; });
    run("nv12.skipped_other", 1, 3, "", [](Args &a) { a.nv[4].h = 1; a.nv[2].w = 7; });
    run("bgr.pitch", 0, -1, "target 0: pitch 100 is below 3 w = 195", [](Args &a) { a.bgr[0].pitch = 100; });
    run("nv12.pitch_y", 1, -1, "target 0: pitch_y 10 is below w = 65", [](Args &a) { a.nv[0].pitch_y = 10; });
    return finish("flow_driver");
}
