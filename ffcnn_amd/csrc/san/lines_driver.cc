// lines_driver.cc -- ffgpu_lines_host.hpp on the CPU under AddressSanitizer + UBSan (`make lines`; tests/test_outlines_abi.py): the outline spec
// resolved into its plan, and the argument checks of the segment rasteriser and the scene composer on good and hostile arguments.  One line per
// case: id, return value, message.  The last line is "lines_driver: N cases, 0 wrong".  Nothing of HIP: the addresses are made up and never followed.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <limits>
#include "../ffgpu_lines_host.hpp"

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
static const unsigned char g_palette[3 * 4] = { 1, 2, 3, 9, 4, 5, 6, 9, 7, 8, 9, 9 };
static const int ALL = FFGPU_OUTLINE_ZONES | FFGPU_OUTLINE_LINES | FFGPU_OUTLINE_TICKS | FFGPU_OUTLINE_MARKERS | FFGPU_OUTLINE_ALARM;

static ffgpu_outline_spec good_spec()
{
    ffgpu_outline_spec sp;
    memset(&sp, 0, sizeof sp);
    sp.flags = ALL; sp.thickness = 2; sp.line_dash = 3; sp.marker = 4;
    sp.color[0] = 10; sp.color[1] = 20; sp.color[2] = 30; sp.color[3] = 40;
    sp.alarm[0] = 250; sp.alarm[1] = 251; sp.alarm[2] = 252; sp.alarm[3] = 253;
    return sp;
}

template <class Fn> static void spec(const char *id, int want_rc, const char *want_msg, Fn change)
{
    ffgpu_outline_spec sp = good_spec();
    change(sp);
    g_err[0] = 0;
    OutlinePlan pl;
    line(id, ffgpu_outline_spec_plan("op", &sp, pl), want_rc, want_msg);
}

struct Scene {
    std::vector<int> streams{ 0, 2, -1, 1, 0 };
    bool have_streams = true, have_spec = true;
    ffgpu_outline_spec spec = good_spec();
    uintptr_t scenes = 0x1000, state = 0x2000, events = 0x3000, items = 0x4000;
    int nstreams = 3, capacity = 16, events_stride = FFGPU_ZONES_ROW + 2 * 20, ntargets = 5, items_stride = FFGPU_OUTLINE_FIXED;
};
template <class Fn> static void scene(const char *id, int want_rc, const char *want_msg, Fn change)
{
    Scene a;
    change(a);
    g_err[0] = 0;
    OutlinePlan pl;
    line(id, ffgpu_outline_scene_args_check("op", at(a.scenes), at(a.state), a.nstreams, a.capacity, at(a.events), a.events_stride,
                                            a.have_streams ? a.streams.data() : nullptr, a.ntargets, a.have_spec ? &a.spec : nullptr, at(a.items), a.items_stride, pl),
         want_rc, want_msg);
}

struct Segs { uintptr_t items = 0x4000, targets = 0x5000; int items_stride = 512, ntargets = 3; };
template <class Fn> static void segs(const char *id, int want_rc, const char *want_msg, Fn change)
{
    Segs a;
    change(a);
    g_err[0] = 0;
    line(id, ffgpu_draw_segments_args_check("op", at(a.items), a.items_stride, at(a.targets), a.ntargets), want_rc, want_msg);
}

int main()
{
    const int imin = std::numeric_limits<int>::min(), imax = std::numeric_limits<int>::max();

    // the plan of a good spec: the colours packed as the draw's palette entries, byte 3 dropped
    {
        ffgpu_outline_spec sp = good_spec();
        OutlinePlan pl;
        g_err[0] = 0;
        line("plan.color", ffgpu_outline_spec_plan("op", &sp, pl), 0, "");
        fact("plan.color_values", pl.npal == 1 && pl.pal[0] == 0x1e140au && pl.pal[1] == 0 && pl.alarm == 0xfcfbfau && pl.flags == ALL && pl.thickness == 2 &&
                                  pl.line_dash == 3 && pl.marker == 4);
        sp.palette = g_palette; sp.npalette = 3;
        line("plan.palette", ffgpu_outline_spec_plan("op", &sp, pl), 0, "");
        fact("plan.palette_values", pl.npal == 3 && pl.pal[0] == 0x030201u && pl.pal[1] == 0x060504u && pl.pal[2] == 0x090807u && pl.pal[3] == 0);
        line("plan.null_spec", ffgpu_outline_spec_plan("op", nullptr, pl), -1, "NULL spec");
    }

    // every combination of the five flags: legal exactly when a part is named, TICKS has LINES and ALARM has ZONES
    {
        bool all_as_stated = true;
        for (int f = 0; f < 32; f++) {
            ffgpu_outline_spec sp = good_spec();
            sp.flags = f;
            OutlinePlan pl;
            const bool legal = (f & OUTLINE_PARTS) && (!(f & FFGPU_OUTLINE_TICKS) || (f & FFGPU_OUTLINE_LINES)) && (!(f & FFGPU_OUTLINE_ALARM) || (f & FFGPU_OUTLINE_ZONES));
            all_as_stated = all_as_stated && (ffgpu_outline_spec_plan("op", &sp, pl) == 0) == legal;
        }
        fact("spec.every_flag_combination", all_as_stated);
    }
    spec("spec.good", 0, "", [](ffgpu_outline_spec &) {});
    spec("spec.zones_only", 0, "", [](ffgpu_outline_spec &s) { s.flags = FFGPU_OUTLINE_ZONES; s.marker = 0; });
    spec("spec.lines_only", 0, "", [](ffgpu_outline_spec &s) { s.flags = FFGPU_OUTLINE_LINES; });
    spec("spec.markers_only", 0, "", [](ffgpu_outline_spec &s) { s.flags = FFGPU_OUTLINE_MARKERS; s.marker = 1; });
    spec("spec.thickness_8_dash_6_marker_32", 0, "", [](ffgpu_outline_spec &s) { s.thickness = 8; s.line_dash = 6; s.marker = 32; });
    spec("spec.palette_256", 0, "", [](ffgpu_outline_spec &s) { static unsigned char big[1024]; s.palette = big; s.npalette = 256; });
    spec("spec.flags_0", -1, "flags 0x0 name no part (FFGPU_OUTLINE_ZONES | _LINES | _MARKERS)", [](ffgpu_outline_spec &s) { s.flags = 0; });
    spec("spec.flags_ticks_alone", -1, "name no part", [](ffgpu_outline_spec &s) { s.flags = FFGPU_OUTLINE_TICKS; });
    spec("spec.flags_32", -1, "unknown flags 0x21", [](ffgpu_outline_spec &s) { s.flags = 33; });
    spec("spec.flags_min", -1, "unknown flags", [&](ffgpu_outline_spec &s) { s.flags = imin; });
    spec("spec.ticks_without_lines", -1, "FFGPU_OUTLINE_TICKS without FFGPU_OUTLINE_LINES", [](ffgpu_outline_spec &s) { s.flags = FFGPU_OUTLINE_ZONES | FFGPU_OUTLINE_TICKS; });
    spec("spec.alarm_without_zones", -1, "FFGPU_OUTLINE_ALARM without FFGPU_OUTLINE_ZONES", [](ffgpu_outline_spec &s) { s.flags = FFGPU_OUTLINE_LINES | FFGPU_OUTLINE_ALARM; });
    spec("spec.thickness_0", -1, "thickness 0 is outside 1..8", [](ffgpu_outline_spec &s) { s.thickness = 0; });
    spec("spec.thickness_9", -1, "thickness 9 is outside 1..8", [](ffgpu_outline_spec &s) { s.thickness = 9; });
    spec("spec.thickness_max", -1, "thickness", [&](ffgpu_outline_spec &s) { s.thickness = imax; });
    spec("spec.dash_neg", -1, "line_dash -1 is outside 0..6", [](ffgpu_outline_spec &s) { s.line_dash = -1; });
    spec("spec.dash_7", -1, "line_dash 7 is outside 0..6", [](ffgpu_outline_spec &s) { s.line_dash = 7; });
    spec("spec.marker_neg", -1, "marker -1 is outside 0..32", [](ffgpu_outline_spec &s) { s.marker = -1; });
    spec("spec.marker_33", -1, "marker 33 is outside 0..32", [](ffgpu_outline_spec &s) { s.marker = 33; });
    spec("spec.marker_0_with_markers", -1, "marker 0 with FFGPU_OUTLINE_MARKERS (at least 1)", [](ffgpu_outline_spec &s) { s.marker = 0; });
    spec("spec.npalette_without_palette", -1, "npalette 3 (0 with a NULL palette, else 1..256)", [](ffgpu_outline_spec &s) { s.npalette = 3; });
    spec("spec.palette_without_npalette", -1, "npalette 0", [](ffgpu_outline_spec &s) { s.palette = g_palette; });
    spec("spec.npalette_257", -1, "npalette 257", [](ffgpu_outline_spec &s) { s.palette = g_palette; s.npalette = 257; });
    spec("spec.reserved", -1, "reserved must be 0", [](ffgpu_outline_spec &s) { s.reserved = 1; });

    scene("scene.good", 0, "", [](Scene &) {});
    scene("scene.stride_512", 0, "", [](Scene &a) { a.items_stride = 512; });
    scene("scene.events_stride_row", 0, "", [](Scene &a) { a.events_stride = FFGPU_ZONES_ROW; });
    scene("scene.capacity_128", 0, "", [](Scene &a) { a.capacity = 128; });
    scene("scene.null_scenes", -1, "NULL scenes", [](Scene &a) { a.scenes = 0; });
    scene("scene.null_state", -1, "NULL state", [](Scene &a) { a.state = 0; });
    scene("scene.null_events", -1, "NULL events", [](Scene &a) { a.events = 0; });
    scene("scene.null_streams", -1, "NULL streams", [](Scene &a) { a.have_streams = false; });
    scene("scene.null_spec", -1, "NULL spec", [](Scene &a) { a.have_spec = false; });
    scene("scene.null_items", -1, "NULL items", [](Scene &a) { a.items = 0; });
    scene("scene.stride_79", -1, "items_stride 79 is outside 80..512", [](Scene &a) { a.items_stride = 79; });
    scene("scene.stride_513", -1, "items_stride 513 is outside 80..512", [](Scene &a) { a.items_stride = 513; });
    scene("scene.stride_min", -1, "items_stride", [&](Scene &a) { a.items_stride = imin; });
    scene("scene.ntargets_0", -1, "0 targets", [](Scene &a) { a.ntargets = 0; });
    scene("scene.ntargets_neg", -1, "-1 targets", [](Scene &a) { a.ntargets = -1; });
    scene("scene.nstreams_0", -1, "nstreams 0", [](Scene &a) { a.nstreams = 0; });
    scene("scene.nstreams_65537", -1, "nstreams 65537", [](Scene &a) { a.nstreams = 65537; });
    scene("scene.capacity_0", -1, "capacity 0", [](Scene &a) { a.capacity = 0; });
    scene("scene.capacity_129", -1, "capacity 129", [](Scene &a) { a.capacity = 129; });
    scene("scene.events_stride_63", -1, "events_stride 63 is below FFGPU_ZONES_ROW = 64", [](Scene &a) { a.events_stride = 63; });
    scene("scene.events_stride_neg", -1, "events_stride", [](Scene &a) { a.events_stride = -1; });
    scene("scene.stream_high", -1, "target 1: stream 2 is outside -1 .. 1", [](Scene &a) { a.nstreams = 2; });
    scene("scene.stream_low", -1, "target 3: stream -2", [](Scene &a) { a.streams[3] = -2; });
    scene("scene.thickness_9", -1, "thickness 9", [](Scene &a) { a.spec.thickness = 9; });
    scene("scene.flags_0", -1, "name no part", [](Scene &a) { a.spec.flags = 0; });
    scene("scene.npalette", -1, "npalette 2", [](Scene &a) { a.spec.npalette = 2; });
    scene("scene.state_unaligned", -1, "4-byte aligned", [](Scene &a) { a.state += 2; });
    scene("scene.items_unaligned", -1, "items must be 4-byte aligned", [](Scene &a) { a.items += 1; });

    segs("segments.good", 0, "", [](Segs &) {});
    segs("segments.stride_1", 0, "", [](Segs &a) { a.items_stride = 1; });
    segs("segments.null_items", -1, "NULL items", [](Segs &a) { a.items = 0; });
    segs("segments.null_targets", -1, "NULL targets", [](Segs &a) { a.targets = 0; });
    segs("segments.items_unaligned", -1, "4-byte aligned", [](Segs &a) { a.items += 3; });
    segs("segments.stride_0", -1, "items_stride 0 is outside 1..512", [](Segs &a) { a.items_stride = 0; });
    segs("segments.stride_513", -1, "items_stride 513 is outside 1..512", [](Segs &a) { a.items_stride = 513; });
    segs("segments.ntargets_0", -1, "0 targets", [](Segs &a) { a.ntargets = 0; });
    segs("segments.ntargets_neg", -1, "-5 targets", [](Segs &a) { a.ntargets = -5; });

    printf("lines_driver: %d cases, %d wrong\n", g_cases, g_wrong);
    return g_wrong ? 1 : 0;
}
