// text_driver.cc -- ffgpu_text_host.hpp on the CPU under AddressSanitizer + UBSan (`make text`; tests/test_captions_abi.py): the built-in font's table
// against the properties include/ffcnn_hip.h states, the caption spec resolved into its plan, and the argument checks of the rasteriser and the two
// composers on good and hostile arguments.  One line per case: id, return value, message.  The last line is "text_driver: N cases, 0 wrong".  Nothing of
// HIP: the addresses are made up and never followed.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <limits>
#include "../ffgpu_text_host.hpp"

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

static ffgpu_caption_spec good_spec()
{
    ffgpu_caption_spec sp;
    memset(&sp, 0, sizeof sp);
    sp.min_score = 0.25f; sp.flags = FFGPU_CAPTION_NAME | FFGPU_CAPTION_SCORE | FFGPU_CAPTION_ID | FFGPU_CAPTION_OPAQUE; sp.identity = FFGPU_ZONES_IDS; sp.scale = 2;
    sp.fg[0] = 250; sp.fg[1] = 251; sp.fg[2] = 252; sp.fg[3] = 253;
    sp.color[0] = 10; sp.color[1] = 20; sp.color[2] = 30; sp.color[3] = 40;
    sp.nnames = 80; sp.d_names = at(0x7000);
    return sp;
}

struct Boxes {
    bool have_spec = true;
    ffgpu_caption_spec spec = good_spec();
    uintptr_t ids = 0x3000, items = 0x4000;
    int items_stride = 32;
};
template <class Fn> static void boxes(const char *id, int want_rc, const char *want_msg, Fn change)
{
    Boxes a;
    change(a);
    g_err[0] = 0;
    CaptionPlan pl;
    line(id, ffgpu_caption_boxes_args_check("op", a.have_spec ? &a.spec : nullptr, at(a.ids), at(a.items), a.items_stride, pl), want_rc, want_msg);
}

struct Scene {
    std::vector<int> streams{ 0, 2, -1, 1, 0 };
    bool have_streams = true, have_spec = true;
    ffgpu_caption_spec spec = good_spec();
    uintptr_t scenes = 0x1000, state = 0x2000, events = 0x3000, items = 0x4000;
    int nstreams = 3, capacity = 16, events_stride = FFGPU_ZONES_ROW + 2 * 20, ntargets = 5, items_stride = 16;
};
template <class Fn> static void scene(const char *id, int want_rc, const char *want_msg, Fn change)
{
    Scene a;
    change(a);
    g_err[0] = 0;
    CaptionPlan pl;
    line(id, ffgpu_caption_scene_args_check("op", at(a.scenes), at(a.state), a.nstreams, a.capacity, at(a.events), a.events_stride,
                                            a.have_streams ? a.streams.data() : nullptr, a.ntargets, a.have_spec ? &a.spec : nullptr, at(a.items), a.items_stride, pl),
         want_rc, want_msg);
}

struct Text { uintptr_t items = 0x4000, targets = 0x5000; int items_stride = 256, ntargets = 3; };
template <class Fn> static void text(const char *id, int want_rc, const char *want_msg, Fn change)
{
    Text a;
    change(a);
    g_err[0] = 0;
    line(id, ffgpu_draw_text_args_check("op", at(a.items), a.items_stride, at(a.targets), a.ntargets), want_rc, want_msg);
}

int main()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();

    // the font: exactly 2 048 bytes are written (ASan sees one more), and the properties of include/ffcnn_hip.h hold
    {
        std::vector<unsigned char> f(2048);
        ffgpu_font_builtin_host(f.data());
        const unsigned char *unknown = f.data() + 8 * 127;
        bool margins = true, space_only = true, distinct = true, others = true, box = true;
        for (int g = 32; g <= 126; g++) {
            bool empty = true;
            for (int r = 0; r < 8; r++) { margins = margins && !(f[g * 8 + r] & 1) && (r < 7 || f[g * 8 + r] == 0); empty = empty && f[g * 8 + r] == 0; }
            space_only = space_only && empty == (g == 32);
            for (int k = 32; k < g; k++) distinct = distinct && memcmp(&f[g * 8], &f[k * 8], 8) != 0;
        }
        for (int g = 0; g < 256; g++)
            if (g < 32 || g > 126) others = others && memcmp(&f[g * 8], unknown, 8) == 0;
        for (int r = 0; r < 7; r++) box = box && unknown[r] == (r == 0 || r == 6 ? 0xf8 : 0x88);
        fact("font.margins_empty", margins);
        fact("font.space_is_the_only_empty_glyph", space_only);
        fact("font.ascii_pairwise_different", distinct);
        fact("font.other_codes_are_the_unknown_glyph", others);
        fact("font.unknown_is_a_hollow_box", box && unknown[7] == 0);
        fact("font.index", ffgpu_font8_index(31) == 95 && ffgpu_font8_index(32) == 0 && ffgpu_font8_index(126) == 94 && ffgpu_font8_index(127) == 95 &&
                           ffgpu_font8_index(-1) == 95 && ffgpu_font8_index(255) == 95);
    }

    // the plan of a good spec: the colours packed as the draw's palette entries, byte 3 dropped
    {
        ffgpu_caption_spec sp = good_spec();
        CaptionPlan pl;
        g_err[0] = 0;
        line("plan.color", ffgpu_caption_spec_check("op", &sp, true, pl), 0, "");
        fact("plan.color_values", pl.npal == 1 && pl.pal[0] == 0x1e140au && pl.pal[1] == 0 && pl.fg == 0xfcfbfau && pl.scale == 2 && pl.nnames == 80 &&
                                  pl.identity == FFGPU_ZONES_IDS && pl.min_score == 0.25f && pl.flags == 15 && pl.d_names == at(0x7000));
        sp.palette = g_palette; sp.npalette = 3;
        line("plan.palette", ffgpu_caption_spec_check("op", &sp, true, pl), 0, "");
        fact("plan.palette_values", pl.npal == 3 && pl.pal[0] == 0x030201u && pl.pal[1] == 0x060504u && pl.pal[2] == 0x090807u && pl.pal[3] == 0);
        sp.min_score = nan; sp.flags = 0; sp.identity = 7; sp.nnames = -1;              // what the scene composer ignores
        line("plan.scene_ignores", ffgpu_caption_spec_check("op", &sp, false, pl), 0, "");
        fact("plan.scene_values", pl.npal == 3 && pl.flags == 0 && pl.nnames == 0 && pl.d_names == nullptr && pl.identity == 0);
    }

    boxes("boxes.good", 0, "", [](Boxes &) {});
    boxes("boxes.none_no_ids", 0, "", [](Boxes &a) { a.spec.identity = FFGPU_ZONES_NONE; a.ids = 0; });
    boxes("boxes.type_no_ids", 0, "", [](Boxes &a) { a.spec.identity = FFGPU_ZONES_TYPE; a.ids = 0; });
    boxes("boxes.no_names", 0, "", [](Boxes &a) { a.spec.nnames = 0; a.spec.d_names = nullptr; });
    boxes("boxes.one_part", 0, "", [](Boxes &a) { a.spec.flags = FFGPU_CAPTION_ID; });
    boxes("boxes.stride_1", 0, "", [](Boxes &a) { a.items_stride = 1; });
    boxes("boxes.stride_256", 0, "", [](Boxes &a) { a.items_stride = 256; });
    boxes("boxes.palette", 0, "", [](Boxes &a) { a.spec.palette = g_palette; a.spec.npalette = 3; });
    boxes("boxes.null_spec", -1, "NULL spec", [](Boxes &a) { a.have_spec = false; });
    boxes("boxes.null_items", -1, "NULL items", [](Boxes &a) { a.items = 0; });
    boxes("boxes.items_unaligned", -1, "items must be 4-byte aligned", [](Boxes &a) { a.items += 2; });
    boxes("boxes.stride_0", -1, "items_stride 0 is outside 1..256", [](Boxes &a) { a.items_stride = 0; });
    boxes("boxes.stride_257", -1, "items_stride 257 is outside 1..256", [](Boxes &a) { a.items_stride = 257; });
    boxes("boxes.stride_min", -1, "items_stride", [](Boxes &a) { a.items_stride = std::numeric_limits<int>::min(); });
    boxes("boxes.min_score_nan", -1, "min_score", [&](Boxes &a) { a.spec.min_score = nan; });
    boxes("boxes.min_score_inf", -1, "min_score", [&](Boxes &a) { a.spec.min_score = inf; });
    boxes("boxes.min_score_neg", -1, "min_score", [](Boxes &a) { a.spec.min_score = -0.5f; });
    boxes("boxes.min_score_high", -1, "min_score", [](Boxes &a) { a.spec.min_score = 1.5f; });
    boxes("boxes.flags_no_part", -1, "name no part", [](Boxes &a) { a.spec.flags = FFGPU_CAPTION_OPAQUE; });
    boxes("boxes.flags_0", -1, "name no part", [](Boxes &a) { a.spec.flags = 0; });
    boxes("boxes.flags_16", -1, "unknown flags 0x11", [](Boxes &a) { a.spec.flags = 17; });
    boxes("boxes.flags_min", -1, "unknown flags", [](Boxes &a) { a.spec.flags = std::numeric_limits<int>::min(); });
    boxes("boxes.identity_3", -1, "identity 3", [](Boxes &a) { a.spec.identity = 3; });
    boxes("boxes.identity_neg", -1, "identity -1", [](Boxes &a) { a.spec.identity = -1; });
    boxes("boxes.scale_0", -1, "scale 0 is outside 1..4", [](Boxes &a) { a.spec.scale = 0; });
    boxes("boxes.scale_5", -1, "scale 5 is outside 1..4", [](Boxes &a) { a.spec.scale = 5; });
    boxes("boxes.npalette_without_palette", -1, "npalette 3", [](Boxes &a) { a.spec.npalette = 3; });
    boxes("boxes.palette_without_npalette", -1, "npalette 0", [](Boxes &a) { a.spec.palette = g_palette; });
    boxes("boxes.npalette_257", -1, "npalette 257", [](Boxes &a) { a.spec.palette = g_palette; a.spec.npalette = 257; });
    boxes("boxes.nnames_neg", -1, "nnames -1", [](Boxes &a) { a.spec.nnames = -1; });
    boxes("boxes.nnames_without_names", -1, "nnames 80", [](Boxes &a) { a.spec.d_names = nullptr; });
    boxes("boxes.names_without_nnames", -1, "nnames 0", [](Boxes &a) { a.spec.nnames = 0; });
    boxes("boxes.ids_missing", -1, "NULL ids with identity FFGPU_ZONES_IDS", [](Boxes &a) { a.ids = 0; });
    boxes("boxes.ids_unwanted_none", -1, "ids given without identity FFGPU_ZONES_IDS", [](Boxes &a) { a.spec.identity = FFGPU_ZONES_NONE; });
    boxes("boxes.ids_unwanted_type", -1, "ids given without identity FFGPU_ZONES_IDS", [](Boxes &a) { a.spec.identity = FFGPU_ZONES_TYPE; });
    boxes("boxes.ids_unaligned", -1, "ids must be 4-byte aligned", [](Boxes &a) { a.ids += 1; });

    scene("scene.good", 0, "", [](Scene &) {});
    scene("scene.spec_parts_ignored", 0, "", [&](Scene &a) { a.spec.flags = 0; a.spec.min_score = nan; a.spec.identity = 9; a.spec.nnames = -4; });
    scene("scene.stride_256", 0, "", [](Scene &a) { a.items_stride = 256; });
    scene("scene.events_stride_row", 0, "", [](Scene &a) { a.events_stride = FFGPU_ZONES_ROW; });
    scene("scene.null_scenes", -1, "NULL scenes", [](Scene &a) { a.scenes = 0; });
    scene("scene.null_state", -1, "NULL state", [](Scene &a) { a.state = 0; });
    scene("scene.null_events", -1, "NULL events", [](Scene &a) { a.events = 0; });
    scene("scene.null_streams", -1, "NULL streams", [](Scene &a) { a.have_streams = false; });
    scene("scene.null_spec", -1, "NULL spec", [](Scene &a) { a.have_spec = false; });
    scene("scene.null_items", -1, "NULL items", [](Scene &a) { a.items = 0; });
    scene("scene.stride_15", -1, "items_stride 15 is outside 16..256", [](Scene &a) { a.items_stride = 15; });
    scene("scene.stride_257", -1, "items_stride 257 is outside 16..256", [](Scene &a) { a.items_stride = 257; });
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
    scene("scene.scale_9", -1, "scale 9", [](Scene &a) { a.spec.scale = 9; });
    scene("scene.npalette", -1, "npalette 2", [](Scene &a) { a.spec.npalette = 2; });
    scene("scene.state_unaligned", -1, "4-byte aligned", [](Scene &a) { a.state += 2; });
    scene("scene.items_unaligned", -1, "items must be 4-byte aligned", [](Scene &a) { a.items += 1; });

    text("text.good", 0, "", [](Text &) {});
    text("text.stride_1", 0, "", [](Text &a) { a.items_stride = 1; });
    text("text.null_items", -1, "NULL items", [](Text &a) { a.items = 0; });
    text("text.null_targets", -1, "NULL targets", [](Text &a) { a.targets = 0; });
    text("text.items_unaligned", -1, "4-byte aligned", [](Text &a) { a.items += 3; });
    text("text.stride_0", -1, "items_stride 0 is outside 1..256", [](Text &a) { a.items_stride = 0; });
    text("text.stride_257", -1, "items_stride 257", [](Text &a) { a.items_stride = 257; });
    text("text.ntargets_0", -1, "0 targets", [](Text &a) { a.ntargets = 0; });
    text("text.ntargets_neg", -1, "-5 targets", [](Text &a) { a.ntargets = -5; });

    printf("text_driver: %d cases, %d wrong\n", g_cases, g_wrong);
    return g_wrong ? 1 : 0;
}
