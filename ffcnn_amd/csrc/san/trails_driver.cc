// trails_driver.cc -- ffgpu_trails_host.hpp on the CPU under AddressSanitizer + UBSan (`make trails`; tests/test_trails_abi.py): the state's size, the
// trails spec resolved into its plan, and the argument checks the operator and the executor form share, on good and hostile arguments.  One line per
// case: id, return value, message.  The last line is "trails_driver: N cases, 0 wrong".  Nothing of HIP: the addresses are made up and never followed.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <limits>
#include "../ffgpu_trails_host.hpp"

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

static ffgpu_trails_spec good_spec()
{
    ffgpu_trails_spec sp;
    memset(&sp, 0, sizeof sp);
    sp.capacity = 16; sp.max_missed = 2; sp.identity = FFGPU_ZONES_IDS; sp.flags = FFGPU_TRAILS_COAST | FFGPU_TRAILS_TAPER; sp.min_score = 0.25f;
    sp.anchor = 1; sp.points = 8; sp.min_move = 3; sp.thickness = 4; sp.coast_dash = 2;
    sp.color[0] = 10; sp.color[1] = 20; sp.color[2] = 30; sp.color[3] = 40;
    return sp;
}

template <class Fn> static void spec(const char *id, int want_rc, const char *want_msg, Fn change)
{
    ffgpu_trails_spec sp = good_spec();
    change(sp);
    g_err[0] = 0;
    TrailsPlan pl;
    line(id, ffgpu_trails_spec_plan("op", &sp, pl), want_rc, want_msg);
}

struct Args {
    std::vector<int> streams{ 0, 2, -1, 1, 0 };
    bool have_streams = true, have_spec = true;
    ffgpu_trails_spec spec = good_spec();
    uintptr_t state = 0x2000, ids = 0x3000, rows = 0x4000, items = 0x5000;
    int nstreams = 3, ntargets = 5, items_stride = 512, first_item = 80, nitems = 432;
};
template <class Fn> static void args(const char *id, int want_rc, const char *want_msg, Fn change)
{
    Args a;
    change(a);
    g_err[0] = 0;
    TrailsPlan pl;
    line(id, ffgpu_trails_args_check("op", a.have_streams ? a.streams.data() : nullptr, a.ntargets, a.have_spec ? &a.spec : nullptr, at(a.state), a.nstreams, at(a.ids),
                                     at(a.rows), at(a.items), a.items_stride, a.first_item, a.nitems, pl),
         want_rc, want_msg);
}

int main()
{
    const int imin = std::numeric_limits<int>::min(), imax = std::numeric_limits<int>::max();
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();

    // the state's size: a 16-byte header and 416 bytes per slot; 0 outside the ranges
    fact("bytes.1x1", ffgpu_trails_state_bytes_host(1, 1) == 432);
    fact("bytes.3x128", ffgpu_trails_state_bytes_host(3, 128) == 3u * (16u + 416u * 128u));
    fact("bytes.65536x128", ffgpu_trails_state_bytes_host(65536, 128) == (size_t)65536 * (16u + 416u * 128u));
    fact("bytes.outside", ffgpu_trails_state_bytes_host(0, 1) == 0 && ffgpu_trails_state_bytes_host(65537, 1) == 0 && ffgpu_trails_state_bytes_host(1, 0) == 0 &&
                          ffgpu_trails_state_bytes_host(1, 129) == 0 && ffgpu_trails_state_bytes_host(imin, imin) == 0 && ffgpu_trails_state_bytes_host(imax, imax) == 0);
    fact("bytes.sixteen", ffgpu_trails_state_bytes_host(7, 5) % 16 == 0 && sizeof(ffgpu_trail_slot) % 16 == 0);

    // the plan of a good spec: the fields copied, the colours packed as the draw's palette entries, byte 3 dropped
    {
        ffgpu_trails_spec sp = good_spec();
        TrailsPlan pl;
        g_err[0] = 0;
        line("plan.color", ffgpu_trails_spec_plan("op", &sp, pl), 0, "");
        fact("plan.color_values", pl.npal == 1 && pl.pal[0] == 0x1e140au && pl.pal[1] == 0 && pl.capacity == 16 && pl.max_missed == 2 && pl.identity == FFGPU_ZONES_IDS &&
                                  pl.flags == 3 && pl.min_score == 0.25f && pl.anchor == 1 && pl.points == 8 && pl.min_move == 3 && pl.thickness == 4 && pl.coast_dash == 2);
        sp.palette = g_palette; sp.npalette = 3;
        line("plan.palette", ffgpu_trails_spec_plan("op", &sp, pl), 0, "");
        fact("plan.palette_values", pl.npal == 3 && pl.pal[0] == 0x030201u && pl.pal[1] == 0x060504u && pl.pal[2] == 0x090807u && pl.pal[3] == 0);
        line("plan.null_spec", ffgpu_trails_spec_plan("op", nullptr, pl), -1, "NULL spec");
    }

    spec("spec.good", 0, "", [](ffgpu_trails_spec &) {});
    spec("spec.type", 0, "", [](ffgpu_trails_spec &s) { s.identity = FFGPU_ZONES_TYPE; });
    spec("spec.smallest", 0, "", [](ffgpu_trails_spec &s) { s.capacity = 1; s.max_missed = 0; s.flags = 0; s.min_score = 0.f; s.anchor = 0; s.points = 2; s.min_move = 0; s.thickness = 1; s.coast_dash = 0; });
    spec("spec.largest", 0, "", [](ffgpu_trails_spec &s) { s.capacity = 128; s.max_missed = 1 << 20; s.min_score = 1.f; s.points = 32; s.min_move = 1 << 20; s.thickness = 8; s.coast_dash = 6; });
    spec("spec.palette_256", 0, "", [](ffgpu_trails_spec &s) { static unsigned char big[1024]; s.palette = big; s.npalette = 256; });
    spec("spec.capacity_0", -1, "capacity 0 is outside 1..128", [](ffgpu_trails_spec &s) { s.capacity = 0; });
    spec("spec.capacity_129", -1, "capacity 129 is outside 1..128", [](ffgpu_trails_spec &s) { s.capacity = 129; });
    spec("spec.capacity_min", -1, "capacity", [&](ffgpu_trails_spec &s) { s.capacity = imin; });
    spec("spec.max_missed_neg", -1, "max_missed -1 is outside 0..2^20", [](ffgpu_trails_spec &s) { s.max_missed = -1; });
    spec("spec.max_missed_big", -1, "max_missed 1048577", [](ffgpu_trails_spec &s) { s.max_missed = (1 << 20) + 1; });
    spec("spec.identity_none", -1, "identity 0 is neither FFGPU_ZONES_TYPE nor _IDS (with _NONE there is nobody to remember)", [](ffgpu_trails_spec &s) { s.identity = FFGPU_ZONES_NONE; });
    spec("spec.identity_3", -1, "identity 3", [](ffgpu_trails_spec &s) { s.identity = 3; });
    spec("spec.identity_neg", -1, "identity -1", [](ffgpu_trails_spec &s) { s.identity = -1; });
    spec("spec.flags_4", -1, "unknown flags 0x4", [](ffgpu_trails_spec &s) { s.flags = 4; });
    spec("spec.flags_min", -1, "unknown flags", [&](ffgpu_trails_spec &s) { s.flags = imin; });
    spec("spec.min_score_nan", -1, "min_score", [&](ffgpu_trails_spec &s) { s.min_score = nan; });
    spec("spec.min_score_inf", -1, "min_score", [&](ffgpu_trails_spec &s) { s.min_score = inf; });
    spec("spec.min_score_neg", -1, "min_score -0.5 is not in [0, 1]", [](ffgpu_trails_spec &s) { s.min_score = -0.5f; });
    spec("spec.min_score_above", -1, "min_score", [](ffgpu_trails_spec &s) { s.min_score = 1.5f; });
    spec("spec.anchor_2", -1, "anchor 2 is neither 0 nor 1", [](ffgpu_trails_spec &s) { s.anchor = 2; });
    spec("spec.anchor_neg", -1, "anchor -1", [](ffgpu_trails_spec &s) { s.anchor = -1; });
    spec("spec.points_1", -1, "points 1 is outside 2..32", [](ffgpu_trails_spec &s) { s.points = 1; });
    spec("spec.points_33", -1, "points 33 is outside 2..32", [](ffgpu_trails_spec &s) { s.points = 33; });
    spec("spec.points_max", -1, "points", [&](ffgpu_trails_spec &s) { s.points = imax; });
    spec("spec.min_move_neg", -1, "min_move -1 is outside 0..2^20", [](ffgpu_trails_spec &s) { s.min_move = -1; });
    spec("spec.min_move_big", -1, "min_move 1048577", [](ffgpu_trails_spec &s) { s.min_move = (1 << 20) + 1; });
    spec("spec.thickness_0", -1, "thickness 0 is outside 1..8", [](ffgpu_trails_spec &s) { s.thickness = 0; });
    spec("spec.thickness_9", -1, "thickness 9 is outside 1..8", [](ffgpu_trails_spec &s) { s.thickness = 9; });
    spec("spec.coast_dash_neg", -1, "coast_dash -1 is outside 0..6", [](ffgpu_trails_spec &s) { s.coast_dash = -1; });
    spec("spec.coast_dash_7", -1, "coast_dash 7 is outside 0..6", [](ffgpu_trails_spec &s) { s.coast_dash = 7; });
    spec("spec.npalette_without_palette", -1, "npalette 3 (0 with a NULL palette, else 1..256)", [](ffgpu_trails_spec &s) { s.npalette = 3; });
    spec("spec.palette_without_npalette", -1, "npalette 0", [](ffgpu_trails_spec &s) { s.palette = g_palette; });
    spec("spec.npalette_257", -1, "npalette 257", [](ffgpu_trails_spec &s) { s.palette = g_palette; s.npalette = 257; });
    spec("spec.reserved", -1, "reserved must be 0", [](ffgpu_trails_spec &s) { s.reserved = 1; });
    spec("spec.reserved0", -1, "reserved must be 0", [](ffgpu_trails_spec &s) { s.reserved0 = -1; });

    args("args.good", 0, "", [](Args &) {});
    args("args.no_items", 0, "", [](Args &a) { a.items = 0; a.items_stride = a.first_item = a.nitems = 0; });
    args("args.one_item", 0, "", [](Args &a) { a.items_stride = 1; a.first_item = 0; a.nitems = 1; });
    args("args.last_item", 0, "", [](Args &a) { a.first_item = 511; a.nitems = 1; });
    args("args.type_without_ids", 0, "", [](Args &a) { a.spec.identity = FFGPU_ZONES_TYPE; a.ids = 0; });
    args("args.null_streams", -1, "NULL streams", [](Args &a) { a.have_streams = false; });
    args("args.null_spec", -1, "NULL spec", [](Args &a) { a.have_spec = false; });
    args("args.null_state", -1, "NULL state", [](Args &a) { a.state = 0; });
    args("args.null_rows", -1, "NULL rows", [](Args &a) { a.rows = 0; });
    args("args.null_ids", -1, "NULL ids with identity FFGPU_ZONES_IDS", [](Args &a) { a.ids = 0; });
    args("args.ids_with_type", -1, "ids given without identity FFGPU_ZONES_IDS", [](Args &a) { a.spec.identity = FFGPU_ZONES_TYPE; });
    args("args.identity_none", -1, "nobody to remember", [](Args &a) { a.spec.identity = FFGPU_ZONES_NONE; a.ids = 0; });
    args("args.points_1", -1, "points 1", [](Args &a) { a.spec.points = 1; });
    args("args.ntargets_0", -1, "0 targets", [](Args &a) { a.ntargets = 0; });
    args("args.ntargets_neg", -1, "-1 targets", [](Args &a) { a.ntargets = -1; });
    args("args.nstreams_0", -1, "nstreams 0", [](Args &a) { a.nstreams = 0; });
    args("args.nstreams_65537", -1, "nstreams 65537", [](Args &a) { a.nstreams = 65537; });
    args("args.state_unaligned", -1, "the state must be 16-byte aligned", [](Args &a) { a.state += 8; });
    args("args.stream_high", -1, "target 1: stream 2 is outside -1 .. 1", [](Args &a) { a.nstreams = 2; });
    args("args.stream_low", -1, "target 3: stream -2", [](Args &a) { a.streams[3] = -2; });
    args("args.null_items_stride", -1, "NULL items with items_stride 512, first_item 0, nitems 0", [](Args &a) { a.items = 0; a.first_item = a.nitems = 0; });
    args("args.null_items_first", -1, "NULL items with items_stride 0, first_item 1, nitems 0", [](Args &a) { a.items = 0; a.items_stride = a.nitems = 0; a.first_item = 1; });
    args("args.null_items_nitems", -1, "NULL items with items_stride 0, first_item 0, nitems 4", [](Args &a) { a.items = 0; a.items_stride = a.first_item = 0; a.nitems = 4; });
    args("args.items_unaligned", -1, "the items must be 4-byte aligned", [](Args &a) { a.items += 2; });
    args("args.stride_0", -1, "items_stride 0 is outside 1..512", [](Args &a) { a.items_stride = 0; });
    args("args.stride_513", -1, "items_stride 513 is outside 1..512", [](Args &a) { a.items_stride = 513; });
    args("args.first_neg", -1, "negative first_item -1", [](Args &a) { a.first_item = -1; });
    args("args.nitems_0", -1, "nitems 0 (at least 1)", [](Args &a) { a.nitems = 0; });
    args("args.nitems_neg", -1, "nitems -3", [](Args &a) { a.nitems = -3; });
    args("args.range_over", -1, "items 80 .. 512 lie outside a row of items_stride 512", [](Args &a) { a.nitems = 433; });
    args("args.range_overflow", -1, "lie outside a row", [&](Args &a) { a.first_item = imax; a.nitems = imax; });

    printf("trails_driver: %d cases, %d wrong\n", g_cases, g_wrong);
    return g_wrong ? 1 : 0;
}
