// zones_driver.cc -- ffgpu_zones_host.hpp on the CPU under AddressSanitizer + UBSan (`make zones`; tests/test_zones_abi.py): the scene check on good and
// hostile scenes, the spec and argument checks, and the grouping of a launch's records by stream against its definition.  One line per case: id, return
// value, message.  The last line is "zones_driver: N cases, 0 wrong".  Nothing of HIP: the addresses are made up and never followed.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <limits>
#include "../ffgpu_zones_host.hpp"

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

static ffgpu_scene good_scene()
{
    ffgpu_scene s;
    memset(&s, 0, sizeof s);
    s.nzones = 2; s.nlines = 1;
    const float sq[4][2] = { { 0, 0 }, { 10, 0 }, { 10, 10 }, { 0, 10 } };
    for (int z = 0; z < 2; z++) {
        s.zone[z].nverts = 4;
        for (int i = 0; i < 4; i++) { s.zone[z].x[i] = sq[i][0] + 20 * z; s.zone[z].y[i] = sq[i][1]; }
        s.zone[z].dwell_frames = 5 * z;
    }
    s.line[0].ax = 0; s.line[0].ay = 5; s.line[0].bx = 30; s.line[0].by = 5;
    return s;
}
template <class Fn> static void scene(const char *id, int want_rc, const char *want_msg, Fn change)
{
    std::vector<ffgpu_scene> v(3, good_scene());
    change(v[1]);
    g_err[0] = 0;
    line(id, ffgpu_scene_check_host(v.data(), 3), want_rc, want_msg);
}

static ffgpu_zones_spec good_spec()
{
    ffgpu_zones_spec sp;
    memset(&sp, 0, sizeof sp);
    sp.capacity = 16; sp.max_missed = 2; sp.identity = FFGPU_ZONES_IDS; sp.min_score = 0.25f; sp.gate_zone = 0xff;
    return sp;
}
static const void *at(uintptr_t a) { return reinterpret_cast<const void *>(a); }
struct Args {
    std::vector<int> streams{ 0, 2, -1, 1, 0 };
    bool have_streams = true, have_spec = true;
    ffgpu_zones_spec spec = good_spec();
    uintptr_t scenes = 0x1000, state = 0x2000, ids = 0x3000, events = 0x4000, orecs = 0x5000, olists = 0x6000;
    int ntargets = 5, nstreams = 3;
};
template <class Fn> static void args(const char *id, int want_rc, const char *want_msg, Fn change)
{
    Args a;
    change(a);
    g_err[0] = 0;
    line(id, ffgpu_zones_args_check("op", a.have_streams ? a.streams.data() : nullptr, a.ntargets, a.have_spec ? &a.spec : nullptr, at(a.scenes), at(a.state),
                                    a.nstreams, at(a.ids), at(a.events), at(a.orecs), at(a.olists)), want_rc, want_msg);
}

// the grouping against its definition: a stable sort by stream, groups of equal streams
static void grouping(const char *id, const std::vector<int> &streams, int t0, int nt)
{
    std::vector<int> order((size_t)nt), gstream((size_t)nt), goff((size_t)nt + 1);   // exactly as long as they may be: ASan sees a write behind them
    const int ng = ffgpu_group_by_stream(streams.data(), t0, nt, order.data(), gstream.data(), goff.data());
    bool ok = ng >= (nt > 0) && ng <= nt && goff[0] == 0 && goff[ng] == nt;
    std::vector<char> seen((size_t)nt, 0);
    for (int g = 0; ok && g < ng; g++) {
        ok = goff[g] < goff[g + 1] && (g == 0 || gstream[g - 1] < gstream[g]);
        for (int i = goff[g]; ok && i < goff[g + 1]; i++) {
            const int t = order[i];
            ok = t >= t0 && t < t0 + nt && !seen[t - t0] && streams[t] == gstream[g] && (i == goff[g] || order[i - 1] < t);
            if (ok) seen[t - t0] = 1;
        }
    }
    g_cases++;
    g_wrong += !ok;
    printf("%s groups=%d%s\n", id, ng, ok ? "" : "   <-- WRONG");
}

int main()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    scene("scene.good", 0, "", [](ffgpu_scene &) {});
    scene("scene.empty", 0, "", [](ffgpu_scene &s) { memset(&s, 0, sizeof s); });
    scene("scene.unused_junk", 0, "", [&](ffgpu_scene &s) { s.zone[5].nverts = -7; s.zone[5].x[0] = nan; s.line[3].ax = inf; s.zone[7].dwell_frames = -1; });
    scene("scene.nzones_9", -1, "scene 1: nzones 9", [](ffgpu_scene &s) { s.nzones = 9; });
    scene("scene.nzones_neg", -1, "scene 1: nzones -1", [](ffgpu_scene &s) { s.nzones = -1; });
    scene("scene.nzones_min", -1, "nzones", [](ffgpu_scene &s) { s.nzones = std::numeric_limits<int>::min(); });
    scene("scene.nlines_9", -1, "scene 1: nlines 9", [](ffgpu_scene &s) { s.nlines = 9; });
    scene("scene.nlines_max", -1, "nlines", [](ffgpu_scene &s) { s.nlines = std::numeric_limits<int>::max(); });
    scene("scene.nverts_2", -1, "zone 1: nverts 2", [](ffgpu_scene &s) { s.zone[1].nverts = 2; });
    scene("scene.nverts_9", -1, "zone 0: nverts 9", [](ffgpu_scene &s) { s.zone[0].nverts = 9; });
    scene("scene.nverts_max", -1, "nverts", [](ffgpu_scene &s) { s.zone[0].nverts = std::numeric_limits<int>::max(); });
    scene("scene.nverts_8", 0, "", [](ffgpu_scene &s) { s.zone[0].nverts = 8; });
    scene("scene.vertex_nan", -1, "zone 1: vertex 2 is not finite", [&](ffgpu_scene &s) { s.zone[1].y[2] = nan; });
    scene("scene.vertex_inf", -1, "zone 0: vertex 3 is not finite", [&](ffgpu_scene &s) { s.zone[0].x[3] = -inf; });
    scene("scene.vertex_unused_nan", 0, "", [&](ffgpu_scene &s) { s.zone[0].x[4] = nan; });
    scene("scene.dwell_neg", -1, "zone 1: negative dwell_frames -3", [](ffgpu_scene &s) { s.zone[1].dwell_frames = -3; });
    scene("scene.zone_reserved", -1, "zone 0: reserved", [](ffgpu_scene &s) { s.zone[0].reserved[1] = 4; });
    scene("scene.line_nan", -1, "line 0 is not finite", [&](ffgpu_scene &s) { s.line[0].by = nan; });
    scene("scene.line_a_is_b", -1, "line 0: A equals B", [](ffgpu_scene &s) { s.line[0].bx = s.line[0].ax; s.line[0].by = s.line[0].ay; });
    scene("scene.anchor_2", -1, "anchor 2", [](ffgpu_scene &s) { s.anchor = 2; });
    scene("scene.anchor_1", 0, "", [](ffgpu_scene &s) { s.anchor = 1; });
    scene("scene.reserved", -1, "scene 1: reserved", [](ffgpu_scene &s) { s.reserved = 1; });
    g_err[0] = 0;
    line("scene.null", ffgpu_scene_check_host(nullptr, 1), -1, "NULL scenes");
    { ffgpu_scene s = good_scene(); g_err[0] = 0; line("scene.n0", ffgpu_scene_check_host(&s, 0), -1, "0 scenes"); }

    args("args.good", 0, "", [](Args &) {});
    args("args.no_outputs", 0, "", [](Args &a) { a.orecs = a.olists = 0; });
    args("args.none_no_ids", 0, "", [](Args &a) { a.spec.identity = FFGPU_ZONES_NONE; a.ids = 0; });
    args("args.type_no_ids", 0, "", [](Args &a) { a.spec.identity = FFGPU_ZONES_TYPE; a.ids = 0; });
    args("args.null_streams", -1, "NULL streams", [](Args &a) { a.have_streams = false; });
    args("args.null_spec", -1, "NULL spec", [](Args &a) { a.have_spec = false; });
    args("args.null_scenes", -1, "NULL scenes", [](Args &a) { a.scenes = 0; });
    args("args.null_state", -1, "NULL state", [](Args &a) { a.state = 0; });
    args("args.null_events", -1, "NULL events", [](Args &a) { a.events = 0; });
    args("args.ids_missing", -1, "NULL ids with identity FFGPU_ZONES_IDS", [](Args &a) { a.ids = 0; });
    args("args.ids_unwanted_none", -1, "ids given without identity FFGPU_ZONES_IDS", [](Args &a) { a.spec.identity = FFGPU_ZONES_NONE; });
    args("args.ids_unwanted_type", -1, "ids given without identity FFGPU_ZONES_IDS", [](Args &a) { a.spec.identity = FFGPU_ZONES_TYPE; });
    args("args.ntargets_0", -1, "0 targets", [](Args &a) { a.ntargets = 0; });
    args("args.ntargets_neg", -1, "-1 targets", [](Args &a) { a.ntargets = -1; });
    args("args.nstreams_0", -1, "nstreams 0", [](Args &a) { a.nstreams = 0; });
    args("args.nstreams_65537", -1, "nstreams 65537", [](Args &a) { a.nstreams = 65537; });
    args("args.stream_high", -1, "target 1: stream 2 is outside -1 .. 1", [](Args &a) { a.nstreams = 2; });
    args("args.stream_low", -1, "target 3: stream -2", [](Args &a) { a.streams[3] = -2; });
    args("args.state_unaligned", -1, "16-byte aligned", [](Args &a) { a.state += 8; });
    args("args.scenes_unaligned", -1, "4-byte aligned", [](Args &a) { a.scenes += 2; });
    args("args.lists_without_records", -1, "d_out_lists without d_out_records", [](Args &a) { a.orecs = 0; });
    args("spec.capacity_0", -1, "capacity 0", [](Args &a) { a.spec.capacity = 0; });
    args("spec.capacity_129", -1, "capacity 129", [](Args &a) { a.spec.capacity = 129; });
    args("spec.capacity_128", 0, "", [](Args &a) { a.spec.capacity = 128; });
    args("spec.max_missed_neg", -1, "max_missed -1", [](Args &a) { a.spec.max_missed = -1; });
    args("spec.max_missed_big", -1, "max_missed", [](Args &a) { a.spec.max_missed = (1 << 20) + 1; });
    args("spec.identity_3", -1, "identity 3", [](Args &a) { a.spec.identity = 3; });
    args("spec.identity_neg", -1, "identity -1", [](Args &a) { a.spec.identity = -1; });
    args("spec.flags_2", -1, "unknown flags 0x2", [](Args &a) { a.spec.flags = 2; });
    args("spec.flags_min", -1, "unknown flags", [](Args &a) { a.spec.flags = std::numeric_limits<int>::min(); });
    args("spec.flags_invert", 0, "", [](Args &a) { a.spec.flags = FFGPU_ZONES_GATE_INVERT; });
    args("spec.min_score_nan", -1, "min_score", [&](Args &a) { a.spec.min_score = nan; });
    args("spec.min_score_high", -1, "min_score", [](Args &a) { a.spec.min_score = 1.5f; });
    args("spec.reserved", -1, "reserved", [](Args &a) { a.spec.reserved = 1; });

    const size_t want_bytes[][3] = { { 1, 1, 208 }, { 1, 128, 144 + 64 * 128 }, { 3, 5, 3 * (144 + 320) }, { 65536, 128, (size_t)65536 * (144 + 64 * 128) },
                                     { 0, 1, 0 }, { 65537, 1, 0 }, { 1, 0, 0 }, { 1, 129, 0 } };
    for (const auto &w : want_bytes) {
        const size_t got = ffgpu_zones_state_bytes_host((int)w[0], (int)w[1]);
        g_cases++;
        g_wrong += got != w[2];
        printf("bytes.%zu_%zu %zu%s\n", w[0], w[1], got, got == w[2] ? "" : "   <-- WRONG");
    }
    g_cases++;
    g_wrong += ffgpu_zones_state_bytes_host(-1, -1) != 0;

    grouping("group.one", { 0 }, 0, 1);
    grouping("group.same", { 4, 4, 4, 4 }, 0, 4);
    grouping("group.mixed", { 2, -1, 0, 2, 1, -1, 0, 2 }, 0, 8);
    grouping("group.window", { 9, 9, 2, -1, 0, 2, 1, 9 }, 2, 5);
    grouping("group.descending", { 5, 4, 3, 2, 1, 0, -1 }, 0, 7);
    {
        std::vector<int> s(2 * ZONES_ARG_ENTRIES + 3);
        unsigned x = 12345u;
        for (size_t i = 0; i < s.size(); i++) { x = x * 1664525u + 1013904223u; s[i] = (int)((x >> 16) % 70u) - 1; }
        grouping("group.full_0", s, 0, ZONES_ARG_ENTRIES);
        grouping("group.full_1", s, ZONES_ARG_ENTRIES, ZONES_ARG_ENTRIES);
        grouping("group.tail", s, 2 * ZONES_ARG_ENTRIES, 3);
        for (size_t i = 0; i < s.size(); i++) s[i] = (int)i;                          // every record its own stream: as many groups as entries
        grouping("group.all_distinct", s, 1, ZONES_ARG_ENTRIES);
    }
    printf("zones_driver: %d cases, %d wrong\n", g_cases, g_wrong);
    return g_wrong ? 1 : 0;
}
