// track_driver.cc -- ffgpu_track_host.hpp on the CPU under AddressSanitizer + UBSan (`make track`; tests/test_tracks_abi.py): every rejection of the
// tracker's spec and arguments, the state's size at its limits and outside them, and a launch's entry table (ffgpu_streams_host.hpp, at the tracker's
// 128 records per launch) against its definition.  One line per case: id, return value, message.  The last line is "track_driver: N cases, 0 wrong".
// Nothing of HIP: the addresses are made up and never followed.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <limits>
#include "../ffgpu_track_host.hpp"

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

static ffgpu_track_spec good_spec()
{
    ffgpu_track_spec sp;
    memset(&sp, 0, sizeof sp);
    sp.capacity = 16; sp.max_missed = 2; sp.min_hits = 2; sp.iou_thresh = 0.25f; sp.min_score = 0.125f; sp.birth_score = 0.25f; sp.class_aware = 1;
    return sp;
}
static const void *at(uintptr_t a) { return reinterpret_cast<const void *>(a); }
struct Args {
    std::vector<int> streams{ 0, 2, -1, 1, 0 };
    bool have_streams = true, have_spec = true;
    ffgpu_track_spec spec = good_spec();
    uintptr_t state = 0x2000, ids = 0x3000, orecs = 0x5000, olists = 0x6000;
    int ntargets = 5, nstreams = 3;
};
template <class Fn> static void args(const char *id, int want_rc, const char *want_msg, Fn change)
{
    Args a;
    change(a);
    g_err[0] = 0;
    line(id, ffgpu_track_args_check("op", a.have_streams ? a.streams.data() : nullptr, a.ntargets, a.have_spec ? &a.spec : nullptr, at(a.state), a.nstreams,
                                    at(a.ids), at(a.orecs), at(a.olists)), want_rc, want_msg);
}

// a launch's table against its definition: the groups ascend by stream, a group's entries are its stream's records of the window in record order, every
// record of the window is in exactly one group and carries its own list start; what lies behind the nt entries stays as it was
#define ENTRIES 128                                   // ffgpu_track.inc: TRACK_ARG_ENTRIES
static void entries(const char *id, const std::vector<int> &streams, int t0, int nt)
{
    std::vector<long long> first(streams.size());
    for (size_t t = 0; t < first.size(); t++) first[t] = 1000003LL * (long long)t + 7;
    StreamEntries<ENTRIES> *en = new StreamEntries<ENTRIES>;                          // (on the heap: ASan sees a write behind it)
    memset(en, 0x5a, sizeof *en);
    const int ng = ffgpu_stream_entries(first, streams.data(), t0, nt, *en);
    bool ok = ng >= (nt > 0) && ng <= nt && en->goff[0] == 0 && en->goff[ng] == nt;
    std::vector<char> seen((size_t)nt, 0);
    for (int g = 0; ok && g < ng; g++) {
        ok = en->goff[g] < en->goff[g + 1] && (g == 0 || en->gstream[g - 1] < en->gstream[g]);
        for (int i = en->goff[g]; ok && i < en->goff[g + 1]; i++) {
            const int t = en->rec[i];
            ok = t >= t0 && t < t0 + nt && !seen[t - t0] && streams[t] == en->gstream[g] && (i == en->goff[g] || en->rec[i - 1] < t) && en->first[i] == first[t];
            if (ok) seen[t - t0] = 1;
        }
    }
    for (int i = nt; ok && i < ENTRIES; i++) ok = en->rec[i] == 0x5a5a5a5a && en->first[i] == 0x5a5a5a5a5a5a5a5aLL;
    const int ignored = ng > 0 && en->gstream[0] == -1 ? en->goff[1] : 0;
    delete en;
    g_cases++;
    g_wrong += !ok;
    printf("%s groups=%d ignored=%d%s\n", id, ng, ignored, ok ? "" : "   <-- WRONG");
}

int main()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    args("args.good", 0, "", [](Args &) {});
    args("args.no_outputs", 0, "", [](Args &a) { a.orecs = a.olists = 0; });
    args("args.records_only", 0, "", [](Args &a) { a.olists = 0; });
    args("args.null_streams", -1, "NULL streams", [](Args &a) { a.have_streams = false; });
    args("args.null_spec", -1, "NULL spec", [](Args &a) { a.have_spec = false; });
    args("args.null_state", -1, "NULL state", [](Args &a) { a.state = 0; });
    args("args.null_ids", -1, "NULL ids", [](Args &a) { a.ids = 0; });
    args("args.ntargets_0", -1, "0 targets", [](Args &a) { a.ntargets = 0; });
    args("args.ntargets_neg", -1, "-1 targets", [](Args &a) { a.ntargets = -1; });
    args("args.ntargets_big", -1, "16777217 targets", [](Args &a) { a.ntargets = (1 << 24) + 1; });
    args("args.nstreams_0", -1, "nstreams 0", [](Args &a) { a.nstreams = 0; });
    args("args.nstreams_65537", -1, "nstreams 65537", [](Args &a) { a.nstreams = 65537; });
    args("args.nstreams_65536", 0, "", [](Args &a) { a.nstreams = 65536; });
    args("args.state_unaligned", -1, "16-byte aligned", [](Args &a) { a.state += 8; });
    args("args.lists_without_records", -1, "d_out_lists without d_out_records", [](Args &a) { a.orecs = 0; });
    args("args.stream_high", -1, "target 1: stream 2 is outside -1 .. 1", [](Args &a) { a.nstreams = 2; });
    args("args.stream_low", -1, "target 3: stream -2 is outside -1 .. 2", [](Args &a) { a.streams[3] = -2; });
    args("args.stream_min", -1, "target 0: stream", [](Args &a) { a.streams[0] = std::numeric_limits<int>::min(); });
    // the order of the checks: the spec before the state, the alignment before the lists, the lists before the streams
    args("order.spec_before_state", -1, "capacity 0", [](Args &a) { a.spec.capacity = 0; a.state = 0; });
    args("order.state_before_ids", -1, "NULL state", [](Args &a) { a.state = 0; a.ids = 0; });
    args("order.ids_before_ntargets", -1, "NULL ids", [](Args &a) { a.ids = 0; a.ntargets = 0; });
    args("order.aligned_before_lists", -1, "16-byte aligned", [](Args &a) { a.state += 4; a.orecs = 0; });
    args("order.lists_before_streams", -1, "d_out_lists without d_out_records", [](Args &a) { a.orecs = 0; a.streams[0] = 7; });
    args("spec.capacity_0", -1, "capacity 0 is outside 1..128", [](Args &a) { a.spec.capacity = 0; });
    args("spec.capacity_129", -1, "capacity 129", [](Args &a) { a.spec.capacity = 129; });
    args("spec.capacity_128", 0, "", [](Args &a) { a.spec.capacity = 128; });
    args("spec.capacity_1", 0, "", [](Args &a) { a.spec.capacity = 1; });
    args("spec.max_missed_neg", -1, "max_missed -1", [](Args &a) { a.spec.max_missed = -1; });
    args("spec.max_missed_big", -1, "max_missed 1048577 is outside 0..2^20", [](Args &a) { a.spec.max_missed = (1 << 20) + 1; });
    args("spec.max_missed_top", 0, "", [](Args &a) { a.spec.max_missed = 1 << 20; });
    args("spec.min_hits_0", -1, "min_hits 0", [](Args &a) { a.spec.min_hits = 0; });
    args("spec.min_hits_big", -1, "min_hits 1048577 is outside 1..2^20", [](Args &a) { a.spec.min_hits = (1 << 20) + 1; });
    args("spec.min_hits_top", 0, "", [](Args &a) { a.spec.min_hits = 1 << 20; });
    args("spec.iou_nan", -1, "iou_thresh", [&](Args &a) { a.spec.iou_thresh = nan; });
    args("spec.iou_high", -1, "iou_thresh 1.5 is not in [0, 1]", [](Args &a) { a.spec.iou_thresh = 1.5f; });
    args("spec.iou_neg", -1, "iou_thresh -0.5", [](Args &a) { a.spec.iou_thresh = -0.5f; });
    args("spec.iou_ends", 0, "", [](Args &a) { a.spec.iou_thresh = 1.f; a.spec.min_score = 0.f; a.spec.birth_score = 1.f; });
    args("spec.min_score_inf", -1, "min_score", [&](Args &a) { a.spec.min_score = inf; });
    args("spec.min_score_neg", -1, "min_score -1", [](Args &a) { a.spec.min_score = -1.f; });
    args("spec.birth_score_nan", -1, "birth_score", [&](Args &a) { a.spec.birth_score = nan; });
    args("spec.birth_score_high", -1, "birth_score 2", [](Args &a) { a.spec.birth_score = 2.f; });
    args("spec.class_aware_2", -1, "class_aware 2 is neither 0 nor 1", [](Args &a) { a.spec.class_aware = 2; });
    args("spec.class_aware_neg", -1, "class_aware -1", [](Args &a) { a.spec.class_aware = -1; });
    args("spec.class_aware_0", 0, "", [](Args &a) { a.spec.class_aware = 0; });
    args("spec.reserved", -1, "spec: reserved must be 0", [](Args &a) { a.spec.reserved = 1; });

    const size_t want_bytes[][3] = { { 1, 1, 64 }, { 1, 128, 16 + 48 * 128 }, { 3, 5, 3 * (16 + 240) }, { 65536, 1, (size_t)65536 * 64 },
                                     { 65536, 128, (size_t)65536 * (16 + 48 * 128) }, { 0, 1, 0 }, { 65537, 1, 0 }, { 1, 0, 0 }, { 1, 129, 0 } };
    for (const auto &w : want_bytes) {
        const size_t got = ffgpu_track_state_bytes_host((int)w[0], (int)w[1]);
        g_cases++;
        g_wrong += got != w[2];
        printf("bytes.%zu_%zu %zu%s\n", w[0], w[1], got, got == w[2] ? "" : "   <-- WRONG");
    }
    const int hostile[][2] = { { -1, -1 }, { -1, 5 }, { 5, -1 }, { std::numeric_limits<int>::min(), 1 }, { 1, std::numeric_limits<int>::max() },
                               { std::numeric_limits<int>::max(), std::numeric_limits<int>::max() } };
    for (const auto &h : hostile) {
        const size_t got = ffgpu_track_state_bytes_host(h[0], h[1]);
        g_cases++;
        g_wrong += got != 0;
        printf("bytes.hostile_%d_%d %zu%s\n", h[0], h[1], got, got == 0 ? "" : "   <-- WRONG");
    }

    entries("entries.one", { 0 }, 0, 1);
    entries("entries.mixed", { 2, -1, 0, 2, 1, -1, 0, 2 }, 0, 8);
    entries("entries.window", { 9, 9, 2, -1, 0, 2, 1, 9 }, 2, 5);
    entries("entries.all_ignored", std::vector<int>(40, -1), 0, 40);
    {
        std::vector<int> s(2 * ENTRIES + 3);
        unsigned x = 54321u;
        for (size_t i = 0; i < s.size(); i++) { x = x * 1664525u + 1013904223u; s[i] = (int)((x >> 16) % 70u) - 1; }
        for (int i = 20; i < 50; i++) s[(size_t)i] = -1;                              // a run of ignored entries inside the first chunk
        s[2 * ENTRIES + 1] = -1;                                                      // and one in the tail
        entries("entries.full_0", s, 0, ENTRIES);
        entries("entries.full_1", s, ENTRIES, ENTRIES);
        entries("entries.tail", s, 2 * ENTRIES, 3);
        for (size_t i = 0; i < s.size(); i++) s[i] = (int)i;                          // every record its own stream: as many groups as entries
        entries("entries.all_distinct", s, 1, ENTRIES);
    }
    printf("track_driver: %d cases, %d wrong\n", g_cases, g_wrong);
    return g_wrong ? 1 : 0;
}
