// streams_driver.cc -- what the per-stream families share, on the CPU under AddressSanitizer + UBSan (`make streams`; tests/test_streams_host.py):
// ffgpu_streams_host.hpp's stream checks and the bytes a reset clears, and ffgpu_args.hpp's colours, palettes and class tables, each rejection with
// its message.  (The grouping's cases are san/zones_driver.cc's, the entry table's san/track_driver.cc's.)  One line per case: id, return value, message
// or result.  The last line is "streams_driver: N cases, 0 wrong".  Nothing of HIP: the addresses are made up and never followed.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include "../ffgpu_streams_host.hpp"
#include "../ffgpu_args.hpp"

static char g_err[512];
extern "C" void ffgpu_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

static int g_cases, g_wrong;
static void line(const char *id, int rc, int want_rc, const char *want_msg, bool also = true)
{
    const bool ok = rc == want_rc && (rc == 0 || strstr(g_err, want_msg)) && also;
    g_cases++;
    g_wrong += !ok;
    printf("%s %d %s%s\n", id, rc, rc ? g_err : "", ok ? "" : "   <-- WRONG");
}
static const void *at(uintptr_t a) { return reinterpret_cast<const void *>(a); }

static void span(const char *id, uintptr_t state, size_t all, int nstreams, int which, int want_rc, const char *want_msg, size_t want_off = 0, size_t want_len = 0)
{
    size_t off = 12345, len = 54321;
    g_err[0] = 0;
    if (!all) ffgpu_set_error("reset: 7 streams of 0 slots");                      // (as a family does before the call)
    const int rc = ffgpu_state_span("reset", at(state), all, nstreams, which, off, len);
    const bool ok = rc == want_rc && (rc ? strstr(g_err, want_msg) && off == 12345 && len == 54321 : off == want_off && len == want_len && off + len <= all);
    g_cases++;
    g_wrong += !ok;
    if (rc) printf("%s %d %s%s\n", id, rc, g_err, ok ? "" : "   <-- WRONG");
    else printf("%s 0 off=%zu len=%zu%s\n", id, off, len, ok ? "" : "   <-- WRONG");
}

int main()
{
    // ntargets, nstreams, the state's alignment: in this order
    struct { const char *id; int nt, ns; uintptr_t st; int rc; const char *msg; } three[] = {
        { "three.good", 5, 3, 0x2000, 0, "" }, { "three.ntargets_1", 1, 1, 0x10, 0, "" }, { "three.limits", 1 << 24, 65536, 0x2000, 0, "" },
        { "three.ntargets_0", 0, 3, 0x2000, -1, "op: 0 targets (ntargets >= 1)" }, { "three.ntargets_neg", -1, 3, 0x2000, -1, "-1 targets" },
        { "three.ntargets_big", (1 << 24) + 1, 3, 0x2000, -1, "16777217 targets" }, { "three.ntargets_min", std::numeric_limits<int>::min(), 3, 0x2000, -1, "targets" },
        { "three.nstreams_0", 5, 0, 0x2000, -1, "op: nstreams 0 is outside 1..65536" }, { "three.nstreams_neg", 5, -4, 0x2000, -1, "nstreams -4" },
        { "three.nstreams_65537", 5, 65537, 0x2000, -1, "nstreams 65537" }, { "three.state_odd", 5, 3, 0x2001, -1, "op: the state must be 16-byte aligned" },
        { "three.state_8", 5, 3, 0x2008, -1, "16-byte aligned" }, { "three.ntargets_first", 0, 0, 0x2001, -1, "0 targets" },
        { "three.nstreams_second", 5, 0, 0x2001, -1, "nstreams 0" },
    };
    for (const auto &c : three) { g_err[0] = 0; line(c.id, ffgpu_streams_check("op", c.nt, c.ns, at(c.st)), c.rc, c.msg); }

    // every target's stream
    struct { const char *id; int s[5]; int ns, rc; const char *msg; } range[] = {
        { "range.good", { 0, 2, -1, 1, 0 }, 3, 0, "" }, { "range.all_ignored", { -1, -1, -1, -1, -1 }, 1, 0, "" }, { "range.top", { 65535, 0, 0, 0, -1 }, 65536, 0, "" },
        { "range.high", { 0, 2, -1, 1, 0 }, 2, -1, "op: target 1: stream 2 is outside -1 .. 1" }, { "range.low", { 0, 2, -1, -2, 0 }, 3, -1, "target 3: stream -2 is outside -1 .. 2" },
        { "range.first_bad", { 3, 4, -2, 1, 0 }, 3, -1, "target 0: stream 3" }, { "range.last_bad", { 0, 0, 0, 0, 1 }, 1, -1, "target 4: stream 1 is outside -1 .. 0" },
        { "range.min", { 0, std::numeric_limits<int>::min(), 0, 0, 0 }, 3, -1, "target 1: stream -2147483648" },
        { "range.max", { 0, 0, std::numeric_limits<int>::max(), 0, 0 }, 65536, -1, "target 2: stream 2147483647" },
    };
    for (const auto &c : range) { g_err[0] = 0; line(c.id, ffgpu_stream_range_check("op", c.s, 5, c.ns), c.rc, c.msg); }
    g_err[0] = 0;
    line("range.none", ffgpu_stream_range_check("op", nullptr, 0, 3), 0, "");                                       // (no target: nothing is read)

    // the bytes a reset clears
    span("span.all", 0x2000, 3 * 256, 3, -1, 0, "", 0, 768);
    span("span.first", 0x2000, 3 * 256, 3, 0, 0, "", 0, 256);
    span("span.last", 0x2000, 3 * 256, 3, 2, 0, "", 512, 256);
    span("span.one_stream", 0x2000, 64, 1, 0, 0, "", 0, 64);
    span("span.one_stream_all", 0x2000, 64, 1, -1, 0, "", 0, 64);
    span("span.which_nstreams", 0x2000, 3 * 256, 3, 3, -1, "reset: stream 3 is outside -1 .. 2");
    span("span.which_m2", 0x2000, 3 * 256, 3, -2, -1, "reset: stream -2 is outside -1 .. 2");
    span("span.which_max", 0x2000, 3 * 256, 3, std::numeric_limits<int>::max(), -1, "stream 2147483647");
    span("span.which_min", 0x2000, 3 * 256, 3, std::numeric_limits<int>::min(), -1, "stream -2147483648");
    span("span.null_state", 0, 3 * 256, 3, -1, -1, "reset: NULL state");
    span("span.odd_state", 0x2001, 3 * 256, 3, -1, -1, "reset: the state must be 16-byte aligned");
    span("span.state_8", 0x2008, 3 * 256, 3, 1, -1, "16-byte aligned");
    span("span.no_size", 0x2000, 0, 7, -1, -1, "reset: 7 streams of 0 slots");
    // the order: NULL, the size, the alignment, the stream
    span("order.null_first", 0, 0, 7, 9, -1, "NULL state");
    span("order.size_second", 0x2001, 0, 7, 9, -1, "7 streams of 0 slots");
    span("order.aligned_third", 0x2001, 3 * 256, 3, 9, -1, "16-byte aligned");
    // totals near SIZE_MAX / 65536: the offset of the last stream and its length stay inside the state
    const size_t big = std::numeric_limits<size_t>::max() / 65536;                    // one stream's bytes, 65536 of them
    span("span.big_all", 0x2000, big * 65536, 65536, -1, 0, "", 0, big * 65536);
    span("span.big_first", 0x2000, big * 65536, 65536, 0, 0, "", 0, big);
    span("span.big_last", 0x2000, big * 65536, 65536, 65535, 0, "", big * 65535, big);
    span("span.big_behind", 0x2000, big * 65536, 65536, 65536, -1, "stream 65536 is outside -1 .. 65535");
    span("span.big_16", 0x2000, (big & ~(size_t)15) * 65536, 65536, 65535, 0, "", (big & ~(size_t)15) * 65535, big & ~(size_t)15);

    // colours
    {
        const unsigned char c[4] = { 0x12, 0x34, 0x56, 0x78 }, hi[3] = { 0xff, 0x80, 0xff };
        const unsigned got = ffgpu_pack_colour(c), got_hi = ffgpu_pack_colour(hi);   // (three bytes are read: ASan watches the fourth of `hi`)
        g_cases += 2;
        g_wrong += (got != 0x563412u) + (got_hi != 0xff80ffu);
        printf("colour.fourth_ignored 0x%06x%s\n", got, got == 0x563412u ? "" : "   <-- WRONG");
        printf("colour.high_bits 0x%06x%s\n", got_hi, got_hi == 0xff80ffu ? "" : "   <-- WRONG");
    }
    // palettes
    {
        unsigned pal[256];
        int npal = -7;
        const unsigned char color[4] = { 1, 2, 3, 99 };
        unsigned char *p256 = (unsigned char *)malloc(1024), *p3 = (unsigned char *)malloc(12);    // exactly as long as they may be read
        for (int i = 0; i < 1024; i++) p256[i] = (unsigned char)(i * 7 + 1);
        for (int i = 0; i < 12; i++) p3[i] = (unsigned char)(0xf0 + i);
        auto rest_zero = [&](int from) { for (int k = from; k < 256; k++) if (pal[k]) return false; return true; };
        memset(pal, 0xee, sizeof pal); g_err[0] = 0;
        int rc = ffgpu_palette_plan("op", nullptr, 0, color, pal, &npal);
        line("palette.single_colour", rc, 0, "", npal == 1 && pal[0] == 0x030201u && rest_zero(1));
        memset(pal, 0xee, sizeof pal); g_err[0] = 0;
        rc = ffgpu_palette_plan("op", p3, 3, color, pal, &npal);
        line("palette.three", rc, 0, "", npal == 3 && pal[0] == 0xf2f1f0u && pal[2] == 0xfaf9f8u && rest_zero(3));
        memset(pal, 0xee, sizeof pal); g_err[0] = 0;
        rc = ffgpu_palette_plan("op", p256, 256, nullptr, pal, &npal);
        bool all = npal == 256;
        for (int k = 0; k < 256; k++) all = all && pal[k] == ((unsigned)p256[4 * k] | (unsigned)p256[4 * k + 1] << 8 | (unsigned)p256[4 * k + 2] << 16);
        line("palette.256_no_colour", rc, 0, "", all);
        struct { const char *id; const unsigned char *p; int n; const char *msg; } bad[] = {
            { "palette.null_with_count", nullptr, 3, "op: npalette 3 (0 with a NULL palette, else 1..256)" }, { "palette.null_with_neg", nullptr, -1, "npalette -1" },
            { "palette.count_0", p3, 0, "npalette 0 (0 with a NULL palette, else 1..256)" }, { "palette.count_neg", p3, -2, "npalette -2" },
            { "palette.count_257", p256, 257, "npalette 257" }, { "palette.count_max", p256, std::numeric_limits<int>::max(), "npalette 2147483647" },
        };
        for (const auto &c : bad) {
            memset(pal, 0xee, sizeof pal); npal = -7; g_err[0] = 0;
            rc = ffgpu_palette_plan("op", c.p, c.n, color, pal, &npal);
            line(c.id, rc, -1, c.msg, npal == -7 && pal[0] == 0xeeeeeeeeu && pal[255] == 0xeeeeeeeeu);              // a rejected palette writes nothing
        }
        free(p256); free(p3);
    }
    // class tables
    {
        unsigned char *c1 = (unsigned char *)malloc(1);
        c1[0] = 1;
        struct { const char *id; const unsigned char *p; int n, rc; const char *msg; } tab[] = {
            { "classes.none", nullptr, 0, 0, "" }, { "classes.one", c1, 1, 0, "" }, { "classes.256", c1, 256, 0, "" },                  // (the table is not read)
            { "classes.null_with_count", nullptr, 80, -1, "op: nclasses 80 (0 with NULL classes, else 1..256)" }, { "classes.null_with_neg", nullptr, -1, -1, "nclasses -1" },
            { "classes.count_0", c1, 0, -1, "nclasses 0 (0 with NULL classes, else 1..256)" }, { "classes.count_neg", c1, -5, -1, "nclasses -5" },
            { "classes.count_257", c1, 257, -1, "nclasses 257" }, { "classes.count_min", c1, std::numeric_limits<int>::min(), -1, "nclasses -2147483648" },
        };
        for (const auto &c : tab) { g_err[0] = 0; line(c.id, ffgpu_class_table_check("op", c.p, c.n), c.rc, c.msg); }
        free(c1);
    }
    printf("streams_driver: %d cases, %d wrong\n", g_cases, g_wrong);
    return g_wrong ? 1 : 0;
}
