// convert_driver.cc -- ffgpu_convert_host.hpp on the CPU under AddressSanitizer + UBSan (`make convert`; tests/test_convert_abi.py): every rejection
// of the convert surfaces on hostile arguments, and the job table of one accepted call per source class.  One line per case: id, return value,
// message.  The last line is "convert_driver: N cases, 0 wrong".  Nothing of HIP: the planes' addresses are made up and never followed.
#include <cstdlib>
#include <vector>
#include "../ffgpu_convert_host.hpp"
#include "driver.hpp"

// a call of four jobs of 70 x 35: surfaces of `format` at odd addresses (even where the format reads pairs) with their planes behind each other, one skipped
struct Call {
    std::vector<ffgpu_surface> s;
    std::vector<ffgpu_bgr_frame> db;
    std::vector<ffgpu_nv12_frame> dn;
    bool have_srcs = true, have_dsts = true;
    int njobs = 4;
    explicit Call(int format) : s(4), db(4), dn(4)
    {
        for (int k = 0; k < 4; k++) {
            memset(&s[k], 0, sizeof s[k]); memset(&db[k], 0, sizeof db[k]); memset(&dn[k], 0, sizeof dn[k]);
            s[k].p[0] = bytes_at(0x100000 + 0x10000 * k + (ffgpu_convert_format(format)->planes == 2 ? 2 : 1)); s[k].w = 70; s[k].h = 35; s[k].format = format; s[k].matrix = k;
            db[k].bgr = bytes_at(0x900003 + 0x10000 * k); db[k].w = 70; db[k].h = 35;
            dn[k].y = bytes_at(0x900003 + 0x10000 * k); dn[k].uv = bytes_at(0x908000 + 0x10000 * k); dn[k].w = 70; dn[k].h = 35;
        }
        s[2].p[0] = nullptr;                                                          // a skipped job
    }
};
template <class Fn> static void call(const char *id, int format, bool nv12, int want_rc, const char *want_msg, Fn change)
{
    Call c(format);
    change(c);
    g_err[0] = 0;
    std::vector<ConvertJob> jobs[CONVERT_NSRC];
    const ffgpu_surface *ss = c.have_srcs ? c.s.data() : nullptr;
    const int rc = nv12 ? ffgpu_convert_args_check("op", ss, c.have_dsts ? c.dn.data() : nullptr, c.njobs, jobs)
                        : ffgpu_convert_args_check("op", ss, c.have_dsts ? c.db.data() : nullptr, c.njobs, jobs);
    line_exact_neg(id, rc, want_rc, want_msg);
    if (rc || want_rc || c.njobs != 4) return;
    // three live jobs, all of the format's class; job 1: the planes behind each other at their least pitches, the destination's defaults resolved
    const ConvertFormat *f = ffgpu_convert_format(format);
    size_t total = 0;
    for (auto &v : jobs) total += v.size();
    bool ok = total == 3 && jobs[f->cls].size() == 3;
    if (ok) {
        const ConvertJob &j = jobs[f->cls][1];
        const int p0 = f->cls == CONVERT_PACKED422 ? 140 : 70 * f->bytes0, p1 = f->cls == CONVERT_PLANAR ? 35 : f->cls == CONVERT_PAIR16 ? 140 : 70;
        ok = j.w == 70 && j.h == 35 && j.fmt == 2 && j.s[0] == c.s[1].p[0] && j.sp[0] == p0 && !j.aligned && j.d[0] == bytes_at(0x910003) && j.dp[0] == (nv12 ? 70 : 212) &&
             j.d[1] == (nv12 ? bytes_at(0x918000) : nullptr) && j.dp[1] == (nv12 ? 70 : 0) && jobs[f->cls][2].s[0] == c.s[3].p[0];
        if (f->planes >= 2) ok = ok && j.s[1 + (format == FFGPU_PIX_YV12)] == j.s[0] + 35 * p0 && j.sp[1] == p1;
        if (f->planes == 3) ok = ok && j.s[format == FFGPU_PIX_YV12 ? 1 : 2] == j.s[0] + 35 * p0 + 18 * 35 && j.sp[2] == 35 && j.sel == 0;
        else ok = ok && j.sel == f->sel && (f->planes == 2 || !j.s[1]) && !j.s[2];
    }
    fact(id, ok);
}

int main()
{
    static const char *const names[12] = { "bgr24", "rgb24", "bgra32", "rgba32", "gray8", "nv12", "nv21", "i420", "yv12", "yuy2", "uyvy", "p010" };
    for (int f = 0; f < 12; f++)
        for (int nv12 = 0; nv12 < 2; nv12++) call(names[f], f, nv12 != 0, 0, "", [](Call &) {});
    // a job whose every address and pitch is a multiple of 4 runs in the aligned form
    call("aligned", FFGPU_PIX_NV12, true, 0, "", [](Call &c) { c.njobs = 1; c.s[0].p[0] = bytes_at(0x100000); c.s[0].w = c.dn[0].w = 72; c.s[0].h = c.dn[0].h = 36; c.dn[0].y = bytes_at(0x900000); });
    {
        Call c(FFGPU_PIX_I420);
        std::vector<ConvertJob> jobs[CONVERT_NSRC];
        c.s[0].p[0] = bytes_at(0x100000); c.s[0].w = c.db[0].w = 72; c.s[0].pitch[1] = c.s[0].pitch[2] = 40; c.db[0].bgr = bytes_at(0x900000);
        fact("aligned", ffgpu_convert_args_check("op", c.s.data(), c.db.data(), 1, jobs) == 0 && jobs[CONVERT_PLANAR].size() == 1 && jobs[CONVERT_PLANAR][0].aligned == 1 &&
                        ffgpu_convert_tiles(jobs[CONVERT_PLANAR].data(), 1) == 5 && CONVERT_TW == 256 && CONVERT_TH == 8 && sizeof(ConvertJob) * CONVERT_ARG_JOBS <= 4096 - 256);
    }
    for (int nv12 = 0; nv12 < 2; nv12++) {
        const bool n = nv12 != 0;
        const int F = FFGPU_PIX_NV12;
        call("null_srcs", F, n, -1, "NULL srcs", [](Call &c) { c.have_srcs = false; });
        call("null_dsts", F, n, -1, "NULL dsts", [](Call &c) { c.have_dsts = false; });
        call("njobs_0", F, n, -1, "0 jobs (1..4096)", [](Call &c) { c.njobs = 0; });
        call("njobs_4097", F, n, -1, "4097 jobs (1..4096)", [](Call &c) { c.njobs = 4097; });
        call("dst_size", F, n, -1, "target 3: bad size 70 x -1", [](Call &c) { c.db[3].h = c.dn[3].h = -1; });
        call("dst_reserved", F, n, -1, "target 1: reserved must be 0", [](Call &c) { c.db[1].reserved = c.dn[1].reserved = 1; });
        call("format_12", F, n, -1, "job 1: format 12 is none of FFGPU_PIX_* (0..11)", [](Call &c) { c.s[1].format = 12; });
        call("format_neg", F, n, -1, "job 0: format -1 is none of", [](Call &c) { c.s[0].format = -1; });
        call("matrix", F, n, -1, "job 3: matrix 4 is none of FFGPU_YUV_* (0..3)", [](Call &c) { c.s[3].matrix = 4; });
        call("reserved", F, n, -1, "job 0: surface: reserved must be 0", [](Call &c) { c.s[0].reserved = 7; });
        call("side", F, n, -1, "job 1: a source of 8193 x 35 (1..8192 each)", [](Call &c) { c.s[1].w = c.db[1].w = c.dn[1].w = 8193; });
        call("side_0", F, n, -1, "job 1: a source of 70 x 0 (1..8192 each)", [](Call &c) { c.s[1].h = 0; });
        call("size", F, n, -1, "job 3: a source of 70 x 36 for a destination of 70 x 35", [](Call &c) { c.s[3].h = 36; });
        call("pitch_low", F, n, -1, "job 0: pitch[0] 69 is below 70", [](Call &c) { c.s[0].pitch[0] = 69; });
        call("pitch_odd", F, n, -1, "job 0: pitch[1] 71 is odd (plane 1 is read as aligned 16-bit values)", [](Call &c) { c.s[0].pitch[1] = 71; });
        call("pitch_422", FFGPU_PIX_YUY2, n, -1, "job 1: pitch[0] 139 is below 140", [](Call &c) { c.s[1].pitch[0] = 139; });
        call("pitch_p010", FFGPU_PIX_P010, n, -1, "job 1: pitch[0] 141 is odd (plane 0", [](Call &c) { c.s[1].pitch[0] = 141; });
        call("pitch_planar", FFGPU_PIX_YV12, n, -1, "job 3: pitch[2] 34 is below 35", [](Call &c) { c.s[3].pitch[2] = 34; });
        call("plane_odd", F, n, -1, "job 0: plane 1's address 0x200001 is odd", [](Call &c) { c.s[0].p[1] = bytes_at(0x200001); });
        call("plane_odd_behind", F, n, -1, "job 1: plane 1's address", [](Call &c) { c.s[1].pitch[0] = 71; });           // (even p[0] + 35 x 71: the plane behind it is odd)
        call("plane_p010", FFGPU_PIX_P010, n, -1, "job 3: plane 0's address 0x130001 is odd", [](Call &c) { c.s[3].p[0] = bytes_at(0x130001); });
        call("unused_plane", F, n, -1, "job 0: p[2] must be NULL: format 5 has 2 planes", [](Call &c) { c.s[0].p[2] = bytes_at(0x300000); });
        call("unused_plane_1", FFGPU_PIX_GRAY8, n, -1, "job 1: p[1] must be NULL: format 4 has 1 plane", [](Call &c) { c.s[1].p[1] = bytes_at(0x300000); });
        call("same", F, n, -1, "job 1: a source plane and a destination plane are the same address 0x910003", [](Call &c) { c.s[1].p[0] = bytes_at(0x910003); c.s[1].p[1] = bytes_at(0x200000); });
        call("same_dst", F, n, -1, "jobs 0 and 3 have the same destination", [](Call &c) { c.db[3].bgr = c.db[0].bgr; c.dn[3].y = c.dn[0].y; });
        call("skipped", F, n, 0, "", [](Call &c) { c.s[2].format = 99; c.s[2].w = -5; c.db[1].bgr = nullptr; c.dn[1].y = nullptr; c.s[1].reserved = 1; c.njobs = 3; });
    }
    call("same_uv", FFGPU_PIX_NV12, true, -1, "job 0: a source plane and a destination plane are the same address 0x908000", [](Call &c) { c.s[0].p[1] = bytes_at(0x908000); });
    call("dst_pitch", FFGPU_PIX_NV12, false, -1, "target 0: pitch 100 is below 3 w = 210", [](Call &c) { c.db[0].pitch = 100; });
    call("dst_uv_odd", FFGPU_PIX_NV12, true, -1, "is odd (U V pairs are written", [](Call &c) { c.dn[1].uv = bytes_at(0x918001); });
    {
        ffgpu_surface s;
        memset(&s, 0, sizeof s);
        s.w = 70; s.h = 35; s.format = FFGPU_PIX_I420; s.pitch[1] = 34;
        g_err[0] = 0;
        line_exact_neg("check.null_p0", ffgpu_convert_check_host("op", &s, 70, 35), -1, "job 0: pitch[1] 34 is below 35");
        s.pitch[1] = 0;
        line_exact_neg("check.null_p0_good", ffgpu_convert_check_host("op", &s, 70, 35), 0, "");
        line_exact_neg("check.null", ffgpu_convert_check_host("op", nullptr, 70, 35), -1, "NULL src");
    }
    return finish("convert_driver");
}
