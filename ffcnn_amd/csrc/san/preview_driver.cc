// preview_driver.cc -- ffgpu_preview_host.hpp on the CPU under AddressSanitizer + UBSan (`make preview`; tests/test_preview_abi.py): the preview spec,
// a pane resolved into its region, image and bars, the wall's layout, the argument checks with the overlap test and the planes of a call, on good and
// hostile arguments.  One line per case: id, return value, message.  The last line is "preview_driver: N cases, 0 wrong".  Nothing of HIP: the
// addresses are made up and never followed.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <limits>
#include "../ffgpu_preview_host.hpp"

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

static const unsigned char *at(uintptr_t a) { return reinterpret_cast<const unsigned char *>(a); }

static ffgpu_preview_spec good_spec()
{
    ffgpu_preview_spec sp;
    memset(&sp, 0, sizeof sp);
    sp.fit = FFGPU_PREVIEW_FIT; sp.fill[0] = 10; sp.fill[1] = 20; sp.fill[2] = 30;
    return sp;
}
template <class Fn> static void spec(const char *id, int want_rc, const char *want_msg, Fn change)
{
    ffgpu_preview_spec sp = good_spec();
    change(sp);
    g_err[0] = 0;
    line(id, ffgpu_preview_spec_check_host("op", &sp), want_rc, want_msg);
}

// resolve of one pane of a 100 x 60 frame into a 50 x 40 surface
static bool rect(const char *id, int fit, bool nv12, ffgpu_preview_pane p, int want_rc, const char *want_msg, std::vector<int> want = {})
{
    ffgpu_preview_spec sp = good_spec();
    sp.fit = fit;
    int out[8] = { 0 };
    g_err[0] = 0;
    const int rc = ffgpu_preview_rect_host("op", 100, 60, 50, 40, &p, &sp, nv12, out);
    line(id, rc, want_rc, want_msg);
    if (rc == 0 && !want.empty()) fact(id, std::vector<int>(out, out + 8) == want);
    return rc == 0;
}

// a call of four panes: three sources into one wall of 40 x 30, and one skipped
struct Call {
    std::vector<ffgpu_bgr_frame> sb, db;
    std::vector<ffgpu_nv12_frame> sn, dn;
    std::vector<ffgpu_preview_pane> panes;
    ffgpu_preview_spec spec = good_spec();
    bool have_srcs = true, have_dsts = true, have_panes = true, have_spec = true;
    int npanes = 4;
    Call()
    {
        sb.resize(4); db.resize(4); sn.resize(4); dn.resize(4); panes.resize(4);
        for (int k = 0; k < 4; k++) {
            memset(&sb[k], 0, sizeof sb[k]); memset(&db[k], 0, sizeof db[k]); memset(&sn[k], 0, sizeof sn[k]); memset(&dn[k], 0, sizeof dn[k]);
            memset(&panes[k], 0, sizeof panes[k]);
            sb[k].bgr = at(0x10001 + 0x10000 * k); sb[k].w = 64 + k; sb[k].h = 48; sb[k].pitch = 3 * (64 + k) + 5;
            sn[k].y = at(0x10001 + 0x10000 * k); sn[k].uv = at(0x18000 + 0x10000 * k); sn[k].w = 64 + k; sn[k].h = 48;
            db[k].bgr = at(0x90003); db[k].w = 40; db[k].h = 30;
            dn[k].y = at(0x90003); dn[k].uv = at(0x98000); dn[k].w = 40; dn[k].h = 30;
            panes[k].dx = 20 * (k & 1); panes[k].dy = 16 * (k >> 1); panes[k].dw = 18; panes[k].dh = 14;
        }
        sb[2].bgr = nullptr; sn[2].y = nullptr;                                      // a skipped pane
        panes[1].sx = 2; panes[1].sy = 4; panes[1].sw = 31; panes[1].sh = 17;
    }
};
template <class Fn> static void call(const char *id, bool nv12, int want_rc, const char *want_msg, Fn change)
{
    Call c;
    change(c);
    g_err[0] = 0;
    std::vector<PreviewJob> jobs[2];
    int rc;
    const ffgpu_preview_pane *pp = c.have_panes ? c.panes.data() : nullptr;
    const ffgpu_preview_spec *sp = c.have_spec ? &c.spec : nullptr;
    if (nv12) rc = ffgpu_preview_args_check("op", c.have_srcs ? c.sn.data() : nullptr, c.have_dsts ? c.dn.data() : nullptr, pp, c.npanes, sp, jobs);
    else      rc = ffgpu_preview_args_check("op", c.have_srcs ? c.sb.data() : nullptr, c.have_dsts ? c.db.data() : nullptr, pp, c.npanes, sp, jobs);
    line(id, rc, want_rc, want_msg);
    if (rc == 0 && want_rc == 0 && c.npanes == 4) {                                  // three live panes; NV12: a U V plane of half the size for each
        bool ok = jobs[0].size() == 3 && jobs[1].size() == (nv12 ? 3u : 0u) && jobs[0][0].pane == 0 && jobs[0][1].pane == 1 && jobs[0][2].pane == 3;
        if (ok) {
            const PreviewJob &j = jobs[0][1];
            ok = j.sx == 2 && j.sy == 4 && j.sw == 31 && j.sh == 17 && j.px == 20 && j.py == 0 && j.pw == 18 && j.ph == 14 && j.ow >= 1 && j.ow <= 18 && j.oh >= 1 && j.oh <= 14 &&
                 j.ix >= j.px && j.ix + j.ow <= j.px + j.pw && j.iy >= j.py && j.iy + j.oh <= j.py + j.ph && j.srow == (nv12 ? 65 : 195) && j.spitch == (nv12 ? 65 : 200) &&
                 j.fill == (nv12 ? 10u : 10u | 20u << 8 | 30u << 16);
            if (ok && nv12) {
                const PreviewJob &u = jobs[1][1];
                ok = u.sx == 1 && u.sy == 2 && u.sw == 16 && u.sh == 9 && u.px == 10 && u.py == 0 && u.pw == 9 && u.ph == 7 && u.ix == j.ix / 2 && u.iy == j.iy / 2 &&
                     u.ow == (j.ow + 1) / 2 && u.oh == (j.oh + 1) / 2 && u.srow == 66 && u.spitch == 66 && u.dpitch == 40 && u.fill == (20u | 30u << 8) && !(j.ix & 1) && !(j.iy & 1);
            }
        }
        fact(id, ok);
    }
}

int main()
{
    const int imin = std::numeric_limits<int>::min(), imax = std::numeric_limits<int>::max();

    spec("spec.good", 0, "", [](ffgpu_preview_spec &) {});
    spec("spec.stretch_keep", 0, "", [](ffgpu_preview_spec &s) { s.fit = FFGPU_PREVIEW_STRETCH; s.flags = FFGPU_PREVIEW_KEEP_BARS; });
    spec("spec.fit_2", -1, "fit 2 is neither FFGPU_PREVIEW_STRETCH nor FFGPU_PREVIEW_FIT", [](ffgpu_preview_spec &s) { s.fit = 2; });
    spec("spec.fit_neg", -1, "fit -1 is neither", [](ffgpu_preview_spec &s) { s.fit = -1; });
    spec("spec.fit_min", -1, "is neither", [&](ffgpu_preview_spec &s) { s.fit = imin; });
    spec("spec.flags_2", -1, "unknown flags 0x2", [](ffgpu_preview_spec &s) { s.flags = 2; });
    spec("spec.flags_min", -1, "unknown flags 0x80000000", [&](ffgpu_preview_spec &s) { s.flags = imin; });
    spec("spec.fill3", -1, "fill[3] must be 0", [](ffgpu_preview_spec &s) { s.fill[3] = 1; });
    spec("spec.reserved", -1, "reserved must be 0", [](ffgpu_preview_spec &s) { s.reserved = 1; });
    g_err[0] = 0;
    line("spec.null", ffgpu_preview_spec_check_host("op", nullptr), -1, "NULL spec");

    // resolve: 100 x 60 into 50 x 40
    rect("rect.default_stretch", 0, false, { 0, 0, 0, 0, 0, 0, 0, 0 }, 0, "", { 0, 0, 100, 60, 0, 0, 50, 40 });
    rect("rect.default_fit", 1, false, { 0, 0, 0, 0, 0, 0, 0, 0 }, 0, "", { 0, 0, 100, 60, 0, 5, 50, 30 });                       // 100 x 60 is wider than 50 x 40
    rect("rect.fit_tall", 1, false, { 3, 5, 10, 50, 1, 1, 40, 30 }, 0, "", { 3, 5, 10, 50, 18, 1, 6, 30 });
    rect("rect.fit_clamp", 1, false, { 0, 7, 100, 1, 2, 2, 8, 8 }, 0, "", { 0, 7, 100, 1, 2, 5, 8, 1 });                         // 100 x 1 into 8 x 8: oh clamps to 1
    rect("rect.fit_nv12_even", 1, true, { 0, 0, 100, 60, 0, 0, 50, 36 }, 0, "", { 0, 0, 100, 60, 0, 2, 50, 30 });                // oy = 3 rounded down to 2
    rect("rect.half_src", 0, false, { 0, 0, 10, 0, 0, 0, 0, 0 }, -1, "pane 0: a source region of 10 x 0 (both 0 for the whole frame, or neither)");
    rect("rect.half_dst", 0, false, { 0, 0, 0, 0, 0, 0, 0, 9 }, -1, "pane 0: a pane of 0 x 9 (both 0 for the whole surface, or neither)");
    rect("rect.default_src_origin", 0, false, { 1, 0, 0, 0, 0, 0, 0, 0 }, -1, "the whole frame as the source region wants sx = sy = 0, not (1, 0)");
    rect("rect.default_dst_origin", 0, false, { 0, 0, 0, 0, 0, 2, 0, 0 }, -1, "the whole surface as the pane wants dx = dy = 0, not (0, 2)");
    rect("rect.src_outside", 0, false, { 91, 0, 10, 10, 0, 0, 0, 0 }, -1, "the source region 10 x 10 at (91, 0) is outside the frame of 100 x 60");
    rect("rect.src_neg", 0, false, { 0, -1, 10, 10, 0, 0, 0, 0 }, -1, "the source region 10 x 10 at (0, -1) is outside the frame");
    rect("rect.src_max", 0, false, { imax, imax, 10, 10, 0, 0, 0, 0 }, -1, "is outside the frame");
    rect("rect.dst_outside", 0, false, { 0, 0, 0, 0, 0, 31, 10, 10 }, -1, "the pane 10 x 10 at (0, 31) is outside the surface of 50 x 40");
    rect("rect.dst_neg", 0, false, { 0, 0, 0, 0, -2, 0, 10, 10 }, -1, "the pane 10 x 10 at (-2, 0) is outside the surface");
    rect("rect.src_side_neg", 0, false, { 0, 0, -5, 10, 0, 0, 0, 0 }, -1, "a source region of -5 x 10 (1..8192 each)");
    rect("rect.dst_side_big", 0, false, { 0, 0, 0, 0, 0, 0, 8193, 1 }, -1, "a pane of 8193 x 1 (1..8192 each)");
    rect("rect.nv12_odd_sx", 0, true, { 1, 0, 10, 10, 0, 0, 0, 0 }, -1, "NV12 wants even sx, sy, dx, dy, not (1, 0) and (0, 0)");
    rect("rect.nv12_odd_dy", 0, true, { 0, 0, 10, 10, 2, 3, 10, 10 }, -1, "NV12 wants even sx, sy, dx, dy, not (0, 0) and (2, 3)");
    {
        ffgpu_preview_spec sp = good_spec();
        ffgpu_preview_pane p;
        memset(&p, 0, sizeof p);
        int out[8];
        g_err[0] = 0;
        line("rect.side_8193", ffgpu_preview_rect_host("op", 8193, 10, 50, 40, &p, &sp, 0, out), -1, "a source region of 8193 x 10 (1..8192 each)");
        line("rect.side_8192", ffgpu_preview_rect_host("op", 8192, 8192, 8192, 8192, &p, &sp, 0, out), 0, "");
        fact("rect.side_8192", out[2] == 8192 && out[6] == 8192 && out[7] == 8192);
        line("rect.one", ffgpu_preview_rect_host("op", 1, 1, 1, 1, &p, &sp, 1, out), 0, "");
        fact("rect.one", out[2] == 1 && out[3] == 1 && out[4] == 0 && out[5] == 0 && out[6] == 1 && out[7] == 1);
        line("rect.null_pane", ffgpu_preview_rect_host("op", 1, 1, 1, 1, nullptr, &sp, 0, out), -1, "NULL pane");
        line("rect.null_out", ffgpu_preview_rect_host("op", 1, 1, 1, 1, &p, &sp, 0, nullptr), -1, "NULL out");
        line("rect.null_spec", ffgpu_preview_rect_host("op", 1, 1, 1, 1, &p, nullptr, 0, out), -1, "NULL spec");
        line("rect.no_frame", ffgpu_preview_rect_host("op", 0, 1, 1, 1, &p, &sp, 0, out), -1, "a frame of 0 x 1 into a surface of 1 x 1");
        sp.fit = 7;
        line("rect.bad_fit", ffgpu_preview_rect_host("op", 1, 1, 1, 1, &p, &sp, 0, out), -1, "fit 7 is neither");
    }

    // the grid
    {
        ffgpu_preview_pane g[8];
        memset(g, 0xff, sizeof g);
        g_err[0] = 0;
        line("grid.2x3", ffgpu_preview_grid_host("op", 6, 2, 97, 61, 2, 0, g), 0, "");
        fact("grid.2x3", g[0].dx == 2 && g[0].dy == 2 && g[0].dw == 45 && g[0].dh == 17 && g[5].dx == 49 && g[5].dy == 40 && g[5].sx == 0 && g[5].sw == 0 && g[5].sh == 0);
        line("grid.nv12", ffgpu_preview_grid_host("op", 5, 3, 97, 61, 2, 1, g), 0, "");
        fact("grid.nv12", g[4].dx == 32 && g[4].dy == 30 && g[4].dw == 28 && g[4].dh == 26);                                      // cw 29 -> 28, ch 27 -> 26
        line("grid.one", ffgpu_preview_grid_host("op", 1, 1, 1, 1, 0, 0, g), 0, "");
        line("grid.npanes_0", ffgpu_preview_grid_host("op", 0, 1, 10, 10, 0, 0, g), -1, "0 panes in 1 columns");
        line("grid.cols_0", ffgpu_preview_grid_host("op", 4, 0, 10, 10, 0, 0, g), -1, "4 panes in 0 columns");
        line("grid.cols_above", ffgpu_preview_grid_host("op", 4, 5, 10, 10, 0, 0, g), -1, "4 panes in 5 columns");
        line("grid.gap_neg", ffgpu_preview_grid_host("op", 4, 2, 10, 10, -1, 0, g), -1, "gap -1 (from 0)");
        line("grid.gap_odd_nv12", ffgpu_preview_grid_host("op", 4, 2, 10, 10, 1, 1, g), -1, "gap 1 (from 0, even for NV12)");
        line("grid.no_room", ffgpu_preview_grid_host("op", 4, 2, 10, 10, 4, 0, g), -1, "2 x 2 panes with gap 4 leave no room in 10 x 10");
        line("grid.no_room_nv12", ffgpu_preview_grid_host("op", 4, 2, 3, 10, 0, 1, g), -1, "leave no room in 3 x 10");
        line("grid.gap_max", ffgpu_preview_grid_host("op", 4, 2, 10, 10, imax, 0, g), -1, "leave no room");
        line("grid.null_out", ffgpu_preview_grid_host("op", 4, 2, 10, 10, 0, 0, nullptr), -1, "NULL out");
    }

    for (int nv12 = 0; nv12 < 2; nv12++) {
        const bool n = nv12 != 0;
        call(n ? "nv12.good" : "bgr.good", n, 0, "", [](Call &) {});
        call(n ? "nv12.null_srcs" : "bgr.null_srcs", n, -1, "NULL srcs", [](Call &c) { c.have_srcs = false; });
        call(n ? "nv12.null_dsts" : "bgr.null_dsts", n, -1, "NULL dsts", [](Call &c) { c.have_dsts = false; });
        call(n ? "nv12.null_panes" : "bgr.null_panes", n, -1, "NULL panes", [](Call &c) { c.have_panes = false; });
        call(n ? "nv12.null_spec" : "bgr.null_spec", n, -1, "NULL spec", [](Call &c) { c.have_spec = false; });
        call(n ? "nv12.npanes_0" : "bgr.npanes_0", n, -1, "0 panes (1..4096)", [](Call &c) { c.npanes = 0; });
        call(n ? "nv12.npanes_4097" : "bgr.npanes_4097", n, -1, "4097 panes (1..4096)", [](Call &c) { c.npanes = 4097; });
        call(n ? "nv12.npanes_min" : "bgr.npanes_min", n, -1, "panes (1..4096)", [&](Call &c) { c.npanes = imin; });
        call(n ? "nv12.fit" : "bgr.fit", n, -1, "fit 3 is neither", [](Call &c) { c.spec.fit = 3; });
        call(n ? "nv12.flags" : "bgr.flags", n, -1, "unknown flags 0x4", [](Call &c) { c.spec.flags = 4; });
        call(n ? "nv12.fill3" : "bgr.fill3", n, -1, "fill[3] must be 0", [](Call &c) { c.spec.fill[3] = 9; });
        call(n ? "nv12.reserved" : "bgr.reserved", n, -1, "spec: reserved must be 0", [](Call &c) { c.spec.reserved = -1; });
        call(n ? "nv12.src_size" : "bgr.src_size", n, -1, "source 1: bad size 0 x 48", [](Call &c) { c.sb[1].w = 0; c.sn[1].w = 0; });
        call(n ? "nv12.dst_size" : "bgr.dst_size", n, -1, "destination 3: bad size 40 x -1", [](Call &c) { c.db[3].h = -1; c.dn[3].h = -1; });
        call(n ? "nv12.src_reserved" : "bgr.src_reserved", n, -1, "source 0: reserved must be 0", [](Call &c) { c.sb[0].reserved = 1; c.sn[0].reserved = 1; });
        call(n ? "nv12.dst_reserved" : "bgr.dst_reserved", n, -1, "destination 1: reserved must be 0", [](Call &c) { c.db[1].reserved = 1; c.dn[1].reserved = 1; });
        call(n ? "nv12.half_src" : "bgr.half_src", n, -1, "pane 1: a source region of 31 x 0", [](Call &c) { c.panes[1].sh = 0; });
        call(n ? "nv12.half_dst" : "bgr.half_dst", n, -1, "pane 3: a pane of 0 x 14", [](Call &c) { c.panes[3].dw = 0; });
        call(n ? "nv12.src_outside" : "bgr.src_outside", n, -1, "pane 1: the source region 31 x 17 at (40, 4) is outside the frame of 65 x 48", [](Call &c) { c.panes[1].sx = 40; });
        call(n ? "nv12.dst_outside" : "bgr.dst_outside", n, -1, "pane 3: the pane 18 x 14 at (20, 18) is outside the surface of 40 x 30", [](Call &c) { c.panes[3].dy = 18; });
        call(n ? "nv12.side" : "bgr.side", n, -1, "pane 0: a pane of 8193 x 14 (1..8192 each)", [](Call &c) { c.panes[0].dw = 8193; });
        call(n ? "nv12.same" : "bgr.same", n, -1, "pane 1: the source and the destination are the same pixels", [](Call &c) { c.sb[1].bgr = c.db[1].bgr; c.sn[1].y = c.dn[1].y; });
        call(n ? "nv12.overlap" : "bgr.overlap", n, -1, "panes 0 and 3 overlap in one destination surface", [](Call &c) { c.panes[3].dx = 16; c.panes[3].dy = 12; });
        call(n ? "nv12.touching" : "bgr.touching", n, 0, "", [](Call &c) { c.panes[3].dx = 18; c.panes[3].dy = 14; });
        call(n ? "nv12.skipped_sizes" : "bgr.skipped_sizes", n, 0, "", [](Call &c) { c.panes[2].sw = -7; c.panes[2].dw = 9000; c.panes[2].dx = 1; });
        call(n ? "nv12.other_surface" : "bgr.other_surface", n, 0, "", [](Call &c) { c.db[3].bgr = at(0xa0000); c.dn[3].y = at(0xa0000); c.dn[3].uv = at(0xa8000); c.panes[3].dx = 0; c.panes[3].dy = 0; });
    }
    call("bgr.src_pitch", false, -1, "source 0: pitch 100 is below 3 w = 192", [](Call &c) { c.sb[0].pitch = 100; });
    call("bgr.dst_pitch", false, -1, "destination 0: pitch 100 is below 3 w = 120", [](Call &c) { c.db[0].pitch = 100; });
    call("bgr.odd_sx_is_fine", false, 0, "", [](Call &c) { c.panes[0].sx = 3; c.panes[0].sy = 1; c.panes[0].sw = 11; c.panes[0].sh = 9; c.panes[0].dx = 1; });
    call("nv12.pitch_y", true, -1, "source 0: pitch_y 10 is below w = 64", [](Call &c) { c.sn[0].pitch_y = 10; });
    call("nv12.uv_odd_src", true, -1, "is odd (U V pairs are read", [](Call &c) { c.sn[0].uv = at(0x18001); });
    call("nv12.uv_odd_dst", true, -1, "is odd (U V pairs are written", [](Call &c) { c.dn[1].uv = at(0x98001); });
    call("nv12.matrix", true, -1, "destination 1: matrix 4", [](Call &c) { c.dn[1].matrix = 4; });
    call("nv12.odd_sx", true, -1, "pane 1: NV12 wants even sx, sy, dx, dy, not (3, 4) and (20, 0)", [](Call &c) { c.panes[1].sx = 3; });
    call("nv12.odd_dy", true, -1, "pane 3: NV12 wants even sx, sy, dx, dy, not (0, 0) and (20, 17)", [](Call &c) { c.panes[3].dy = 17; c.panes[3].dh = 13; });

    // the launch's grid: the tiles of the largest pane
    {
        PreviewJob j[2];
        memset(j, 0, sizeof j);
        j[0].pw = 64; j[0].ph = 16; j[1].pw = 129; j[1].ph = 33;
        fact("tiles", ffgpu_preview_tiles(j, 1) == 1 && ffgpu_preview_tiles(j, 2) == 9 && PREVIEW_TW == 64 && PREVIEW_TH == 16 && PREVIEW_ARG_JOBS == 32);
    }

    printf("preview_driver: %d cases, %d wrong\n", g_cases, g_wrong);
    return g_wrong ? 1 : 0;
}
