// warp_driver.cc -- ffgpu_warp_host.hpp on the CPU under AddressSanitizer + UBSan (`make warp`; tests/test_warp_abi.py): the warp spec, the mesh
// builders into buffers of exactly the mesh's size (a point too many is a heap overflow), the interpolation rule on meshes of extreme values, the
// argument checks and the planes of a call, on good and hostile arguments.  One line per case: id, return value, message.  The last line is
// "warp_driver: N cases, 0 wrong".  Nothing of HIP: the frames' and the device meshes' addresses are made up and never followed.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <limits>
#include "../ffgpu_warp_host.hpp"

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
static const int IMIN = std::numeric_limits<int>::min(), IMAX = std::numeric_limits<int>::max();

static ffgpu_warp_spec good_spec()
{
    ffgpu_warp_spec sp;
    memset(&sp, 0, sizeof sp);
    sp.filter = FFGPU_WARP_BILINEAR; sp.border = FFGPU_WARP_FILL; sp.fill[0] = 10; sp.fill[1] = 20; sp.fill[2] = 30;
    return sp;
}
template <class Fn> static void spec(const char *id, int want_rc, const char *want_msg, Fn change)
{
    ffgpu_warp_spec sp = good_spec();
    change(sp);
    g_err[0] = 0;
    line(id, ffgpu_warp_spec_check_host("op", &sp), want_rc, want_msg);
}

// a heap buffer of exactly the mesh's points
static std::vector<int> mesh_buf(int dw, int dh, int cell) { return std::vector<int>(2 * (size_t)((dw - 1) / cell + 2) * (size_t)((dh - 1) / cell + 2)); }

// a call of four jobs: three sources of (64 + k) x 48 into destinations of 40 x 30 with cells of 8, and one skipped
struct Call {
    std::vector<ffgpu_bgr_frame> sb, db;
    std::vector<ffgpu_nv12_frame> sn, dn;
    std::vector<ffgpu_warp_mesh> meshes;
    ffgpu_warp_spec spec = good_spec();
    bool have_srcs = true, have_dsts = true, have_meshes = true, have_spec = true;
    int njobs = 4;
    Call()
    {
        sb.resize(4); db.resize(4); sn.resize(4); dn.resize(4); meshes.resize(4);
        for (int k = 0; k < 4; k++) {
            memset(&sb[k], 0, sizeof sb[k]); memset(&db[k], 0, sizeof db[k]); memset(&sn[k], 0, sizeof sn[k]); memset(&dn[k], 0, sizeof dn[k]);
            memset(&meshes[k], 0, sizeof meshes[k]);
            sb[k].bgr = at(0x10001 + 0x10000 * k); sb[k].w = 64 + k; sb[k].h = 48; sb[k].pitch = 3 * (64 + k) + 5;
            sn[k].y = at(0x10001 + 0x10000 * k); sn[k].uv = at(0x18000 + 0x10000 * k); sn[k].w = 64 + k; sn[k].h = 48;
            db[k].bgr = at(0x90003 + 0x10000 * k); db[k].w = 40; db[k].h = 30;
            dn[k].y = at(0x90003 + 0x10000 * k); dn[k].uv = at(0x98000 + 0x10000 * k); dn[k].w = 40; dn[k].h = 30;
            meshes[k].xy = reinterpret_cast<const int *>(at(0x200008 + 0x1000 * k)); meshes[k].mw = 6; meshes[k].mh = 5; meshes[k].cell = 8;
        }
        sb[2].bgr = nullptr; sn[2].y = nullptr;                                      // a skipped job
        meshes[1].cell = 32; meshes[1].mw = 3; meshes[1].mh = 2;
    }
};
template <class Fn> static void call(const char *id, bool nv12, int want_rc, const char *want_msg, Fn change)
{
    Call c;
    change(c);
    g_err[0] = 0;
    std::vector<WarpJob> jobs[2];
    int rc;
    const ffgpu_warp_mesh *mm = c.have_meshes ? c.meshes.data() : nullptr;
    const ffgpu_warp_spec *sp = c.have_spec ? &c.spec : nullptr;
    if (nv12) rc = ffgpu_warp_args_check("op", c.have_srcs ? c.sn.data() : nullptr, c.have_dsts ? c.dn.data() : nullptr, mm, c.njobs, sp, jobs);
    else      rc = ffgpu_warp_args_check("op", c.have_srcs ? c.sb.data() : nullptr, c.have_dsts ? c.db.data() : nullptr, mm, c.njobs, sp, jobs);
    line(id, rc, want_rc, want_msg);
    if (rc == 0 && want_rc == 0 && c.njobs == 4) {                                    // three live jobs; NV12: a U V plane of half the size for each
        bool ok = jobs[0].size() == 3 && jobs[1].size() == (nv12 ? 3u : 0u);
        if (ok) {
            const WarpJob &j = jobs[0][1];
            ok = j.sw == 65 && j.sh == 48 && j.dw == 40 && j.dh == 30 && j.mw == 3 && j.shift == 5 && j.spitch == (nv12 ? 65 : 200) && j.dpitch == (nv12 ? 40 : 120) &&
                 j.xy == c.meshes[1].xy && j.src == (nv12 ? c.sn[1].y : c.sb[1].bgr) && jobs[0][2].src == (nv12 ? c.sn[3].y : c.sb[3].bgr);
            if (ok && nv12) {
                const WarpJob &u = jobs[1][1];
                ok = u.sw == 33 && u.sh == 24 && u.dw == 20 && u.dh == 15 && u.mw == 3 && u.shift == (5 | 1 << 8) && u.spitch == 66 && u.dpitch == 40 && u.src == c.sn[1].uv && u.xy == j.xy;
            }
        }
        fact(id, ok);
    }
}

int main()
{
    spec("spec.good", 0, "", [](ffgpu_warp_spec &) {});
    spec("spec.nearest_clamp", 0, "", [](ffgpu_warp_spec &s) { s.filter = FFGPU_WARP_NEAREST; s.border = FFGPU_WARP_CLAMP; });
    spec("spec.filter_2", -1, "filter 2 is neither FFGPU_WARP_BILINEAR nor FFGPU_WARP_NEAREST", [](ffgpu_warp_spec &s) { s.filter = 2; });
    spec("spec.filter_min", -1, "is neither FFGPU_WARP_BILINEAR", [](ffgpu_warp_spec &s) { s.filter = IMIN; });
    spec("spec.border_2", -1, "border 2 is neither FFGPU_WARP_FILL nor FFGPU_WARP_CLAMP", [](ffgpu_warp_spec &s) { s.border = 2; });
    spec("spec.border_neg", -1, "border -1 is neither", [](ffgpu_warp_spec &s) { s.border = -1; });
    spec("spec.fill3", -1, "fill[3] must be 0", [](ffgpu_warp_spec &s) { s.fill[3] = 1; });
    spec("spec.reserved", -1, "spec: reserved must be 0", [](ffgpu_warp_spec &s) { s.reserved = 1; });
    g_err[0] = 0;
    line("spec.null", ffgpu_warp_spec_check_host("op", nullptr), -1, "NULL spec");

    // the mesh's size
    {
        int m[2] = { 0, 0 };
        line("size.1x1", ffgpu_warp_mesh_size_host("op", 1, 1, 8, m), 0, "");
        fact("size.1x1", m[0] == 2 && m[1] == 2);
        line("size.8192", ffgpu_warp_mesh_size_host("op", 8192, 8192, 64, m), 0, "");
        fact("size.8192", m[0] == 129 && m[1] == 129);
        line("size.8192_c8", ffgpu_warp_mesh_size_host("op", 8192, 8, 8, m), 0, "");
        fact("size.8192_c8", m[0] == 1025 && m[1] == 2);
        line("size.9x17", ffgpu_warp_mesh_size_host("op", 9, 17, 8, m), 0, "");
        fact("size.9x17", m[0] == 3 && m[1] == 4);
        line("size.side_0", ffgpu_warp_mesh_size_host("op", 0, 5, 8, m), -1, "a destination of 0 x 5 (1..8192 each)");
        line("size.side_8193", ffgpu_warp_mesh_size_host("op", 5, 8193, 8, m), -1, "a destination of 5 x 8193 (1..8192 each)");
        line("size.side_min", ffgpu_warp_mesh_size_host("op", IMIN, IMAX, 8, m), -1, "(1..8192 each)");
        line("size.cell_4", ffgpu_warp_mesh_size_host("op", 5, 5, 4, m), -1, "cell 4 is none of 8, 16, 32, 64");
        line("size.cell_24", ffgpu_warp_mesh_size_host("op", 5, 5, 24, m), -1, "cell 24 is none of");
        line("size.cell_min", ffgpu_warp_mesh_size_host("op", 5, 5, IMIN, m), -1, "is none of 8, 16, 32, 64");
        line("size.cell_0", ffgpu_warp_mesh_size_host("op", 5, 5, 0, m), -1, "cell 0 is none of");
        line("size.null_out", ffgpu_warp_mesh_size_host("op", 5, 5, 8, nullptr), -1, "NULL out");
    }

    // the orientations: exact integers, into buffers of exactly the mesh's size; orient k then its inverse is the identity at every mesh point
    {
        static const int inverse[8] = { 0, 3, 2, 1, 4, 5, 6, 7 };
        for (int o = 0; o < 8; o++) {
            char id[32];
            snprintf(id, sizeof id, "orient.%d", o);
            int wh[2] = { 0, 0 }, wh2[2] = { 0, 0 };
            line(id, ffgpu_warp_mesh_orient_host("op", 37, 23, o, 8, wh, nullptr), 0, "");
            fact(id, wh[0] == ((o & 1) ? 23 : 37) && wh[1] == ((o & 1) ? 37 : 23));
            std::vector<int> a = mesh_buf(wh[0], wh[1], 8);
            line(id, ffgpu_warp_mesh_orient_host("op", 37, 23, o, 8, wh, a.data()), 0, "");
            // destination pixel (0, 0) is the source corner the table names
            const int x0 = (o == 2 || o == 3 || o == 4 || o == 5) ? 36 : 0, y0 = (o == 1 || o == 2 || o == 5 || o == 6) ? 22 : 0;
            fact(id, a[0] == 256 * x0 && a[1] == 256 * y0);
            // composed with the inverse: the point of mesh `a` at the position mesh `b` names is the identity (both are affine with integer terms)
            std::vector<int> b = mesh_buf(37, 23, 8);
            line(id, ffgpu_warp_mesh_orient_host("op", wh[0], wh[1], inverse[o], 8, wh2, b.data()), 0, "");
            bool ok = wh2[0] == 37 && wh2[1] == 23;
            const int mw = (wh[0] - 1) / 8 + 2;
            const int ax = (a[2] - a[0]) / 8, ay = (a[3] - a[1]) / 8, bx = (a[2 * mw] - a[0]) / 8, by = (a[2 * mw + 1] - a[1]) / 8;      // a's terms per pixel, in 1 / 256
            for (int u = 0; u < 5 && ok; u++)
                for (int v = 0; v < 3 && ok; v++) {                                  // b at mesh point (u, v) is destination pixel (8 u, 8 v) of the round trip
                    const int bi = b[2 * (v * 6 + u)] / 256, bj = b[2 * (v * 6 + u) + 1] / 256;
                    ok = a[0] + ax * bi + bx * bj == 256 * 8 * u && a[1] + ay * bi + by * bj == 256 * 8 * v;
                }
            fact(id, ok);
        }
        int wh[2];
        std::vector<int> big = mesh_buf(8192, 8192, 64);
        line("orient.8192", ffgpu_warp_mesh_orient_host("op", 8192, 8192, 5, 64, wh, big.data()), 0, "");
        fact("orient.8192", big[0] == 256 * 8191 && big[1] == 256 * 8191 && big[2 * 128] == 256 * 8191 && big[2 * 128 + 1] == 256 * (8191 - 8192));
        std::vector<int> one = mesh_buf(1, 1, 8);
        line("orient.1x1", ffgpu_warp_mesh_orient_host("op", 1, 1, 2, 8, wh, one.data()), 0, "");
        fact("orient.1x1", one[0] == 0 && one[1] == 0 && one[2] == -2048 && one[7] == -2048);
        line("orient.8", ffgpu_warp_mesh_orient_host("op", 37, 23, 8, 8, wh, nullptr), -1, "orient 8 (0..7)");
        line("orient.neg", ffgpu_warp_mesh_orient_host("op", 37, 23, -1, 8, wh, nullptr), -1, "orient -1 (0..7)");
        line("orient.side", ffgpu_warp_mesh_orient_host("op", 8193, 23, 0, 8, wh, nullptr), -1, "a source of 8193 x 23 (1..8192 each)");
        line("orient.side_0", ffgpu_warp_mesh_orient_host("op", 37, 0, 0, 8, wh, nullptr), -1, "a source of 37 x 0");
        line("orient.cell", ffgpu_warp_mesh_orient_host("op", 37, 23, 0, 7, wh, nullptr), -1, "cell 7 is none of");
        line("orient.null_wh", ffgpu_warp_mesh_orient_host("op", 37, 23, 0, 8, nullptr, nullptr), -1, "NULL out_dst_wh");
    }

    // the homography and the lens: into exact buffers; non-finite values and denominators that are not above 0
    {
        std::vector<int> m = mesh_buf(40, 30, 8);                                    // 6 x 5 points
        const double ident[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 };
        line("homography.identity", ffgpu_warp_mesh_homography_host("op", 40, 30, 8, ident, m.data()), 0, "");
        fact("homography.identity", m[0] == 0 && m[1] == 0 && m[2] == 2048 && m[2 * 6 + 1] == 2048 && m[2 * 29] == 256 * 40 && m[2 * 29 + 1] == 256 * 32);
        const double shift[9] = { 1, 0, 2.5, 0, -1, 29, 0, 0, 1 };
        line("homography.flip", ffgpu_warp_mesh_homography_host("op", 40, 30, 8, shift, m.data()), 0, "");
        fact("homography.flip", m[0] == 640 && m[1] == 256 * 29 && m[2 * 6 + 1] == 256 * 21);
        const double persp[9] = { 1, 0, 0, 0, 1, 0, -0.125, 0, 1 };                    // the denominator 1 - i / 8 is 0 at i = 8 and below 0 behind it
        line("homography.den", ffgpu_warp_mesh_homography_host("op", 40, 30, 8, persp, m.data()), 0, "");
        fact("homography.den", m[0] == 0 && m[2] == IMIN && m[3] == IMIN && m[4] == IMIN && m[5] == IMIN);
        const double huge[9] = { 1e300, 0, 1e9, 0, -1e300, -1e9, 0, 0, 1 };
        line("homography.saturate", ffgpu_warp_mesh_homography_host("op", 40, 30, 8, huge, m.data()), 0, "");
        fact("homography.saturate", m[0] == IMAX && m[1] == IMIN && m[2] == IMAX && m[2 * 6 + 1] == IMIN);
        const double nans[9] = { std::numeric_limits<double>::quiet_NaN(), 0, 0, 0, std::numeric_limits<double>::infinity(), 0, 0, 0, 1 };
        line("homography.nan", ffgpu_warp_mesh_homography_host("op", 40, 30, 8, nans, m.data()), 0, "");
        fact("homography.nan", m[0] == IMIN && m[1] == IMIN && m[2 * 6] == IMIN && m[2 * 6 + 1] == IMIN);           // (inf * 0 is NaN at j = 0)
        const double nanden[9] = { 1, 0, 0, 0, 1, 0, 0, 0, std::numeric_limits<double>::quiet_NaN() };
        line("homography.nan_den", ffgpu_warp_mesh_homography_host("op", 40, 30, 8, nanden, m.data()), 0, "");
        fact("homography.nan_den", m[0] == IMIN && m[59] == IMIN);
        line("homography.null_h", ffgpu_warp_mesh_homography_host("op", 40, 30, 8, nullptr, m.data()), -1, "NULL h");
        line("homography.null_xy", ffgpu_warp_mesh_homography_host("op", 40, 30, 8, ident, nullptr), -1, "NULL xy");
        line("homography.cell", ffgpu_warp_mesh_homography_host("op", 40, 30, 9, ident, m.data()), -1, "cell 9 is none of");
        line("homography.side", ffgpu_warp_mesh_homography_host("op", 40, -30, 8, ident, m.data()), -1, "a destination of 40 x -30");

        ffgpu_warp_lens ln;
        memset(&ln, 0, sizeof ln);
        ln.model = FFGPU_WARP_LENS_BROWN; ln.dst[0] = ln.dst[1] = 16; ln.dst[2] = 16; ln.dst[3] = 8; ln.src[0] = ln.src[1] = 32; ln.src[2] = 100; ln.src[3] = 50;
        line("lens.pinhole", ffgpu_warp_mesh_lens_host("op", 40, 30, 8, &ln, m.data()), 0, "");
        fact("lens.pinhole", m[0] == 256 * 68 && m[1] == 256 * 34 && m[2 * 2] == 256 * 100 && m[2 * 8 + 1] == 256 * 50);      // no distortion: x = 32 (i - 16) / 16 + 100
        ln.k[0] = -0.25;
        line("lens.brown", ffgpu_warp_mesh_lens_host("op", 40, 30, 8, &ln, m.data()), 0, "");
        fact("lens.brown", m[2 * 2] == 256 * 100 && m[2 * 2 + 1] == 256 * 35 && m[2 * 8] == 256 * 100 && m[2 * 8 + 1] == 256 * 50);  // (16, 0): yn = -0.5, rad = 1 - 0.0625, y = 50 - 15
        ln.model = FFGPU_WARP_LENS_EQUIDISTANT; ln.k[0] = 0;
        line("lens.fisheye", ffgpu_warp_mesh_lens_host("op", 40, 30, 8, &ln, m.data()), 0, "");
        fact("lens.fisheye", m[2 * 8] == 256 * 100 && m[2 * 8 + 1] == 256 * 50 && m[2 * 9] > 256 * 100 && m[2 * 9] < 256 * 116);      // r = 0: scale 1; atan(r) < r
        ln.k[3] = 1e308; ln.k[2] = 1e308;
        line("lens.overflow", ffgpu_warp_mesh_lens_host("op", 40, 30, 8, &ln, m.data()), 0, "");
        fact("lens.overflow", m[2 * 8] == 256 * 100 && (m[0] == IMIN || m[0] == IMAX));
        ln.model = 2;
        line("lens.model", ffgpu_warp_mesh_lens_host("op", 40, 30, 8, &ln, m.data()), -1, "model 2 is neither FFGPU_WARP_LENS_BROWN nor FFGPU_WARP_LENS_EQUIDISTANT");
        ln.model = 0; ln.reserved = 3;
        line("lens.reserved", ffgpu_warp_mesh_lens_host("op", 40, 30, 8, &ln, m.data()), -1, "lens: reserved must be 0");
        ln.reserved = 0; ln.dst[0] = 0;
        line("lens.fx_0", ffgpu_warp_mesh_lens_host("op", 40, 30, 8, &ln, m.data()), -1, "must be finite and above 0");
        ln.dst[0] = 16; ln.dst[1] = std::numeric_limits<double>::infinity();
        line("lens.fy_inf", ffgpu_warp_mesh_lens_host("op", 40, 30, 8, &ln, m.data()), -1, "must be finite and above 0");
        ln.dst[1] = std::numeric_limits<double>::quiet_NaN();
        line("lens.fy_nan", ffgpu_warp_mesh_lens_host("op", 40, 30, 8, &ln, m.data()), -1, "must be finite and above 0");
        ln.dst[1] = 16;
        line("lens.null", ffgpu_warp_mesh_lens_host("op", 40, 30, 8, nullptr, m.data()), -1, "NULL lens");
        line("lens.null_xy", ffgpu_warp_mesh_lens_host("op", 40, 30, 8, &ln, nullptr), -1, "NULL xy");
        line("lens.cell", ffgpu_warp_mesh_lens_host("op", 40, 30, 128, &ln, m.data()), -1, "cell 128 is none of");
    }

    // the interpolation rule on a host mesh of extreme values: every result inside [min, max] of its four points, exact at the points
    {
        std::vector<int> m = mesh_buf(20, 12, 8);                                    // 4 x 3 points
        for (size_t n = 0; n < m.size(); n++) m[n] = (n % 3 == 0) ? IMIN : (n % 3 == 1) ? IMAX : (int)(n * 7919u);
        ffgpu_warp_mesh mesh;
        memset(&mesh, 0, sizeof mesh);
        mesh.xy = m.data(); mesh.mw = 4; mesh.mh = 3; mesh.cell = 8;
        bool ok = true;
        int out[2];
        for (int j = 0; j < 12 && ok; j++)
            for (int i = 0; i < 20 && ok; i++) {
                ok = ffgpu_warp_point_host("op", &mesh, 20, 12, i, j, out) == 0;
                for (int ch = 0; ch < 2 && ok; ch++) {
                    const int *p = m.data() + 2 * ((j >> 3) * 4 + (i >> 3)) + ch;
                    const int lo = std::min(std::min(p[0], p[2]), std::min(p[8], p[10])), hi = std::max(std::max(p[0], p[2]), std::max(p[8], p[10]));
                    ok = out[ch] >= lo && out[ch] <= hi && (((i | j) & 7) || out[ch] == p[0]);
                }
            }
        fact("point.extreme", ok);
        for (size_t n = 0; n < m.size(); n++) m[n] = IMAX;
        line("point.all_max", ffgpu_warp_point_host("op", &mesh, 20, 12, 19, 11, out), 0, "");
        fact("point.all_max", out[0] == IMAX && out[1] == IMAX);
        for (size_t n = 0; n < m.size(); n++) m[n] = IMIN;
        line("point.all_min", ffgpu_warp_point_host("op", &mesh, 20, 12, 3, 5, out), 0, "");
        fact("point.all_min", out[0] == IMIN && out[1] == IMIN);
        line("point.outside", ffgpu_warp_point_host("op", &mesh, 20, 12, 20, 0, out), -1, "pixel (20, 0) is outside the destination of 20 x 12");
        line("point.neg", ffgpu_warp_point_host("op", &mesh, 20, 12, 0, -1, out), -1, "pixel (0, -1) is outside");
        line("point.null_mesh", ffgpu_warp_point_host("op", nullptr, 20, 12, 0, 0, out), -1, "NULL mesh");
        line("point.null_out", ffgpu_warp_point_host("op", &mesh, 20, 12, 0, 0, nullptr), -1, "NULL out");
        line("point.size", ffgpu_warp_point_host("op", &mesh, 30, 12, 0, 0, out), -1, "mesh: 4 x 3 points, a destination of 30 x 12 with cells of 8 has 5 x 3");
        line("point.side", ffgpu_warp_point_host("op", &mesh, 0, 12, 0, 0, out), -1, "a destination of 0 x 12");
        mesh.cell = 5;
        line("point.cell", ffgpu_warp_point_host("op", &mesh, 20, 12, 0, 0, out), -1, "mesh: cell 5 is none of");
        mesh.cell = 8; mesh.xy = nullptr;
        line("point.null_xy", ffgpu_warp_point_host("op", &mesh, 20, 12, 0, 0, out), -1, "mesh: NULL xy");
    }

    for (int nv12 = 0; nv12 < 2; nv12++) {
        const bool n = nv12 != 0;
        call(n ? "nv12.good" : "bgr.good", n, 0, "", [](Call &) {});
        call(n ? "nv12.null_srcs" : "bgr.null_srcs", n, -1, "NULL srcs", [](Call &c) { c.have_srcs = false; });
        call(n ? "nv12.null_dsts" : "bgr.null_dsts", n, -1, "NULL dsts", [](Call &c) { c.have_dsts = false; });
        call(n ? "nv12.null_meshes" : "bgr.null_meshes", n, -1, "NULL meshes", [](Call &c) { c.have_meshes = false; });
        call(n ? "nv12.null_spec" : "bgr.null_spec", n, -1, "NULL spec", [](Call &c) { c.have_spec = false; });
        call(n ? "nv12.njobs_0" : "bgr.njobs_0", n, -1, "0 jobs (1..4096)", [](Call &c) { c.njobs = 0; });
        call(n ? "nv12.njobs_4097" : "bgr.njobs_4097", n, -1, "4097 jobs (1..4096)", [](Call &c) { c.njobs = 4097; });
        call(n ? "nv12.njobs_min" : "bgr.njobs_min", n, -1, "jobs (1..4096)", [](Call &c) { c.njobs = IMIN; });
        call(n ? "nv12.filter" : "bgr.filter", n, -1, "filter 3 is neither", [](Call &c) { c.spec.filter = 3; });
        call(n ? "nv12.border" : "bgr.border", n, -1, "border 4 is neither", [](Call &c) { c.spec.border = 4; });
        call(n ? "nv12.fill3" : "bgr.fill3", n, -1, "fill[3] must be 0", [](Call &c) { c.spec.fill[3] = 9; });
        call(n ? "nv12.reserved" : "bgr.reserved", n, -1, "spec: reserved must be 0", [](Call &c) { c.spec.reserved = -1; });
        call(n ? "nv12.src_size" : "bgr.src_size", n, -1, "source 1: bad size 0 x 48", [](Call &c) { c.sb[1].w = 0; c.sn[1].w = 0; });
        call(n ? "nv12.dst_size" : "bgr.dst_size", n, -1, "destination 3: bad size 40 x -1", [](Call &c) { c.db[3].h = -1; c.dn[3].h = -1; });
        call(n ? "nv12.src_reserved" : "bgr.src_reserved", n, -1, "source 0: reserved must be 0", [](Call &c) { c.sb[0].reserved = 1; c.sn[0].reserved = 1; });
        call(n ? "nv12.dst_reserved" : "bgr.dst_reserved", n, -1, "destination 1: reserved must be 0", [](Call &c) { c.db[1].reserved = 1; c.dn[1].reserved = 1; });
        call(n ? "nv12.src_side" : "bgr.src_side", n, -1, "job 0: a source of 8193 x 48 (1..8192 each)", [](Call &c) { c.sb[0].w = 8193; c.sb[0].pitch = 0; c.sn[0].w = 8193; });
        call(n ? "nv12.dst_side" : "bgr.dst_side", n, -1, "job 3: a destination of 40 x 8193 (1..8192 each)", [](Call &c) { c.db[3].h = 8193; c.dn[3].h = 8193; });
        call(n ? "nv12.mesh_null" : "bgr.mesh_null", n, -1, "job 1: mesh: NULL xy", [](Call &c) { c.meshes[1].xy = nullptr; });
        call(n ? "nv12.mesh_align" : "bgr.mesh_align", n, -1, "job 3: mesh: xy 0x20300c is not 8-byte aligned", [](Call &c) { c.meshes[3].xy = reinterpret_cast<const int *>(at(0x20300c)); });
        call(n ? "nv12.mesh_size" : "bgr.mesh_size", n, -1, "job 0: mesh: 6 x 6 points, a destination of 40 x 30 with cells of 8 has 6 x 5", [](Call &c) { c.meshes[0].mh = 6; });
        call(n ? "nv12.mesh_size_w" : "bgr.mesh_size_w", n, -1, "job 1: mesh: 4 x 2 points, a destination of 40 x 30 with cells of 32 has 3 x 2", [](Call &c) { c.meshes[1].mw = 4; });
        call(n ? "nv12.mesh_cell" : "bgr.mesh_cell", n, -1, "job 0: mesh: cell 12 is none of 8, 16, 32, 64", [](Call &c) { c.meshes[0].cell = 12; });
        call(n ? "nv12.mesh_cell_0" : "bgr.mesh_cell_0", n, -1, "job 3: mesh: cell 0 is none of", [](Call &c) { c.meshes[3].cell = 0; });
        call(n ? "nv12.mesh_reserved" : "bgr.mesh_reserved", n, -1, "job 1: mesh: reserved must be 0", [](Call &c) { c.meshes[1].reserved = 1; });
        call(n ? "nv12.same" : "bgr.same", n, -1, "job 1: the source and the destination are the same pixels", [](Call &c) { c.sb[1].bgr = c.db[1].bgr; c.sn[1].y = c.dn[1].y; });
        call(n ? "nv12.same_dst" : "bgr.same_dst", n, -1, "jobs 0 and 3 have the same destination", [](Call &c) { c.db[3].bgr = c.db[0].bgr; c.dn[3].y = c.dn[0].y; });
        call(n ? "nv12.same_dst_skipped" : "bgr.same_dst_skipped", n, 0, "", [](Call &c) { c.db[2].bgr = c.db[0].bgr; c.dn[2].y = c.dn[0].y; });
        call(n ? "nv12.skipped_mesh" : "bgr.skipped_mesh", n, 0, "", [](Call &c) { c.meshes[2].xy = nullptr; c.meshes[2].cell = -7; c.db[2].w = 9000; c.dn[2].w = 9000; });
        call(n ? "nv12.skipped_dst" : "bgr.skipped_dst", n, 0, "", [](Call &c) { c.sb[2].bgr = at(0x30001); c.sn[2].y = at(0x30001); c.db[2].bgr = nullptr; c.dn[2].y = nullptr; c.meshes[2].mw = 0; });
        call(n ? "nv12.shared_source" : "bgr.shared_source", n, 0, "", [](Call &c) { c.sb[3] = c.sb[0]; c.sn[3] = c.sn[0]; });
    }
    call("bgr.src_pitch", false, -1, "source 0: pitch 100 is below 3 w = 192", [](Call &c) { c.sb[0].pitch = 100; });
    call("bgr.dst_pitch", false, -1, "destination 0: pitch 100 is below 3 w = 120", [](Call &c) { c.db[0].pitch = 100; });
    call("nv12.pitch_y", true, -1, "source 0: pitch_y 10 is below w = 64", [](Call &c) { c.sn[0].pitch_y = 10; });
    call("nv12.uv_odd_src", true, -1, "is odd (U V pairs are read", [](Call &c) { c.sn[0].uv = at(0x18001); });
    call("nv12.uv_odd_dst", true, -1, "is odd (U V pairs are written", [](Call &c) { c.dn[1].uv = at(0xa8001); });
    call("nv12.matrix", true, -1, "destination 1: matrix 4", [](Call &c) { c.dn[1].matrix = 4; });

    // the launch's grid: the tiles of the largest job
    {
        WarpJob j[2];
        memset(j, 0, sizeof j);
        j[0].dw = 64; j[0].dh = 16; j[1].dw = 129; j[1].dh = 33;
        fact("tiles", ffgpu_warp_tiles(j, 1) == 1 && ffgpu_warp_tiles(j, 2) == 9 && WARP_TW == 64 && WARP_TH == 16 && WARP_ARG_JOBS == 64);
    }

    printf("warp_driver: %d cases, %d wrong\n", g_cases, g_wrong);
    return g_wrong ? 1 : 0;
}
