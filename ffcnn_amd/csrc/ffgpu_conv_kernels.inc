// ffgpu_conv_kernels.inc -- convolution kernel selection (included by ffgpu_kernels.hip)
#include "ffgpu_dw_stream.inc"
#include "ffgpu_pw_mfma.inc"
#include "ffgpu_pw_gemm32.inc"
#include "ffgpu_pw_bf16.inc"
#include "ffgpu_conv_igemm.inc"
#include "ffgpu_dwpw.inc"
#include "ffgpu_conv_dense.inc"
#include "ffgpu_irb.inc"
#include "ffgpu_irb_thin.inc"
#include "ffgpu_irb_thin_s2.inc"
#include "ffgpu_front.inc"
#include "ffgpu_irb_wave.inc"
#include "ffgpu_irb_wave2.inc"
#include "ffgpu_irb_stage.inc"
#include "ffgpu_pw_x3.inc"
#include "ffgpu_pw_x3t.inc"
#include "ffgpu_conv_x3.inc"
#include "ffgpu_dw_lds.inc"
#include "ffgpu_dw_pair.inc"
#include "ffgpu_conv_thin.inc"

// Scratch for the packed weight image of a BARE single-layer call (conv_image): per host thread and per DEVICE -- one thread may drive several GPUs -- grown on demand
struct BareScratch {
    float *p = nullptr; size_t n = 0; int dev = -1;
    float *get(size_t need)
    {
        int d = 0;
        (void)hipGetDevice(&d);
        if (p && dev == d && n >= need) return p;
        if (p) (void)hipFree(p);
        p = nullptr; n = 0; dev = d;
        if (hipMalloc(&p, need * sizeof(float)) != hipSuccess) { p = nullptr; return nullptr; }
        n = need;
        return p;
    }
};

// CUs of the current device (a node plans on every GPU of the box), asked once per device and process (ADVICE r05: no runtime query per launch); 256 if the runtime does not say
static int device_cus()
{
    static int cu_of[64];
    static std::mutex cu_mu;
    int dev = 0, cus = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(cu_mu);
    if (dev >= 0 && dev < 64) {
        if (!cu_of[dev]) (void)hipDeviceGetAttribute(&cu_of[dev], hipDeviceAttributeMultiprocessorCount, dev);
        cus = cu_of[dev];
    } else (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    return cus > 0 ? cus : 256;
}

// m with i / dv == __umulhi(i, m) for 32-bit i (exact while i * dv < 2^32): ceil(2^32 / dv), dv >= 1.  A divisor of 1 has no 32-bit m (2^32
// wraps to 0, which the earlier copies reached with and without saying so): k_conv_igemm, k_conv_first and k_dw_lds read m == 0 as "divisor 1, the
// quotient is i"; k_dw_pair multiplies unconditionally and never gets one (dw_pair_ok: every divisor is >= 2).
static unsigned umulhi_magic(long dv) { return dv == 1 ? 0u : (unsigned)(((1ULL << 32) + (unsigned long long)dv - 1) / (unsigned long long)dv); }

// Pixel tiles of the two tiled pointwise GEMMs (k_pw_gemm32, k_pw_x3t): main tiles of 128 pixels, then narrow ones of 64 over the rest.  The narrow
// ones take over the partial last round: with `slots` workgroups resident, (tiles % slots) main tiles would run alone at the end.
static void split_main_narrow(long P, int ntm, int slots, bool narrow_on, long *ntn_main, long *ntn_narrow)
{
    const long ntn_all = (P + 127) / 128, total_all = ntn_all * ntm;
    long tail_tiles = total_all % slots;                           // main tiles of the partial round
    if (total_all <= slots / 2) tail_tiles = total_all;            // a launch that never fills the chip: all narrow
    else if (tail_tiles > slots * 5 / 8) tail_tiles = 0;           // a nearly full round: leave it
    if (!narrow_on) tail_tiles = 0;
    const long tail_ntn = (tail_tiles + ntm - 1) / ntm;            // pixel tiles handed to the narrow form
    *ntn_main = ntn_all - tail_ntn;
    const long npx_narrow = P - *ntn_main * 128;
    *ntn_narrow = npx_narrow > 0 ? (npx_narrow + 63) / 64 : 0;
}

static bool conv_cnhw_contiguous(const ConvDesc &d)
{
    return d.in_ns == (long)d.iw * d.ih && d.in_cs == (long)d.N * d.iw * d.ih &&
           d.out_ns == (long)d.ow * d.oh && d.out_cs == (long)d.N * d.ow * d.oh &&
           (!d.residual || (d.res_ns == d.out_ns && d.res_cs == d.out_cs));
}
static bool conv_is_depthwise(const ConvDesc &d) { return d.groups == d.ic && d.ic == d.oc; }
static bool conv_is_pointwise(const ConvDesc &d) { return d.fs == 1 && d.stride == 1 && d.pad == 0 && d.groups == 1; }

static bool dw_stream_ok(const ConvDesc &d)
{
    return conv_is_depthwise(d) && d.fs == 3 && d.stride == 1 && d.pad == 1 && conv_cnhw_contiguous(d) &&
           d.iw % 4 == 0 && d.iw >= 40 && d.iw <= 512 && d.ih >= 2 && !d.residual && d.act != 3;
}
static bool pw_mfma_ok(const ConvDesc &d)
{
    const long P = (long)d.N * d.iw * d.ih;
    return conv_is_pointwise(d) && conv_cnhw_contiguous(d) && P % 4 == 0 && ((d.ic + 3) & ~3) <= 1024 && P < (1L << 28);   // 3 P + 64 floats in a 32-bit byte offset
}

// split-bf16 pointwise kernel (ffgpu_pw_x3.inc): fp32-equivalent results on the bf16 matrix cores; worth it where the layer is a
// real contraction (the expand / project layers inside fused blocks never get here)
static int pw_x3_mt(const ConvDesc &d) { const int f = knob(K_PWX3_MT); return f == 4 || f == 2 || f == 1 ? f : 4; }
static bool pw_x3_ok(const ConvDesc &d)
{
    const long P = (long)d.N * d.iw * d.ih;
    return pw_mfma_ok(d) && (long)(d.ic + 32) * P < (1L << 30);
}
// AUTO takes it where it wins (tools/pw_x3_bench.py, bench.py roofline_pw): big contractions -- BASELINE config[2] (256 -> 512 on 20x20 x 256)
// 186 us against 218-224 us of k_pw_gemm32 inside bench.py; on the heads' layers of yolo-fastest (120 -> 120 / 255 on 25 600 pixels)
// k_pw_mfma / k_pw_gemm32 stay ahead (each wave re-reads and re-splits its input rows per 64-channel tile).  FFGPU_PW_X3=0: never.
static bool pw_x3_auto(const ConvDesc &d)
{
    const long P = (long)d.N * d.iw * d.ih;
    return pw_x3_ok(d) && d.ic >= knob(K_PWX3_MIN_IC) && d.oc >= knob(K_PWX3_MIN_OC) && P >= knob(K_PWX3_MIN_P) &&
           knob(K_PW_X3) != 0;
}
// tiled split-bf16 GEMM (ffgpu_pw_x3t.inc): a workgroup splits every input value once per 256 output channels.  AUTO: real contractions with
// enough pixels to fill the chip (BASELINE config[2]); FFGPU_PW_X3T=0: never.
static bool pw_x3t_ok(const ConvDesc &d)
{
    const long P = (long)d.N * d.iw * d.ih;
    return pw_mfma_ok(d) && (long)(d.ic + 32) * P < (1L << 29) && (long)(d.oc + 256) * P < (1L << 30);      // (buffer offsets in bytes < 2^31)
}
static bool pw_x3t_auto(const ConvDesc &d)
{
    const long P = (long)d.N * d.iw * d.ih;
    return pw_x3t_ok(d) && knob(K_PW_X3T) != 0 && d.ic >= knob(K_PWX3T_MIN_IC) && d.oc >= knob(K_PWX3T_MIN_OC) &&
           P >= knob(K_PWX3T_MIN_P);
}
// 32-row blocks per wave: workgroup tiles of 256 channels (default) or 128 (tuning, FFGPU_PWXT_TM=128).  Part of the packed image's layout: a planned layer carries it in
// ConvDesc::x3_mt (ffgpu_conv_plan), pack and every launch read THAT -- the environment only decides for unplanned single-layer calls (ADVICE r05)
static int  pwx3t_rb_env() { return knob(K_PWXT_TM) == 128 ? 1 : 2; }
static int  pwx3t_rb(const ConvDesc &d) { return (d.kernel == FFGPU_K_PW_X3T && (d.x3_mt == 1 || d.x3_mt == 2)) ? d.x3_mt : pwx3t_rb_env(); }
static void pwx3t_dims(const ConvDesc &d, int &nchunks, int &ntm) { nchunks = ((d.ic + 2 * XT_KC - 1) / (2 * XT_KC)) * 2; ntm = (d.oc + xt_tm(pwx3t_rb(d)) - 1) / xt_tm(pwx3t_rb(d)); }     // chunks in pairs (zero weights behind ic)
static size_t pwx3t_img_dwords(const ConvDesc &d) { int nc, ntm; pwx3t_dims(d, nc, ntm); return ((size_t)nc * xt_ach(pwx3t_rb(d)) + 2 * xt_tm(pwx3t_rb(d))) * ntm; }
static int pwx3t_pack(const ConvDesc &d, float *pk, hipStream_t s)
{
    PwX3tPackP q;
    q.filt = d.filt; q.pk = reinterpret_cast<unsigned *>(pk); q.ic = d.ic; q.oc = d.oc; q.k4 = (d.ic + 3) & ~3;
    pwx3t_dims(d, q.nchunks, q.ntm);
    q.rb = pwx3t_rb(d);
    const long total = (long)pwx3t_img_dwords(d);
    hipLaunchKernelGGL(k_pw_x3t_pack, dim3((unsigned)std::min((total + 255) / 256, 8192L)), dim3(256), 0, s, q);
    LAUNCH_OK("pw_x3t_pack");
    return 0;
}
static void pwx3_dims(const ConvDesc &d, int &ksteps, int &nrb) { ksteps = (d.ic + 31) / 32; nrb = (d.oc + 15) / 16; }
static size_t pwx3_img_dwords(const ConvDesc &d) { int ks, nrb; pwx3_dims(d, ks, nrb); return (size_t)nrb * ks * 3 * 256; }
static int pwx3_pack(const ConvDesc &d, float *pk, hipStream_t s)
{
    PwX3PackP q;
    q.filt = d.filt; q.pk = reinterpret_cast<unsigned *>(pk); q.ic = d.ic; q.oc = d.oc; q.k4 = (d.ic + 3) & ~3;
    pwx3_dims(d, q.ksteps, q.nrb);
    const long total = (long)pwx3_img_dwords(d);
    hipLaunchKernelGGL(k_pw_x3_pack, dim3((unsigned)std::min((total + 255) / 256, 8192L)), dim3(256), 0, s, q);
    LAUNCH_OK("pw_x3_pack");
    return 0;
}

static bool dw_lds_ok(const ConvDesc &d)
{
    return conv_is_depthwise(d) && (d.fs == 3 || d.fs == 5) && (d.stride == 1 || d.stride == 2) && conv_cnhw_contiguous(d) &&
           !d.residual && d.iw + 2 * d.pad <= 1024 && d.ow >= 1 && d.oh >= 1;
}

// depthwise 5x5 s1 p2 on small planes, two channels per workgroup (ffgpu_dw_pair.inc)
static bool dw_pair_ok(const ConvDesc &d)
{
    return dw_lds_ok(d) && d.fs == 5 && d.stride == 1 && d.pad == 2 && d.ic % 2 == 0 && d.iw % 2 == 0 && d.iw >= 6 && d.iw <= 40 && d.ih <= 40 &&
           d.act != 3 && !(d.flags & FFGPU_COMPAT_V6) && (long)d.ic * d.N * d.iw * d.ih < (1L << 30) && !knob(K_NO_DW_PAIR);
}

static int launch_dw_pair(const ConvDesc &d, hipStream_t s)
{
    constexpr int BR = 5;
    DwPairP p;
    p.in = d.in; p.filt = d.filt; p.out = d.out;
    p.W = d.iw; p.H = d.ih; p.N = d.N; p.rowlen = conv_k4(d) + 4;
    p.quads = (d.iw + 3) / 4; p.bands = (d.ih + BR - 1) / BR; p.TPI = p.quads * p.bands;
    p.LW = p.quads * 4 + 4; p.LH = p.bands * BR + 4;
    const int vec = d.iw % 4 == 0 ? 4 : 2;
    p.WQ = d.iw / vec;
    p.slope = d.act == 2 ? 0.1f : (d.act == 1 ? 0.f : 1.f);
    // frames per workgroup: as many as 256 threads and 64 KB of LDS take, then evened out over the workgroups of a pair
    const long plane2 = (long)p.LH * p.LW * 2;
    int NI = std::min(256 / p.TPI, (int)(64 * 1024 / 4 / plane2));
    NI = std::max(1, std::min(NI, d.N));
    if (const int f = knob(K_DWP_NI); f > 0) NI = std::min(f, NI);              // tuning only
    const int nb = (d.N + NI - 1) / NI;
    NI = (d.N + nb - 1) / nb;
    p.NI = NI;
    p.m_tpi = umulhi_magic(p.TPI); p.m_quads = umulhi_magic(p.quads); p.m_hwq = umulhi_magic((long)p.H * p.WQ); p.m_wq = umulhi_magic(p.WQ);      // every divisor >= 2 (dw_pair_ok)
    const size_t lds = (size_t)NI * plane2 * sizeof(float);
    const dim3 grid((unsigned)nb, (unsigned)(d.ic / 2));
    if (vec == 4) hipLaunchKernelGGL((k_dw_pair<5, BR, 4>), grid, dim3(256), lds, s, p);
    else          hipLaunchKernelGGL((k_dw_pair<5, BR, 2>), grid, dim3(256), lds, s, p);
    LAUNCH_OK("dw_pair");
    return 0;
}

static bool dense_small_ok(const ConvDesc &d)
{
    return d.groups == 1 && (d.fs == 3 || d.fs == 5) && d.ic <= 8;
}

// thin groups (2..7 input channels per group, grouped or dense): ffgpu_conv_thin.inc
static bool group_thin_ok(const ConvDesc &d)
{
    const int gic = d.groups >= 1 && d.ic % d.groups == 0 ? d.ic / d.groups : 0;
    const int rl = ((d.fs * d.fs * gic + 3) & ~3) + 4;
    return gic >= 2 && gic <= 7 && d.oc % d.groups == 0 && d.fs >= 1 && d.fs <= 11 && (long)d.oh * d.ow < (1L << 30) &&
           (long)(d.oc / d.groups) * rl <= THIN_WCAP && (long)d.ih * d.iw < (1L << 30) &&
           (long)d.groups * d.N * (((long)d.oh * d.ow + 255) / 256) < (1L << 31) && !(d.flags & FFGPU_COMPAT_V6 && d.fs == 5 && d.groups == d.ic);
}

static bool pw_gemm_ok(const ConvDesc &d)
{
    return pw_mfma_ok(d) && d.oc >= 128 && d.ic >= 64 && (long)d.N * d.iw * d.ih < (1L << 26);      // (32-bit lane offsets of 4 rows in the epilogue)
}

// dense K x K (any stride / padding / input strides) on the matrix cores: worth it from 8 input channels up (K >= 32 for a
// 2x2 filter); the first layer of a darknet cfg (3 channels) stays on the small-channel kernels
static bool igemm_ok(const ConvDesc &d)
{
    const long P = (long)d.N * d.oh * d.ow, K = (long)d.fs * d.fs * d.ic;
    return d.groups >= 1 && d.groups <= 16 && d.ic % d.groups == 0 && d.oc % d.groups == 0 &&
           d.fs >= 1 && d.fs <= 11 && d.ow >= 1 && d.oh >= 1 && P < (1L << 31) && K < (1L << 20) &&
           d.out_ns == (long)d.ow * d.oh && d.out_cs == (long)d.N * d.ow * d.oh && (!d.residual || (d.res_ns == d.out_ns && d.res_cs == d.out_cs));
}
// (per group: gic = ic / groups input channels, goc = oc / groups filters)
static int igemm_wm(const ConvDesc &d) { return d.oc / d.groups > 64 ? 2 : 1; }
// the 3x3 / stride 1 / pad 1 form with the vectorised gather (quads of output pixels: ow % 4 == 0; 16-byte aligned rows)
static bool igemm_vec(const ConvDesc &d)
{
    return d.fs == 3 && d.stride == 1 && d.pad == 1 && d.ow >= 4 && d.iw == d.ow && d.ih == d.oh &&
           (long)d.N * d.oh * ((d.ow + 3) & ~3) < (1L << 31) && !knob(K_IGEMM_NOVEC);
}
static int igemm_kc(const ConvDesc &d) { return igemm_vec(d) ? (igemm_wm(d) == 1 ? IG_KC3N : IG_KC3) : IG_KC; }
// split-K: a layer whose tiles do not fill the chip (768 resident workgroups: 3 per CU) and whose K loop is long is cut along K
// The factor is part of the PLAN: an executor stores it in ConvDesc::nsplit next to the packed image whose tail holds the partial
// sums, so a later change of the environment (NO_GRAPH executors launch kernel by kernel) cannot outgrow that room.  Note on
// rounding: with S > 1 an output is S k-ordered fmaf chains added in split order instead of one chain, and S depends on the tile
// count -- i.e. on the batch size -- so a dense K x K layer of a small batch and of a large batch can differ in the last bits
// (same tolerance class; FFGPU_IGEMM_SPLIT=1 keeps the single chain everywhere).
static int igemm_split(const ConvDesc &d)
{
    if (d.nsplit > 0) return d.nsplit;
    const int f = knob(K_IGEMM_SPLIT);
    const int WM = d.oc / d.groups > 64 ? 2 : 1, TN = WM == 2 ? 128 : 256, kc = igemm_kc(d);
    const long P = (long)d.N * d.oh * (igemm_vec(d) ? (d.ow + 3) & ~3 : d.ow), tiles = ((P + TN - 1) / TN) * ((d.oc / d.groups + 64 * WM - 1) / (64 * WM)) * d.groups;      // (all groups in one grid)
    const int nchunks = (d.fs * d.fs * (d.ic / d.groups) + kc - 1) / kc;
    int S = 1;
    const long slots = 768;                                         // the split stops where tiles x S would pass this many workgroups
    while (S < 8 && tiles * (S + 1) <= slots && nchunks / (S + 1) >= 4) S++;
    if (f >= 1 && f <= 16) S = std::min(f, std::max(1, nchunks));
    return S;
}
static size_t igemm_part_floats(const ConvDesc &d) { const int S = igemm_split(d); return S > 1 ? (size_t)S * d.oc * d.N * d.oh * d.ow : 0; }      // (every group's parts: the groups run in one grid)
static void igemm_dims(const ConvDesc &d, int &WM, int &nchunks, int &ntm, int &img)
{
    WM = igemm_wm(d);
    const int kc = igemm_kc(d);
    nchunks = (d.fs * d.fs * (d.ic / d.groups) + kc - 1) / kc; ntm = (d.oc / d.groups + 64 * WM - 1) / (64 * WM);
    img = nchunks * (kc / 2) * WM * 128 + 2 * 64 * WM;
}

// split-bf16 form of the dense 3x3 / stride 1 / pad 1 layer (ffgpu_conv_x3.inc): CNHW-style strided input through a plain pointer, one group,
// input channels in whole blocks of 8, 32-bit lane offsets.  MT (16-row blocks per wave: part of the packed image's layout) is frozen with the plan in ConvDesc::x3_mt.
static bool ig_x3_ok(const ConvDesc &d)
{
    if (!(igemm_ok(d) && d.groups == 1 && !d.in_ind && !(d.flags & FFGPU_F_BATCH_INPUT) && d.ic >= 8 && d.ic % 8 == 0 && d.in_cs > 0 && d.in_ns > 0 &&
          (long)(d.ic + 32) * d.in_cs + (long)d.N * d.in_ns < (1L << 30))) return false;
    if (d.fs == 1)        // the pointwise form: contiguous CNHW, whole quads of the flat pixel space
        return d.stride == 1 && d.pad == 0 && conv_cnhw_contiguous(d) && ((long)d.N * d.ih * d.iw) % 4 == 0;
    if ((long)d.N * d.oh * ((d.ow + 3) & ~3) >= (1L << 31) - 64 || d.ow < 4) return false;
    if (d.fs == 3 && d.stride == 2 && d.pad == 1)      // the downsampling form: even planes
        return d.iw == 2 * d.ow && d.ih == 2 * d.oh && knob(K_IGX3_S2) != 0;
    return igemm_vec(d) && d.iw >= 4;
}
// waves per workgroup: 4 (two workgroups per CU, out of phase) measured ahead of 8 on every stride-1 layer; the stride-2 form (256 VGPRs, a few spills in its
// 4-wave build) is level or ahead with 8
static int ig_x3_nw(const ConvDesc &d) { const int f = knob(K_IGX3_NW); return f == 8 || f == 4 ? f : (d.stride == 2 ? 8 : 4); }
static long ig_x3_npg(const ConvDesc &d) { const long ntn = ((long)d.N * d.oh * (d.fs == 1 ? d.ow : (d.ow + 3) & ~3) + 63) / 64; return (ntn + ig_x3_nw(d) - 1) / ig_x3_nw(d); }
// 16-row blocks per wave: 4 (every split input value feeds 64 output channels) while that leaves enough workgroups, else 2
static int ig_x3_mt_plan(const ConvDesc &d)
{
    const int f = knob(K_IGX3_MT);
    if (f == 4 || f == 2 || f == 1) return f;
    if (d.oc <= 32 || d.stride == 2) return d.oc <= 16 ? 1 : 2;     // (stride 2: nine input columns per lane -- no registers for four blocks)
    return ig_x3_npg(d) * ((d.oc + 63) / 64) >= knob(K_IGX3_MT4_WGS) ? 4 : 2;
}
static int ig_x3_mt(const ConvDesc &d) { const int m = d.x3_mt == 4 || d.x3_mt == 2 || d.x3_mt == 1 ? d.x3_mt : ig_x3_mt_plan(d); return d.stride == 2 && m > 2 ? 2 : m; }
static void ig_x3_dims(const ConvDesc &d, int &MT, int &ngr, int &nrb, int &ntm) { MT = ig_x3_mt(d); ngr = (d.fs * (d.ic / 8) + 3) / 4; nrb = (d.oc + 15) / 16; ntm = (nrb + MT - 1) / MT; }
// The sparse form of a yolo head's input layer (ConvDesc::sp_classes; ffgpu_conv_x3.inc "SPARSE HEAD"): form sp = 1 (box pass: one 16-row block at MT = 1) and
// sp = 2 (class pass: 3 x classes rows at the layer's own MT) read row-permuted images that lie BEHIND the regular one in the layer's packed image -- sized,
// filled and refreshed with it by this table's one rule (conv_image, ffgpu_pw_pack_floats, ffgpu_pw_pack).
static bool ig_x3_sparse(const ConvDesc &d) { return d.sp_classes > 0 && d.fs == 1 && d.oc == 3 * (5 + d.sp_classes); }
static void ig_x3_sp_dims(const ConvDesc &d, int sp, int &MT, int &ngr, int &nrb, int &ntm)
{
    ig_x3_dims(d, MT, ngr, nrb, ntm);
    if (sp == 1) { MT = 1; nrb = 1; }
    if (sp == 2) nrb = (3 * d.sp_classes + 15) / 16;
    ntm = (nrb + MT - 1) / MT;
}
static size_t ig_x3_sp_dwords(const ConvDesc &d, int sp) { int MT, ngr, nrb, ntm; ig_x3_sp_dims(d, sp, MT, ngr, nrb, ntm); return (size_t)ntm * ngr * 3 * d.fs * MT * 256; }
static size_t ig_x3_img_dwords(const ConvDesc &d) { return ig_x3_sp_dwords(d, 0) + (ig_x3_sparse(d) ? ig_x3_sp_dwords(d, 1) + ig_x3_sp_dwords(d, 2) : 0); }
// AUTO takes it where it wins over k_conv_igemm (tools/igemm_bench.py): enough (channel tile, pixel range) workgroups to fill the chip -- the
// fp32 kernel has split-K for the small planes, this one has not.  FFGPU_IG_X3=0: never.
static bool ig_x3_auto(const ConvDesc &d)
{
    if (!ig_x3_ok(d)) return false;
    const int ntm = ((d.oc + 15) / 16 + ig_x3_mt_plan(d) - 1) / ig_x3_mt_plan(d);      // (never from ConvDesc::x3_mt: AUTO is the same question whether or not a plan exists)
    // pointwise form: the heads' layers of yolo-fastest (>= 96 channels either side) -- alone 15.6 -> 11.8 us (120 -> 120 on 20x20 x 64) and 24.9 -> 16.7 us
    // (120 -> 255), the 10x10 ones level; with four chains in flight the seven layers together: 193.9 k -> 202.3 k frames/s (same box, alternating).  FFGPU_PW_X3S=0: never
    if (d.fs == 1)
        return knob(K_PW_X3S) != 0 && d.ic >= knob(K_PWX3S_MIN_IC) && d.oc >= knob(K_PWX3S_MIN_OC) &&
               ig_x3_npg(d) * ntm >= knob(K_PWX3S_MIN_WGS);
    if (knob(K_IG_X3) == 0) return false;
    return d.ic >= knob(K_IGX3_MIN_IC) && ig_x3_npg(d) * ntm >= knob(K_IGX3_MIN_WGS);
}
static int ig_x3_pack(const ConvDesc &d, float *pk, hipStream_t s)
{
    unsigned *img = reinterpret_cast<unsigned *>(pk);
    for (int sp = 0; sp <= (ig_x3_sparse(d) ? 2 : 0); sp++) {         // the regular image, then a sparse head's two
        IgX3PackP q;
        int nrb;
        q.filt = d.filt; q.pk = img; q.ic = d.ic; q.oc = d.oc; q.k4 = conv_k4(d); q.fs = d.fs; q.sp = sp; q.classes = d.sp_classes;
        ig_x3_sp_dims(d, sp, q.MT, q.ngr, nrb, q.ntm);
        q.nunits = d.fs * (d.ic / 8);
        const long total = (long)ig_x3_sp_dwords(d, sp);
        hipLaunchKernelGGL(k_conv_x3_pack, dim3((unsigned)std::min((total + 255) / 256, 8192L)), dim3(256), 0, s, q);
        LAUNCH_OK("conv_x3_pack");
        img += total;
    }
    return 0;
}

static int conv_pick(const ConvDesc &d, int variant)
{
    if (variant != FFGPU_K_AUTO) return variant;
    if (d.kernel) return d.kernel;                       // frozen with the plan (ffgpu_conv_plan)
    if (knob(K_FORCE_GENERIC)) return FFGPU_K_GENERIC;
    if (dw_stream_ok(d)) return FFGPU_K_DW_STREAM;
    if (!(d.flags & FFGPU_BF16_PW) && pw_x3t_auto(d)) return FFGPU_K_PW_X3T;                  // (config[2]: the tiled form, round 5)
    if (!(d.flags & FFGPU_BF16_PW) && d.fs == 1 && ig_x3_auto(d)) return FFGPU_K_CONV_X3;     // (ahead of k_pw_x3 wherever both apply: config[2] 171 against 199 us on one box)
    if (!(d.flags & FFGPU_BF16_PW) && pw_x3_auto(d)) return FFGPU_K_PW_X3;
    if ((d.flags & FFGPU_BF16_PW) && pw_gemm_ok(d) && d.oc >= 128 && d.ic >= 128 && (long)d.N * d.iw * d.ih >= 16384) return FFGPU_K_PW_BF16;   // opt-in only
    if (pw_gemm_ok(d) && d.oc >= knob(K_PWG_MIN_OC) && d.ic >= knob(K_PWG_MIN_IC) && (long)d.N * d.iw * d.ih >= 16384 && !knob(K_NO_PW_GEMM)) return FFGPU_K_PW_GEMM;
    if (pw_mfma_ok(d)) return FFGPU_K_PW_MFMA;
    if (dw_lds_ok(d)) return FFGPU_K_DW_LDS;
    if (dense_small_ok(d)) return FFGPU_K_DENSE_SMALL;
    const bool igemm_on = !knob(K_NO_IGEMM);
    if (igemm_on && ig_x3_auto(d)) return FFGPU_K_CONV_X3;
    if (igemm_on && igemm_ok(d) && d.ic / d.groups >= 8) return FFGPU_K_IGEMM;
    if (group_thin_ok(d) && !knob(K_NO_GROUP_THIN)) return FFGPU_K_GROUP_THIN;
    return FFGPU_K_GENERIC;
}

// Plan-time freeze (executors; ADVICE r04): the kernel AUTO picks NOW, and the two numbers that shape its packed image (for k_conv_x3 and k_pw_x3t the
// tile form the image is laid out for).  Everything that sizes, fills or reads ConvDesc::wpack goes through conv_pick(d, AUTO), which returns d.kernel once it is set.
void ffgpu_conv_plan(ConvDesc &d)
{
    d.kernel = 0; d.nsplit = 0; d.x3_mt = 0;
    const int k = conv_pick(d, FFGPU_K_AUTO);
    if (k == FFGPU_K_IGEMM) d.nsplit = igemm_split(d);
    if (k == FFGPU_K_CONV_X3) d.x3_mt = ig_x3_mt_plan(d);
    if (k == FFGPU_K_PW_X3T) d.x3_mt = pwx3t_rb_env();
    d.kernel = k;
}

template <int NV, int U, bool NT>
static void dw_stream_launch(const DwStreamP &p, hipStream_t s)
{
    const long blocks = (p.ntasks + 3) / 4;
    hipLaunchKernelGGL((k_dw3_stream<NV, U, NT>), dim3((unsigned)blocks), dim3(256), 0, s, p);
}

static int launch_dw_stream(const ConvDesc &d, const float *, hipStream_t s)
{
    // defaults from the sweep in profiles/r01_dw3_tuning.txt: 4-row tasks walked in address order keep the
    // chip-wide access window compact (5.95 TB/s vs 4.95 TB/s for one long stream per wave)
    // NT: outputs of 128 MB and more are streamed past the caches (ffgpu_dw_stream.inc DW_NT_MASK; FFGPU_DW_NT=0 / 1 forces)
    const int U = knob(K_DW_U), BAND = knob(K_DW_BAND);
    const int nt_env = knob(K_DW_NT), NT = nt_env >= 0 ? nt_env : ((long)d.ic * d.N * d.iw * d.ih * 4 >= (128L << 20));
    DwStreamP p;
    p.in = d.in; p.filt = d.filt; p.out = d.out; p.residual = nullptr;
    p.W = d.iw; p.H = d.ih; p.planes = d.ic * d.N; p.N = d.N;
    p.lpr = d.iw / 4;
    const int NV = p.lpr > 64 ? 2 : 1;
    p.G = NV == 1 ? 64 / p.lpr : 1;
    const long pgroups = ((long)p.planes + p.G - 1) / p.G;
    // enough wave tasks to fill 256 CUs x 16 waves; whole planes per wave when there are plenty of planes
    int nb = BAND > 0 ? (d.ih + BAND - 1) / BAND : (int)((6144 + pgroups - 1) / pgroups);
    if (nb < 1) nb = 1;
    if (nb > (d.ih + 3) / 4) nb = (d.ih + 3) / 4;
    int band = (d.ih + nb - 1) / nb;
    band = (band + U - 1) / U * U;
    p.band = band; p.nbands = (d.ih + band - 1) / band;
    p.rowlen = conv_k4(d) + 4; p.act = d.act; p.res_act = 0;
    p.ntasks = pgroups * p.nbands;
    p.nblocks = (p.ntasks + 3) / 4;
    p.xcd_remap = knob(K_DW_XCD);
    if (NV == 1) {
        if (U == 1)      { if (NT) dw_stream_launch<1, 1, true>(p, s); else dw_stream_launch<1, 1, false>(p, s); }
        else if (U == 2) { if (NT) dw_stream_launch<1, 2, true>(p, s); else dw_stream_launch<1, 2, false>(p, s); }
        else             { if (NT) dw_stream_launch<1, 4, true>(p, s); else dw_stream_launch<1, 4, false>(p, s); }
    } else {
        if (U == 1)      { if (NT) dw_stream_launch<2, 1, true>(p, s); else dw_stream_launch<2, 1, false>(p, s); }
        else if (U == 2) { if (NT) dw_stream_launch<2, 2, true>(p, s); else dw_stream_launch<2, 2, false>(p, s); }
        else             { if (NT) dw_stream_launch<2, 4, true>(p, s); else dw_stream_launch<2, 4, false>(p, s); }
    }
    LAUNCH_OK("dw3_stream");
    return 0;
}

template <int OT, int KSP, int NW>
static int pw_launch_t(const PwP &p, int ocblocks, size_t lds, hipStream_t s)
{
    if (lds_allow((const void *)k_pw_mfma<OT, KSP, NW>, lds, "pw_mfma")) return -1;
    long gx = KSP == 1 ? (p.nstrips + NW - 1) / NW : p.nstrips;
    const long cap = 256L * 8 / ocblocks > 256 ? 256L * 8 / ocblocks : 256;
    if (gx > cap) gx = cap;
    hipLaunchKernelGGL((k_pw_mfma<OT, KSP, NW>), dim3((unsigned)gx, (unsigned)ocblocks), dim3(NW * 64), lds, s, p);
    LAUNCH_OK("pw_mfma");
    return 0;
}

template <int OT, int KSP>
static int pw_launch(const PwP &p, int ocblocks, hipStream_t s)
{
    const size_t lds = ((size_t)p.k4 * OT * 16 + OT * 32 + (KSP > 1 ? (size_t)(KSP - 1) * OT * 16 * 64 : 0)) * sizeof(float);
    // a big weight image limits workgroups per CU: 8 waves share it so 4 waves per SIMD keep the MFMA pipe fed
    if (KSP == 1 && lds > 40 * 1024) return pw_launch_t<OT, KSP, 8>(p, ocblocks, lds, s);
    return pw_launch_t<OT, KSP, 4>(p, ocblocks, lds, s);
}

// output-channel tiles per wave for a pointwise layer (shared by the plan-time weight packer):
// as many as the accumulators allow when there are plenty of pixel strips (the input is then read
// once per 64 channels), fewer when strips are scarce so the launch still has >= ~1500 waves.
static int pw_ot(int oc, long nstrips)
{
    int ot = oc <= 16 ? 1 : (oc <= 32 ? 2 : (oc <= 48 ? 3 : 4));
    const long target = 1536;                        // (the shape alone: pack and launch must agree on it)
    while (ot > 1 && nstrips * ((oc + ot * 16 - 1) / (ot * 16)) < target) ot = ot == 3 ? 2 : ot / 2;
    return ot;
}

static int launch_pw_mfma(const ConvDesc &d, const float *image, hipStream_t s)
{
    PwP p;
    p.in = d.in; p.filt = d.filt; p.out = d.out; p.residual = d.residual;
    p.P = (long)d.N * d.iw * d.ih; p.ic = d.ic; p.oc = d.oc; p.k4 = (d.ic + 3) & ~3;
    p.act = d.act; p.res_act = d.res_act;
    p.nstrips = (p.P + 63) / 64;
    p.wpack = image;                     // (none: the kernel builds its LDS image from the filter rows)
    const int OT = pw_ot(d.oc, p.nstrips), ocblocks = (d.oc + OT * 16 - 1) / (OT * 16);
    // still too few waves and a long K loop: let the 4 waves of a workgroup split K (the 10x10 tail)
    const long ks_waves = 1024;
    const bool ksplit = p.nstrips * ocblocks < ks_waves && p.k4 >= 32;
    switch (OT) {
    case 1: return ksplit ? pw_launch<1, 4>(p, ocblocks, s) : pw_launch<1, 1>(p, ocblocks, s);
    case 2: return ksplit ? pw_launch<2, 4>(p, ocblocks, s) : pw_launch<2, 1>(p, ocblocks, s);
    case 3: return ksplit ? pw_launch<3, 4>(p, ocblocks, s) : pw_launch<3, 1>(p, ocblocks, s);
    default: return ksplit ? pw_launch<4, 4>(p, ocblocks, s) : pw_launch<4, 1>(p, ocblocks, s);
    }
}

// plan-time packing of a pointwise layer's LDS image (A fragments + scale'/bias' per channel block)
struct PwPackP { const float *filt; float *pk; int ic, oc, k4, OT, ocblocks; };
__global__ void k_pw_pack(PwPackP p)
{
    const int ksteps = p.k4 >> 2, rl = p.k4 + 4;
    const int img = ksteps * p.OT * 64 + p.OT * 32;
    const int total = img * p.ocblocks;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int blk = i / img, j = i - blk * img, oc0 = blk * p.OT * 16;
        float v = 0.f;
        if (j < ksteps * p.OT * 64) {
            const int l = j & 63, t = (j >> 6) % p.OT, ks = (j >> 6) / p.OT;
            const int o = oc0 + 16 * t + (l & 15), ci = 4 * ks + (l >> 4);
            if (o < p.oc) v = p.filt[(long)o * rl + ci];
        } else {
            const int k = j - ksteps * p.OT * 64, o = oc0 + (k >> 1);
            if (o < p.oc) v = p.filt[(long)o * rl + p.k4 + (k & 1)];
        }
        p.pk[i] = v;
    }
}
static void pw_mfma_dims(const ConvDesc &d, int &k4, int &OT, int &ocblocks) { k4 = (d.ic + 3) & ~3; OT = pw_ot(d.oc, ((long)d.N * d.iw * d.ih + 63) / 64); ocblocks = (d.oc + OT * 16 - 1) / (OT * 16); }
static size_t pw_mfma_img_dwords(const ConvDesc &d) { int k4, OT, ocblocks; pw_mfma_dims(d, k4, OT, ocblocks); return ((size_t)(k4 / 4) * OT * 64 + OT * 32) * ocblocks; }
static int pw_mfma_pack(const ConvDesc &d, float *pk, hipStream_t s)
{
    PwPackP q;
    q.filt = d.filt; q.pk = pk; q.ic = d.ic; q.oc = d.oc;
    pw_mfma_dims(d, q.k4, q.OT, q.ocblocks);
    const int total = ((q.k4 / 4) * q.OT * 64 + q.OT * 32) * q.ocblocks;
    hipLaunchKernelGGL(k_pw_pack, dim3((total + 255) / 256), dim3(256), 0, s, q);
    LAUNCH_OK("pw_pack");
    return 0;
}

// waves per workgroup of the pointwise GEMM: 8 (256-channel tiles: the input chunk shared by twice as many waves) from 256 filters up
static int pwg32_wm(const ConvDesc &d) { const int f = knob(K_PWG_WM); return f == 4 || f == 8 ? f : (d.oc >= 256 - 8 ? 8 : 4); }
static void pwg32_dims(const ConvDesc &d, int &nchunks, int &ntm) { nchunks = (d.ic + PWG_KC - 1) / PWG_KC; ntm = (d.oc + 32 * pwg32_wm(d) - 1) / (32 * pwg32_wm(d)); }
static int pwg32_img(const ConvDesc &d) { int nc, ntm; pwg32_dims(d, nc, ntm); return nc * 512 * pwg32_wm(d) + 64 * pwg32_wm(d); }
static size_t pwg32_img_dwords(const ConvDesc &d) { int nc, ntm; pwg32_dims(d, nc, ntm); return (size_t)pwg32_img(d) * ntm; }

// one image per group, behind each other (igemm_pack), rounded to 64 floats; then the split-K partial sums
static size_t igemm_images_floats(const ConvDesc &d) { int WM, nchunks, ntm, img; igemm_dims(d, WM, nchunks, ntm, img); return ((size_t)img * ntm * d.groups + 63) & ~(size_t)63; }
static size_t igemm_img_dwords(const ConvDesc &d) { return igemm_images_floats(d) + igemm_part_floats(d); }
static int igemm_pack(const ConvDesc &d, float *pk, hipStream_t s)
{
    IgemmPackP q;
    int img;
    const int goc = d.oc / d.groups;
    q.K = d.fs * d.fs * (d.ic / d.groups); q.k4 = (q.K + 3) & ~3; q.oc = goc;
    igemm_dims(d, q.WM, q.nchunks, q.ntm, img);
    q.kc = igemm_kc(d);
    const long total = (long)img * q.ntm;
    for (int g = 0; g < d.groups; g++) {                          // one image per group, behind each other
        q.filt = d.filt + (long)g * goc * (q.k4 + 4); q.pk = pk + (long)g * total;
        hipLaunchKernelGGL(k_conv_igemm_pack, dim3((unsigned)std::min((total + 255) / 256, 4096L)), dim3(256), 0, s, q);
        LAUNCH_OK("conv_igemm_pack");
    }
    return 0;
}

static void pwbf16_dims(const ConvDesc &d, int &nchunks, int &ntm) { nchunks = (d.ic + PWB_KC - 1) / PWB_KC; ntm = (d.oc + 127) / 128; }
static size_t pwbf16_img_dwords(const ConvDesc &d) { int nchunks, ntm; pwbf16_dims(d, nchunks, ntm); return (size_t)(nchunks * 2048 + 256) * ntm; }
static int pwbf16_pack(const ConvDesc &d, float *pk, hipStream_t s)
{
    PwBf16PackP q;
    q.filt = d.filt; q.pk = reinterpret_cast<unsigned *>(pk); q.ic = d.ic; q.oc = d.oc; q.k4 = (d.ic + 3) & ~3;
    pwbf16_dims(d, q.nchunks, q.ntm);
    const int total = (q.nchunks * 2048 + 256) * q.ntm;
    hipLaunchKernelGGL(k_pw_bf16_pack, dim3((total + 255) / 256), dim3(256), 0, s, q);
    LAUNCH_OK("pw_bf16_pack");
    return 0;
}

static int pwg32_pack(const ConvDesc &d, float *pk, hipStream_t s)
{
    PwG32PackP q;
    q.filt = d.filt; q.pk = pk; q.ic = d.ic; q.oc = d.oc; q.k4 = (d.ic + 3) & ~3;
    pwg32_dims(d, q.nchunks, q.ntm);
    q.wm = pwg32_wm(d);
    const int total = pwg32_img(d) * q.ntm;
    hipLaunchKernelGGL(k_pw_gemm32_pack, dim3((total + 255) / 256), dim3(256), 0, s, q);
    LAUNCH_OK("pw_gemm32_pack");
    return 0;
}

static int launch_generic(const ConvDesc &d, const float *, hipStream_t s)
{
    const long total = (long)d.oc * d.N * d.oh * d.ow;
    hipLaunchKernelGGL(k_conv_generic, dim3(grid_for(total, 256, 256 * 32)), dim3(256), 0, s, d);
    LAUNCH_OK("conv_generic");
    return 0;
}

static int launch_group_thin(const ConvDesc &d, const float *, hipStream_t s)
{
    ThinGP p;
    p.in = d.in; p.in_ind = d.in_ind; p.filt = d.filt; p.out = d.out; p.residual = d.residual;
    p.N = d.N; p.iw = d.iw; p.ih = d.ih; p.ow = d.ow; p.oh = d.oh; p.gic = d.ic / d.groups; p.goc = d.oc / d.groups; p.groups = d.groups;
    p.fs = d.fs; p.stride = d.stride; p.pad = d.pad; p.act = d.act; p.res_act = d.res_act;
    p.k4 = (d.fs * d.fs * p.gic + 3) & ~3; p.rl = p.k4 + 4;
    p.in_cs = d.in_cs; p.in_ns = d.in_ns; p.out_cs = d.out_cs; p.out_ns = d.out_ns; p.res_cs = d.res_cs; p.res_ns = d.res_ns;
    p.tiles = (int)(((long)d.oh * d.ow + 255) / 256);
    const dim3 grid((unsigned)((long)p.tiles * d.N * d.groups));
    // outputs per lane and pass: every loaded input value feeds that many FMAs
#define THIN_LAUNCH(FS) do { \
        if (p.goc >= 7)      hipLaunchKernelGGL((k_conv_thin<8, FS>), grid, dim3(256), 0, s, p); \
        else if (p.goc >= 3) hipLaunchKernelGGL((k_conv_thin<4, FS>), grid, dim3(256), 0, s, p); \
        else                 hipLaunchKernelGGL((k_conv_thin<2, FS>), grid, dim3(256), 0, s, p); } while (0)
    if (d.fs == 3) THIN_LAUNCH(3); else if (d.fs == 5) THIN_LAUNCH(5); else THIN_LAUNCH(0);
#undef THIN_LAUNCH
    LAUNCH_OK("conv_thin");
    return 0;
}

static int launch_pw_gemm(const ConvDesc &d, const float *image, hipStream_t s)
{
    PwG32P p;                                 // LDS-tiled 32x32x2 GEMM (ffgpu_pw_gemm32.inc); the A operand comes from the packed image
    p.in = d.in; p.out = d.out; p.residual = d.residual;
    p.P = (long)d.N * d.iw * d.ih; p.ic = d.ic; p.oc = d.oc; p.act = d.act; p.res_act = d.res_act;
    pwg32_dims(d, p.nchunks, p.ntm);
    p.wm = pwg32_wm(d);
    p.img = pwg32_img(d);
    p.wpack = image;
    // resident workgroups per CU: 4 of the 4-wave form (LDS 33 KB, 16 waves), 3 of the 8-wave form (LDS 50 KB, 24 waves)
    const int slots = (p.wm == 8 ? 3 : 4) * device_cus();
    long ntn_main, ntn_narrow;
    split_main_narrow(p.P, p.ntm, slots, knob(K_PWG_NARROW) != 0, &ntn_main, &ntn_narrow);
    p.ntn = ntn_main;
    const long total = p.ntn * p.ntm;
    p.per_xcd = (int)((total + 7) / 8);
    p.dbg = knob(K_PWG_DBG);
    const dim3 grid((unsigned)(8 * p.per_xcd + ntn_narrow * p.ntm));
    if (p.wm == 8) hipLaunchKernelGGL(k_pw_gemm32<8>, grid, dim3(512), 0, s, p);
    else           hipLaunchKernelGGL(k_pw_gemm32<4>, grid, dim3(256), 0, s, p);
    LAUNCH_OK("pw_gemm32");
    return 0;
}

static int launch_pw_x3(const ConvDesc &d, const float *image, hipStream_t s)
{
    PwX3P p;
    p.in = d.in; p.out = d.out; p.residual = d.residual; p.filt = d.filt;
    p.P = (long)d.N * d.iw * d.ih; p.ic = d.ic; p.oc = d.oc; p.k4 = (d.ic + 3) & ~3; p.act = d.act; p.res_act = d.res_act;
    pwx3_dims(d, p.ksteps, p.nrb);
    p.wpack = reinterpret_cast<const unsigned *>(image);
    // M tile of 16 MT rows whose three-part image for all k-steps fits the LDS (3 KB per 16 rows and k-step)
    int MT = pw_x3_mt(d);
    while (MT > 1 && (size_t)p.ksteps * MT * 3072 > 144 * 1024) MT /= 2;
    const size_t lds = (size_t)p.ksteps * MT * 3072 + (size_t)MT * 128;
    if (lds > 160 * 1024 - 1024) { ffgpu_set_error("pw_x3: %d input channels are too many for the LDS-resident weight tile", d.ic); return -1; }
    p.ntm = (p.nrb + MT - 1) / MT;
    p.ntn = (p.P + 63) / 64;
    const int cus = device_cus(), per_cu = lds <= 72 * 1024 ? 2 : 1;                 // workgroups (8 waves, 2 per SIMD at 256 VGPRs ... 1 per SIMD each when two share a CU)
    long nslots = std::max(1L, (long)cus * per_cu / p.ntm);
    nslots = std::min(nslots, (p.ntn + 7) / 8);
    if (nslots >= 8) nslots &= ~7L;                               // a multiple of the XCD count: the channel tiles of a pixel range share an XCD's L2 (see the kernel)
    p.nslots = (int)nslots;
    const dim3 grid((unsigned)(nslots * p.ntm));
#define PWX3_LAUNCH(mt) do { if (lds_allow((const void *)k_pw_x3<mt>, lds, "pw_x3")) return -1; hipLaunchKernelGGL((k_pw_x3<mt>), grid, dim3(512), lds, s, p); } while (0)
    if (MT == 4) PWX3_LAUNCH(4); else if (MT == 2) PWX3_LAUNCH(2); else PWX3_LAUNCH(1);
#undef PWX3_LAUNCH
    LAUNCH_OK("pw_x3");
    return 0;
}

static int launch_pw_x3t(const ConvDesc &d, const float *image, hipStream_t s)
{
    PwX3tP p;
    p.in = d.in; p.out = d.out; p.residual = d.residual;
    p.P = (long)d.N * d.iw * d.ih; p.ic = d.ic; p.oc = d.oc; p.act = d.act; p.res_act = d.res_act;
    pwx3t_dims(d, p.nchunks, p.ntm);
    const int RBv = pwx3t_rb(d);
    p.img = (long)p.nchunks * xt_ach(RBv) + 2 * xt_tm(RBv);
    p.wpack = reinterpret_cast<const unsigned *>(image);
    const int slots = (RBv == 2 ? 2 : 3) * device_cus();          // resident workgroups: two of the 256-channel form per CU, three of the 128-channel one
    long ntn_main, ntn_narrow;
    split_main_narrow(p.P, p.ntm, slots, knob(K_PWXT_NARROW) != 0, &ntn_main, &ntn_narrow);
    p.ntn = ntn_main;
    const long total = p.ntn * p.ntm;
    p.per_xcd = (int)((total + 7) / 8);
    p.nmain = 8 * p.per_xcd; p.tpw = 1;
    if (knob(K_PWXT_PERSIST) && total > slots) {      // tuning: persistent workgroups over the main tiles (slots of them, a multiple of 8)
        p.nmain = slots / 8 * 8;
        p.tpw = (int)((8L * p.per_xcd + p.nmain - 1) / p.nmain);
    }
    p.dbg = knob(K_PWXT_DBG);
    { const int nt = knob(K_PWXT_NT); p.nt = nt >= 0 ? (nt != 0) : ((long)d.oc * p.P * 4 >= (128L << 20)); }
    const dim3 grid((unsigned)(p.nmain + ntn_narrow * p.ntm));
    p.dbg_t = nullptr;
#if XT_TRACE                                                        // lab builds: one traced launch, dumped as text (tile words) to FFGPU_PWXT_TRACE
    if (const char *tf = knob_text(K_PWXT_TRACE)) {
        const size_t nw = (size_t)((p.P + 31) / 32 + 4) * p.ntm * 8;
        unsigned long long *d_t = nullptr;
        if (hipMalloc(&d_t, nw * 8) != hipSuccess) return -1;
        (void)hipMemsetAsync(d_t, 0, nw * 8, s);
        p.dbg_t = d_t;
        if (RBv == 2) hipLaunchKernelGGL(k_pw_x3t<2>, grid, dim3(256), 0, s, p); else hipLaunchKernelGGL(k_pw_x3t<1>, grid, dim3(256), 0, s, p);
        (void)hipStreamSynchronize(s);
        std::vector<unsigned long long> h(nw);
        (void)hipMemcpy(h.data(), d_t, nw * 8, hipMemcpyDeviceToHost);
        (void)hipFree(d_t);
        if (FILE *fp = fopen(tf, "w")) {
            for (size_t i = 0; i < nw; i += 8) if (h[i]) fprintf(fp, "%llu %llu %llu %llu %llu %llu %llu\n", h[i], h[i + 1], h[i + 2], h[i + 3], h[i + 4], h[i + 5], h[i + 6]);
            fclose(fp);
        }
        return 0;
    }
#endif
    if (RBv == 2) hipLaunchKernelGGL(k_pw_x3t<2>, grid, dim3(256), 0, s, p);
    else          hipLaunchKernelGGL(k_pw_x3t<1>, grid, dim3(256), 0, s, p);
    LAUNCH_OK("pw_x3t");
    return 0;
}

static int launch_pw_bf16(const ConvDesc &d, const float *image, hipStream_t s)
{
    PwBf16P p;
    p.in = d.in; p.out = d.out; p.residual = d.residual;
    p.P = (long)d.N * d.iw * d.ih; p.ic = d.ic; p.oc = d.oc; p.act = d.act; p.res_act = d.res_act;
    pwbf16_dims(d, p.nchunks, p.ntm);
    p.img = p.nchunks * 2048 + 256;
    p.wpack = reinterpret_cast<const unsigned *>(image);
    p.ntn = (p.P + 127) / 128;
    p.per_xcd = (int)((p.ntn * p.ntm + 7) / 8);
    hipLaunchKernelGGL(k_pw_bf16, dim3((unsigned)(8 * p.per_xcd)), dim3(256), 0, s, p);
    LAUNCH_OK("pw_bf16");
    return 0;
}

// the launch of one form: sp = 0 the layer as planned, sp = 1 / 2 the box and the class pass of a sparse head on their images behind the regular one
static int launch_conv_x3_form(const ConvDesc &d, const float *image, int sp, hipStream_t s)
{
    IgX3P p;
    int MT;
    p.in = d.in; p.out = d.out; p.residual = d.residual; p.filt = d.filt;
    p.iw = d.iw; p.ih = d.ih; p.ow = d.ow; p.oh = d.oh; p.ic = d.ic; p.oc = d.oc; p.k4 = conv_k4(d); p.act = d.act; p.res_act = d.res_act;
    p.in_cs = (unsigned)d.in_cs; p.in_ns = (unsigned)d.in_ns;
    ig_x3_sp_dims(d, sp, MT, p.ngr, p.nrb, p.ntm);
    p.nunits = d.fs * (d.ic / 8);
    p.wpack = reinterpret_cast<const unsigned *>(image) + (sp >= 1 ? ig_x3_sp_dwords(d, 0) : 0) + (sp == 2 ? ig_x3_sp_dwords(d, 1) : 0);
    p.sp_list = d.sp_list; p.sp_ctr = d.sp_ctr; p.sp_classes = d.sp_classes; p.sp_thresh = d.sp_thresh;
    p.sp_cap = (int)((long)d.N * d.oh * d.ow / 4);
    const int NW = ig_x3_nw(d);
    p.owp = d.fs == 1 ? d.ow : (d.ow + 3) & ~3; p.P = (long)d.N * d.oh * d.ow; p.Pp = (long)d.N * d.oh * p.owp;
    p.ntn = (p.Pp + 63) / 64; p.npg = (p.ntn + NW - 1) / NW;
    const long nblk = 8 * (long)p.ntm * ((p.npg + 7) / 8);
    if (nblk > (1L << 30)) { ffgpu_set_error("conv_x3: too many tiles"); return -1; }
    const size_t lds = (size_t)2 * 3 * d.fs * MT * 1024 + (size_t)MT * 128;
    const dim3 grid((unsigned)nblk);
    if (sp) {
#define IGX3_LAUNCH_SP(mt, nw, spv) do { if (lds_allow((const void *)k_conv_x3<mt, nw, 1, 1, spv>, lds, "conv_x3")) return -1; hipLaunchKernelGGL((k_conv_x3<mt, nw, 1, 1, spv>), grid, dim3(64 * nw), lds, s, p); } while (0)
        if (sp == 1) { if (NW == 8) IGX3_LAUNCH_SP(1, 8, 1); else IGX3_LAUNCH_SP(1, 4, 1); }
        else if (NW == 8) { if (MT == 4) IGX3_LAUNCH_SP(4, 8, 2); else if (MT == 2) IGX3_LAUNCH_SP(2, 8, 2); else IGX3_LAUNCH_SP(1, 8, 2); }
        else              { if (MT == 4) IGX3_LAUNCH_SP(4, 4, 2); else if (MT == 2) IGX3_LAUNCH_SP(2, 4, 2); else IGX3_LAUNCH_SP(1, 4, 2); }
#undef IGX3_LAUNCH_SP
        LAUNCH_OK(sp == 1 ? "conv_x3 (box pass)" : "conv_x3 (class pass)");
        return 0;
    }
#define IGX3_LAUNCH(mt, nw, fs) do { if (lds_allow((const void *)k_conv_x3<mt, nw, fs>, lds, "conv_x3")) return -1; hipLaunchKernelGGL((k_conv_x3<mt, nw, fs>), grid, dim3(64 * nw), lds, s, p); } while (0)
#define IGX3_LAUNCH2(mt, nw) do { if (d.fs == 1) IGX3_LAUNCH(mt, nw, 1); else IGX3_LAUNCH(mt, nw, 3); } while (0)
    if (d.stride == 2) {
#define IGX3_LAUNCH_S2(mt, nw) do { if (lds_allow((const void *)k_conv_x3<mt, nw, 3, 2>, lds, "conv_x3")) return -1; hipLaunchKernelGGL((k_conv_x3<mt, nw, 3, 2>), grid, dim3(64 * nw), lds, s, p); } while (0)
        if (NW == 8) { if (MT == 2) IGX3_LAUNCH_S2(2, 8); else IGX3_LAUNCH_S2(1, 8); }
        else         { if (MT == 2) IGX3_LAUNCH_S2(2, 4); else IGX3_LAUNCH_S2(1, 4); }
#undef IGX3_LAUNCH_S2
    } else
    if (NW == 8) { if (MT == 4) IGX3_LAUNCH2(4, 8); else if (MT == 2) IGX3_LAUNCH2(2, 8); else IGX3_LAUNCH2(1, 8); }
    else         { if (MT == 4) IGX3_LAUNCH2(4, 4); else if (MT == 2) IGX3_LAUNCH2(2, 4); else IGX3_LAUNCH2(1, 4); }
#undef IGX3_LAUNCH2
#undef IGX3_LAUNCH
    LAUNCH_OK("conv_x3");
    return 0;
}

// a layer marked as a sparse head's (with its list and counter): the box pass, then the class pass over what the box pass listed; every other layer as planned
static int launch_conv_x3(const ConvDesc &d, const float *image, hipStream_t s)
{
    if (!(ig_x3_sparse(d) && d.sp_list && d.sp_ctr && !d.residual)) return launch_conv_x3_form(d, image, 0, s);
    return launch_conv_x3_form(d, image, 1, s) || launch_conv_x3_form(d, image, 2, s) ? -1 : 0;
}

// what the launch of the layer in front of a yolo head does, as one line: the sparse pair with its grids and the list's capacity, or the kernel's name
int ffgpu_conv_sparse_head_line(const ConvDesc &d0, int classes, bool wanted, char *buf, size_t cap)
{
    ConvDesc d = d0;
    ffgpu_conv_plan(d);
    if (!wanted || !ffgpu_conv_sparse_head_ok(d, classes)) return snprintf(buf, cap, "dense %s", ffgpu_conv_kernel_name(d, FFGPU_K_AUTO));
    d.sp_classes = classes;
    int MT, ngr, nrb, ntm1, ntm2;
    ig_x3_sp_dims(d, 1, MT, ngr, nrb, ntm1);
    ig_x3_sp_dims(d, 2, MT, ngr, nrb, ntm2);
    const long slots = (ig_x3_npg(d) + 7) / 8 * 8;
    return snprintf(buf, cap, "sparse box<1,%d> rows=15 grid=%ld class<%d,%d> rows=%d grid=%ld quads=%ld image=%zu", ig_x3_nw(d), slots * ntm1, MT, ig_x3_nw(d),
                    3 * classes, slots * ntm2, (long)d.N * d.oh * d.ow / 4, ig_x3_img_dwords(d));
}

bool ffgpu_conv_sparse_head_ok(const ConvDesc &d, int classes)
{
    return classes >= 1 && d.fs == 1 && d.oc == 3 * (5 + classes) && !d.residual && conv_pick(d, FFGPU_K_AUTO) == FFGPU_K_CONV_X3 && ig_x3_ok(d);
}

static int launch_igemm(const ConvDesc &d, const float *image, hipStream_t s)
{
    IgemmP p;
    int WM;
    const int gic = d.ic / d.groups, goc = d.oc / d.groups;
    p.in = d.in; p.in_ind = d.in_ind;
    p.P = (long)d.N * d.oh * d.ow; p.in_cs = d.in_cs; p.in_ns = d.in_ns;
    p.N = d.N; p.iw = d.iw; p.ih = d.ih; p.ic = gic; p.ow = d.ow; p.oh = d.oh; p.oc = goc; p.fs = d.fs; p.stride = d.stride; p.pad = d.pad;
    p.K = d.fs * d.fs * gic; p.act = d.act; p.res_act = d.res_act;
    igemm_dims(d, WM, p.nchunks, p.ntm, p.img);
    p.m_ff = umulhi_magic((long)d.fs * d.fs); p.m_f = umulhi_magic(d.fs);      // (1x1: 0, the kernel then does not divide)
    const size_t per_group = (size_t)p.img * p.ntm;
    p.nsplit = igemm_split(d);
    p.part = p.nsplit > 1 ? const_cast<float *>(image) + igemm_images_floats(d) : nullptr;      // (behind the images: [group][split][filter][pixel])
    const int TN = WM == 2 ? 128 : 256;
    p.owp = (d.ow + 3) & ~3; p.Pp = (long)d.N * d.oh * p.owp;
    p.ntn = ((igemm_vec(d) ? p.Pp : p.P) + TN - 1) / TN;
    const long total = p.ntn * p.ntm * p.nsplit * d.groups;        // conv-v0.c:46-51: every group's tiles in ONE grid
    if (total > (1L << 28)) { ffgpu_set_error("conv_igemm: too many tiles"); return -1; }
    p.per_xcd = (int)((total + 7) / 8);
    p.groups = d.groups; p.in_off = 0; p.g_in = (long)gic * d.in_cs; p.g_out = (long)goc * d.out_cs; p.g_w = (long)per_group;
    p.out = d.out; p.residual = d.residual; p.wpack = image;
    const dim3 grid((unsigned)(8 * p.per_xcd));
    if (igemm_vec(d)) {
        if (WM == 2)        hipLaunchKernelGGL((k_conv_igemm<2, true>), grid, dim3(256), 0, s, p);
        else if (goc <= 32) hipLaunchKernelGGL((k_conv_igemm<1, true, true>), grid, dim3(256), 0, s, p);
        else                hipLaunchKernelGGL((k_conv_igemm<1, true>), grid, dim3(256), 0, s, p);
    } else {
        if (WM == 2)        hipLaunchKernelGGL((k_conv_igemm<2, false>), grid, dim3(256), 0, s, p);
        else if (goc <= 32) hipLaunchKernelGGL((k_conv_igemm<1, false, true>), grid, dim3(256), 0, s, p);
        else                hipLaunchKernelGGL((k_conv_igemm<1, false>), grid, dim3(256), 0, s, p);
    }
    if (p.nsplit > 1) {
        IgemmRedP q;
        const int K = d.fs * d.fs * gic, k4 = (K + 3) & ~3;
        q.part = p.part; q.filt = d.filt; q.residual = d.residual; q.out = d.out; q.P = p.P; q.oc = d.oc; q.goc = goc;
        q.nsplit = p.nsplit; q.rl = k4 + 4; q.k4 = k4; q.act = d.act; q.res_act = d.res_act;
        hipLaunchKernelGGL(k_conv_igemm_reduce, dim3((unsigned)std::min(((long)d.oc * p.P + 255) / 256, 65536L)), dim3(256), 0, s, q);
    }
    LAUNCH_OK("conv_igemm");
    return 0;
}

static int launch_dw_lds(const ConvDesc &d, const float *, hipStream_t s)
{
    if (dw_pair_ok(d)) return launch_dw_pair(d, s);
    DwLdsP p;
    p.in = d.in; p.filt = d.filt; p.out = d.out;
    p.W = d.iw; p.H = d.ih; p.OW = d.ow; p.OH = d.oh; p.planes = d.ic * d.N; p.N = d.N;
    p.fs = d.fs; p.stride = d.stride; p.pad = d.pad; p.act = d.act; p.flags = d.flags; p.rowlen = conv_k4(d) + 4;
    // staged row: the padded input row plus the columns a trailing partial quad may touch, 16-byte pitch
    p.LW = (((d.ow + 3) / 4 * 4 - 1) * d.stride + d.fs + 4 + 3) & ~3;
    if (p.LW < d.iw + 2 * d.pad) p.LW = (d.iw + 2 * d.pad + 3) & ~3;
    // band height: ~1024 outputs per plane-band, input window <= 32 KB
    int BH = d.oh;
    while (BH > 1 && ((long)BH * d.ow > 1024 || ((long)(BH - 1) * d.stride + d.fs) * p.LW * 4 > 32 * 1024)) BH = (BH + 1) / 2;
    if (const int f = knob(K_DWL_BH); f > 0) BH = std::min(f, d.oh);       // tuning only
    p.BH = BH; p.nbands = (d.oh + BH - 1) / BH;
    p.IH = (BH - 1) * d.stride + d.fs;
    int NPL = 1;
    // (tools/tune_dwl.py: the per-item skeleton -- staging, barriers, index arithmetic -- dominates on the small planes
    //  of the heads, so items are as large as LDS allows while a few per CU remain)
    while (NPL < 16 && (long)(NPL * 2) * BH * d.ow <= 4096 && (long)(NPL * 2) * p.IH * p.LW * 4 <= 32 * 1024 &&
           (long)p.planes * p.nbands / (NPL * 2) >= 600) NPL *= 2;
    if (const int f = knob(K_DWL_NPL); f > 0) NPL = f;                      // tuning only
    p.NPL = NPL;
    p.nitems = (((long)p.planes + NPL - 1) / NPL) * p.nbands;
    const long ppl = (long)p.IH * p.LW, owq = (d.ow + 3) / 4, per = (long)BH * owq;
    // exactness of umulhi(i, m): i * d < 2^32 with i < NPL * ppl (staging) resp. NPL * per (outputs)
    if ((long)NPL * ppl * ppl >= (1L << 32) || (long)NPL * per * per >= (1L << 32) || (long)p.planes >= (1L << 31)) {
        ffgpu_set_error("dw_lds: item too large for 32-bit index arithmetic"); return -1; }
    p.m_ppl = umulhi_magic(ppl); p.m_lw = umulhi_magic(p.LW); p.m_per = umulhi_magic(per); p.m_owq = umulhi_magic(owq);
    p.vec4 = d.ow % 4 == 0 && ((long)d.ow * d.oh) % 4 == 0;
    const size_t lds = ((size_t)NPL * p.IH * p.LW + NPL * (d.fs * d.fs + 2) + 8) * sizeof(float);
    const int grid = (int)(p.nitems < 256L * 16 ? p.nitems : 256L * 16);
    if (d.fs == 3 && d.stride == 1)      hipLaunchKernelGGL((k_dw_lds<3, 1>), dim3(grid), dim3(256), lds, s, p);
    else if (d.fs == 3)                  hipLaunchKernelGGL((k_dw_lds<3, 2>), dim3(grid), dim3(256), lds, s, p);
    else if (d.stride == 1)              hipLaunchKernelGGL((k_dw_lds<5, 1>), dim3(grid), dim3(256), lds, s, p);
    else                                 hipLaunchKernelGGL((k_dw_lds<5, 2>), dim3(grid), dim3(256), lds, s, p);
    LAUNCH_OK("dw_lds");
    return 0;
}

static int launch_dense_small(const ConvDesc &d, const float *, hipStream_t s)
{
    // the usual first layer (3x3 s2 p1, 3 input channels, even geometry, 16-byte aligned planes, leaky / relu / linear):
    // four pixels per thread -- fewer issue slots, chosen when the batch is big enough for issue slots to be what counts
    if (d.fs == 3 && (d.stride == 2 || d.stride == 1) && d.pad == 1 && d.ic == 3 && !d.residual && d.act != 3 && d.iw == d.stride * d.ow && d.ih == d.stride * d.oh &&
        d.ow % 4 == 0 && d.in_cs % 4 == 0 && d.in_ns % 4 == 0 && d.out_cs % 4 == 0 && d.out_ns % 4 == 0 && d.in_ns < (1L << 30) &&
        d.out_ns * d.N < (1L << 30) && (long)d.N * d.oh * d.ow >= knob(K_CONV_FIRST_MIN_PX) && !knob(K_NO_CONV_FIRST)) {
        const int owq = d.ow / 4, per = d.oh * owq;
        const unsigned m = umulhi_magic(owq);
        const dim3 grid((per + 255) / 256, d.N, (d.oc + 7) / 8);
        if (d.stride == 2) hipLaunchKernelGGL((k_conv_first<3, 2>), grid, dim3(256), (size_t)(27 * 8 + 16) * sizeof(float), s, d, m);
        else               hipLaunchKernelGGL((k_conv_first<3, 1>), grid, dim3(256), (size_t)(27 * 8 + 16) * sizeof(float), s, d, m);
        LAUNCH_OK("conv_first");
        return 0;
    }
    const long npx = (long)d.N * d.oh * d.ow;
    const int ppt = npx >= 262144 ? 2 : 1;
    const dim3 grid(grid_for((npx + ppt - 1) / ppt, 256, 256 * 16), (d.oc + 7) / 8);
    const size_t lds = ((size_t)d.fs * d.fs * d.ic * 8 + 16) * sizeof(float);
    if (d.fs == 3 && ppt == 2)      hipLaunchKernelGGL((k_conv_dense8<3, 2>), grid, dim3(256), lds, s, d);
    else if (d.fs == 3)             hipLaunchKernelGGL((k_conv_dense8<3, 1>), grid, dim3(256), lds, s, d);
    else if (ppt == 2)              hipLaunchKernelGGL((k_conv_dense8<5, 2>), grid, dim3(256), lds, s, d);
    else                            hipLaunchKernelGGL((k_conv_dense8<5, 1>), grid, dim3(256), lds, s, d);
    LAUNCH_OK("conv_dense8");
    return 0;
}

// ---------------------------------------------------------------------------
// THE table of convolution kernels: everything the dispatcher knows about an FFGPU_K_* id.  Adding a kernel is one entry here plus its place in
// conv_pick's AUTO order.
struct ConvKernel {
    int         id;
    const char *(*name)(const ConvDesc &);
    bool        (*ok)(const ConvDesc &);                       // can run this shape
    size_t      (*image_dwords)(const ConvDesc &);              // packed weight image; nullptr: reads the filter rows as they are
    int         (*pack)(const ConvDesc &, float *, hipStream_t);
    int         (*launch)(const ConvDesc &, const float *image, hipStream_t);
    bool        reads_ind;                                      // honours ConvDesc::in_ind
    bool        image_optional;                                 // without a plan-time image it runs from the filter rows: bare calls pack nothing
};
static bool any_shape_ok(const ConvDesc &) { return true; }
static const char *name_generic(const ConvDesc &)     { return "conv_generic"; }
static const char *name_dw_stream(const ConvDesc &)   { return "dw3_stream"; }
static const char *name_dw_lds(const ConvDesc &)      { return "dw_lds"; }
static const char *name_pw_mfma(const ConvDesc &)     { return "pw_mfma"; }
static const char *name_pw_gemm(const ConvDesc &)     { return "pw_gemm"; }
static const char *name_dense_small(const ConvDesc &) { return "conv_dense8"; }
static const char *name_igemm(const ConvDesc &)       { return "conv_igemm"; }
static const char *name_pw_bf16(const ConvDesc &)     { return "pw_bf16"; }
static const char *name_group_thin(const ConvDesc &)  { return "conv_thin"; }
static const char *name_pw_x3(const ConvDesc &)       { return "pw_x3"; }
static const char *name_conv_x3(const ConvDesc &d)    { return d.fs == 1 ? "pw_x3s" : "conv_x3"; }
static const char *name_pw_x3t(const ConvDesc &)      { return "pw_x3t"; }

static const ConvKernel conv_kernels[] = {
    //  id                   name              ok              image_dwords        pack          launch              reads_ind  image_optional
    { FFGPU_K_GENERIC,     name_generic,     any_shape_ok,   nullptr,            nullptr,      launch_generic,     true,  false },
    { FFGPU_K_DW_STREAM,   name_dw_stream,   dw_stream_ok,   nullptr,            nullptr,      launch_dw_stream,   false, false },
    { FFGPU_K_DW_LDS,      name_dw_lds,      dw_lds_ok,      nullptr,            nullptr,      launch_dw_lds,      false, false },      // (pair-able 5x5 shapes: k_dw_pair)
    { FFGPU_K_PW_MFMA,     name_pw_mfma,     pw_mfma_ok,     pw_mfma_img_dwords, pw_mfma_pack, launch_pw_mfma,     false, true  },
    { FFGPU_K_PW_GEMM,     name_pw_gemm,     pw_gemm_ok,     pwg32_img_dwords,   pwg32_pack,   launch_pw_gemm,     false, false },
    { FFGPU_K_DENSE_SMALL, name_dense_small, dense_small_ok, nullptr,            nullptr,      launch_dense_small, true,  false },      // (the usual first layer: k_conv_first)
    { FFGPU_K_IGEMM,       name_igemm,       igemm_ok,       igemm_img_dwords,   igemm_pack,   launch_igemm,       true,  false },      // (image: the groups' images, then the split-K partial sums)
    { FFGPU_K_PW_BF16,     name_pw_bf16,     pw_gemm_ok,     pwbf16_img_dwords,  pwbf16_pack,  launch_pw_bf16,     false, false },
    { FFGPU_K_GROUP_THIN,  name_group_thin,  group_thin_ok,  nullptr,            nullptr,      launch_group_thin,  true,  false },
    { FFGPU_K_PW_X3,       name_pw_x3,       pw_x3_ok,       pwx3_img_dwords,    pwx3_pack,    launch_pw_x3,       false, false },
    { FFGPU_K_CONV_X3,     name_conv_x3,     ig_x3_ok,       ig_x3_img_dwords,   ig_x3_pack,   launch_conv_x3,     false, false },
    { FFGPU_K_PW_X3T,      name_pw_x3t,      pw_x3t_ok,      pwx3t_img_dwords,   pwx3t_pack,   launch_pw_x3t,      false, false },
};
static const ConvKernel *conv_kernel(int id)
{
    for (const ConvKernel &k : conv_kernels) if (k.id == id) return &k;
    return nullptr;
}

// THE rule for the image a launch of kernel k reads.  ConvDesc::wpack is the plan-time image, sized (ffgpu_pw_pack_floats) and filled (ffgpu_pw_pack) for
// the kernel AUTO picks -- so it serves k only if k IS that kernel.  Every other launch (bare single-layer calls; an explicit variant next to somebody
// else's image) packs into the calling thread's scratch on the launch's stream first.  One scratch per kernel id: two bare calls of different
// kernels on one stream must not overwrite each other's image before the first has run.
static int conv_image(const ConvDesc &d, const ConvKernel &k, hipStream_t s, const float **image)
{
    static thread_local BareScratch bare_scratch[FFGPU_K_PW_X3T + 1];
    *image = nullptr;
    if (!k.image_dwords) return 0;
    if (d.wpack && conv_pick(d, FFGPU_K_AUTO) == k.id) { *image = d.wpack; return 0; }
    if (k.image_optional) return 0;
    float *sc = bare_scratch[k.id].get(k.image_dwords(d));
    if (!sc) { ffgpu_set_error("%s: hipMalloc failed", k.name(d)); return -1; }
    if (k.pack(d, sc, s)) return -1;
    *image = sc;
    return 0;
}

bool ffgpu_conv_supports_ind(const ConvDesc &d)
{
    const ConvKernel *k = conv_kernel(conv_pick(d, FFGPU_K_AUTO));
    return k && k->reads_ind;
}

const char *ffgpu_conv_kernel_name(const ConvDesc &d, int variant)
{
    const ConvKernel *k = conv_kernel(conv_pick(d, variant));
    return k && k->ok(d) ? k->name(d) : "unsupported";
}

// plan-time weight image of the kernel AUTO picks, in floats rounded up to 64; 0: that kernel reads the filter rows as they are
size_t ffgpu_pw_pack_floats(const ConvDesc &d)
{
    const ConvKernel *k = conv_kernel(conv_pick(d, FFGPU_K_AUTO));
    return k && k->image_dwords ? (k->image_dwords(d) + 63) & ~(size_t)63 : 0;
}

int ffgpu_pw_pack(const ConvDesc &d, float *pk, hipStream_t s)
{
    const ConvKernel *k = conv_kernel(conv_pick(d, FFGPU_K_AUTO));
    return k && k->pack ? k->pack(d, pk, s) : 0;
}

int ffgpu_launch_conv(const ConvDesc &d, int variant, hipStream_t s)
{
    if (d.groups < 1 || d.ic % d.groups || d.oc % d.groups || d.fs < 1 || d.stride < 1) {
        ffgpu_set_error("groupconv: bad geometry (ic=%d oc=%d groups=%d fs=%d stride=%d)", d.ic, d.oc, d.groups, d.fs, d.stride);
        return -1;
    }
    const int id = conv_pick(d, variant);
    const ConvKernel *k = conv_kernel(id);
    if (!k || !k->ok(d)) {
        ffgpu_set_error("groupconv: kernel variant %d does not support this shape", id);
        return -1;
    }
    const float *image;
    if (conv_image(d, *k, s, &image)) return -1;
    return k->launch(d, image, s);
}

// ---------------------------------------------------------------------------
// depthwise K x K + pointwise 1 x 1 in one kernel (ffgpu_dwpw.inc): geometry, constant packing, launch
static bool dwpw_geometry(const ConvDesc &dw, const ConvDesc &pw, DwPwP &p, size_t &lds)
{
    const int fs = dw.fs, W = dw.iw, H = dw.ih;
    // cheapest tiling: TW x TH <= 128 pixels, halo tile <= 256 positions, fewest halo positions over the plane
    long best = -1;
    for (int tw = 4; tw <= std::min(W, 32); tw++)
        for (int th = 1; th <= std::min(H, 32); th++) {
            if (tw * th > 128 || (tw + fs - 1) * (th + fs - 1) > 256) continue;
            const long ntx = (W + tw - 1) / tw, nty = (H + th - 1) / th;
            const long cost = ntx * nty * ((tw + fs - 1) * (th + fs - 1) + 64);       // + a constant per tile (tables, epilogue)
            const long padded = ntx * nty * (((tw * th + 15) / 16) * 16);             // MFMA columns incl. padding
            const long score = cost + padded;
            if (best < 0 || score < best) { best = score; p.TW = tw; p.TH = th; }
        }
    if (best < 0) return false;
    p.N = dw.N; p.W = W; p.H = H; p.C = dw.ic; p.OC = pw.oc;
    p.TP = p.TW * p.TH; p.NCT = (p.TP + 15) / 16; p.TPS = p.NCT * 16 + 4;
    p.ntx = (W + p.TW - 1) / p.TW; p.nty = (H + p.TH - 1) / p.TH;
    p.HW_ = p.TW + fs - 1; p.HH_ = p.TH + fs - 1;
    p.NRT = (p.OC + 15) / 16; p.nchunks = (p.C + 7) / 8;
    // x segments: as many items as 256 threads take, segments of at most 8 pixels
    int xs = std::max(1, 256 / (8 * p.TH));
    xs = std::min(xs, p.TW);
    int seg = (p.TW + xs - 1) / xs;
    if (seg > 8) { seg = 8; xs = (p.TW + 7) / 8; }
    xs = (p.TW + seg - 1) / seg;
    if (8 * p.TH * xs > 256) return false;
    p.XS = xs; p.SEG = seg;
    p.rld = conv_k4(dw) + 4;
    const int aimg = 2 * p.nchunks * p.NRT * 64 + p.NRT * 32, tapw = fs * fs + 3;
    lds = (size_t)(((aimg + 3) & ~3) + ((p.nchunks * 8 * tapw + 3) & ~3) + ((8 * p.HW_ * p.HH_ + 3) & ~3) + 2 * 8 * p.TPS) * sizeof(float);
    return p.NRT <= 8 && p.NCT <= 8 && lds <= 150 * 1024;
}

bool ffgpu_dwpw_ok(const ConvDesc &dw, const ConvDesc &pw)
{
    DwPwP p; size_t lds;
    return conv_is_depthwise(dw) && (dw.fs == 3 || dw.fs == 5) && dw.stride == 1 && dw.pad == dw.fs / 2 && conv_cnhw_contiguous(dw) && !dw.residual &&
           dw.act != 3 && !(dw.flags & FFGPU_COMPAT_V6) && conv_is_pointwise(pw) && conv_cnhw_contiguous(pw) && !pw.residual && pw.act != 3 &&
           pw.ic == dw.oc && pw.iw == dw.ow && pw.ih == dw.oh && pw.N == dw.N &&
           (long)dw.N * dw.iw * dw.ih * std::max(dw.ic, pw.oc) < (1L << 31) && dwpw_geometry(dw, pw, p, lds);
}

size_t ffgpu_dwpw_pack_floats(const ConvDesc &dw, const ConvDesc &pw)
{
    const int nrt = (pw.oc + 15) / 16, nchunks = (dw.ic + 7) / 8;
    return ((size_t)(2 * nchunks * nrt * 64 + nrt * 32) + 63) & ~(size_t)63;
}

int ffgpu_dwpw_pack(const ConvDesc &dw, const ConvDesc &pw, float *pk, hipStream_t s)
{
    DwPwPackP q;
    q.filt = pw.filt; q.pk = pk; q.C = dw.ic; q.OC = pw.oc; q.NRT = (pw.oc + 15) / 16; q.nchunks = (dw.ic + 7) / 8;
    const int total = 2 * q.nchunks * q.NRT * 64 + q.NRT * 32;
    hipLaunchKernelGGL(k_dwpw_pack, dim3((total + 255) / 256), dim3(256), 0, s, q);
    LAUNCH_OK("dwpw_pack");
    return 0;
}

template <int FS, int SG>
static int dwpw_launch_t(const DwPwP &p, size_t lds, unsigned grid, hipStream_t s)
{
    if (lds_allow((const void *)k_dwpw<FS, SG>, lds, "dwpw")) return -1;
    hipLaunchKernelGGL((k_dwpw<FS, SG>), dim3(grid), dim3(256), lds, s, p);
    LAUNCH_OK("dwpw");
    return 0;
}

int ffgpu_launch_dwpw(const ConvDesc &dw, const ConvDesc &pw, const float *wpack, hipStream_t s)
{
    DwPwP p; size_t lds;
    if (!ffgpu_dwpw_ok(dw, pw) || !dwpw_geometry(dw, pw, p, lds)) { ffgpu_set_error("dwpw: unsupported layer pair"); return -1; }
    p.in = dw.in; p.out = pw.out; p.wd = dw.filt; p.wpack = wpack;
    p.slope_d = dw.act == 2 ? 0.1f : (dw.act == 1 ? 0.f : 1.f); p.slope_p = pw.act == 2 ? 0.1f : (pw.act == 1 ? 0.f : 1.f);
    const unsigned grid = (unsigned)(p.N * p.ntx * p.nty);
    if (dw.fs == 5) return p.SEG <= 4 ? dwpw_launch_t<5, 4>(p, lds, grid, s) : dwpw_launch_t<5, 8>(p, lds, grid, s);
    return p.SEG <= 4 ? dwpw_launch_t<3, 4>(p, lds, grid, s) : dwpw_launch_t<3, 8>(p, lds, grid, s);
}

// ---------------------------------------------------------------------------
// fused inverted-residual block: one plan per block, constant packing, launch.
// ffgpu_irb_plan picks the family -- thin (k_irb_thin), wave (k_irbw / k_irbw2) or workgroup (k_irb) --, the instantiation, the tile, the layout of the
// packed image and the launch shape, and writes them into IrbDesc::plan.  It is the only function of this section that reads a choice or layout switch
// of the FFGPU_* environment: ffgpu_irb_pack_floats, ffgpu_irb_pack, ffgpu_launch_irb and the front kernel follow the plan, so a switch changed after
// planning cannot pair one kernel with another kernel's image.  (Read at launch: the diagnostics FFGPU_IRB_TRACE, FFGPU_VERBOSE_IRB, FFGPU_IRB_SKIP, and
// -- a thin block has no image -- FFGPU_THIN_PAIR with the paired form's FFGPU_THIN_BAND: thin_form.)
static float act_slope(int act) { return act == 2 ? 0.1f : (act == 1 ? 0.f : 1.f); }

// tuning only (make TRACE=1 / -DIRB_TRACE=1, FFGPU_IRB_TRACE=1): in-kernel timeline of wave 0 of each workgroup of one k_irbw / k_irb launch, printed per
// launch.  Of a workgroup's 16 slots, 0 .. nd are consecutive timestamps (100 MHz; a zero one: the phase did not run) and 8 .. 8 + ns - 1 sums over phases.
struct IrbTraceFmt { const char *what; int nd, ns; const char *dname[7], *sname[6]; };
static const IrbTraceFmt irbw_trace = { "irbw", 5, 6, { "issue loads", "barrier", "groups", "reduce", "rows" }, { "expand mfma", "store", "dw0", "prj0", "dw1", "prj1" } };
static const IrbTraceFmt irb_trace = { "irb", 7, 4, { "consts", "wait", "load", "chunks", "reduce", "epilogue", "other-tiles" }, { "bar1", "expand", "bar2", "dw+project" } };
static const IrbTraceFmt &irb_trace_of(const IrbwP &) { return irbw_trace; }
static const IrbTraceFmt &irb_trace_of(const IrbP &) { return irb_trace; }

static unsigned long long *irb_trace_begin(hipStream_t s)
{
    static unsigned long long *d_t = nullptr;
    if (!d_t && hipMalloc(&d_t, 4096 * 16 * sizeof(unsigned long long)) != hipSuccess) return d_t = nullptr;
    (void)hipMemsetAsync(d_t, 0, 4096 * 16 * sizeof(unsigned long long), s);
    return d_t;
}

template <typename P>
static int irb_trace_end(const P &p, const unsigned long long *d_t, long nblocks, hipStream_t s)
{
    const IrbTraceFmt &f = irb_trace_of(p);
    (void)hipStreamSynchronize(s);
    const long nb = std::min(nblocks, 4096L);
    std::vector<unsigned long long> h((size_t)nb * 16);
    (void)hipMemcpy(h.data(), d_t, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    unsigned long long t0 = ~0ull, t1 = 0; double d[7] = { 0 }, sum[6] = { 0 }, late = 0;
    for (long b = 0; b < nb; b++) t0 = std::min(t0, h[b * 16]);
    for (long b = 0; b < nb; b++) {
        unsigned long long prev = h[b * 16];
        late = std::max(late, (double)(prev - t0) * 0.01);
        for (int k = 0; k < f.nd; k++) { const unsigned long long t = h[b * 16 + k + 1] ? h[b * 16 + k + 1] : prev; d[k] += (double)(t - prev) / nb * 0.01; prev = t; }
        t1 = std::max(t1, prev);
        for (int k = 0; k < f.ns; k++) sum[k] += (double)h[b * 16 + 8 + k] / nb * 0.01;
    }
    fprintf(stderr, "  trace %s %dx%d %d->%d->%d: span %.2f us (first %ld blocks), last start +%.2f |", f.what, p.W, p.H, p.ic, p.ec, p.oc, (double)(t1 - t0) * 0.01, nb, late);
    for (int k = 0; k < f.nd; k++) fprintf(stderr, " %s %.2f", f.dname[k], d[k]);
    fprintf(stderr, " [");
    for (int k = 0; k < f.ns; k++) fprintf(stderr, "%s%s %.2f", k ? " " : "", f.sname[k], sum[k]);
    fprintf(stderr, "] (us, wave 0, mean per workgroup)\n");
    return 0;
}

// every k_irbw / k_irbw2 / k_irb launch: the planned LDS allowed, the planned grid and block, the trace if asked for
template <typename P, void (*K)(P)>
static int irb_launch_t(const P &p, const IrbPlan &c, hipStream_t s)
{
    const char *const what = irb_trace_of(p).what;
    if (lds_allow((const void *)K, (size_t)c.lds, what)) return -1;
    if (knob(K_IRB_TRACE)) {
        P q = p;
        if (!(q.dbg_t = irb_trace_begin(s))) return -1;
        hipLaunchKernelGGL(K, dim3((unsigned)c.grid), dim3(c.block), (size_t)c.lds, s, q);
        return irb_trace_end(p, q.dbg_t, c.grid, s);
    }
    hipLaunchKernelGGL(K, dim3((unsigned)c.grid), dim3(c.block), (size_t)c.lds, s, p);
    LAUNCH_OK(what);
    return 0;
}

#define IRB_LDS_MAX (160 * 1024)                     // per workgroup on gfx950

// ---- thin form (ffgpu_irb_thin.inc): 8 expanded channels, streaming; the kernel reads the filter rows directly
static bool irb_thin_ok(const IrbDesc &d)
{
    return d.stride == 1 && d.ec == 8 && (d.ic == 4 || d.ic == 8) && (d.oc == 4 || d.oc == 8) && d.W % 4 == 0 && d.W / 4 <= 64 &&
           8L * d.N * d.W * d.H < (1L << 30) &&          // 32-bit offsets inside a frame-major tensor
           d.act1 != 3 && d.actd != 3 && d.act2 != 3 && d.res_act != 3 && !knob(K_NO_THIN);
}

// rows per wave of k_irb_thin and k_front: every band expands two extra rows, so long bands waste least -- but the launch wants ~1000 waves;
// 16 rows at batch 64 (640 waves, 12 % extra expand work), 2 rows for a single frame (80 waves)
static int thin_band(int N, int H)
{
    int band = 2;
    while (band < 16 && (long)N * H >= 640L * band * 2) band *= 2;
    return band;
}

static ThinP thin_params(const IrbDesc &d)
{
    ThinP p;
    p.in = d.in; p.out = d.out; p.residual = d.residual; p.w1 = d.w1; p.wd = d.wd; p.w2 = d.w2;
    p.W = d.W; p.H = d.H; p.N = d.N;
    p.band = d.plan.band; p.nbands = (d.H + p.band - 1) / p.band;
    p.act1 = act_slope(d.act1); p.actd = act_slope(d.actd); p.act2 = act_slope(d.act2); p.res_act = act_slope(d.res_act);
    p.ntasks = (long)d.N * p.nbands;
    return p;
}

template <int IC, int EC, int OC>
static int irb_thin_launch(const ThinP &p, const IrbPlan &c, hipStream_t s)
{
    hipLaunchKernelGGL((k_irb_thin<IC, EC, OC>), dim3((unsigned)c.grid), dim3(c.block), 0, s, p);
    LAUNCH_OK("irb_thin");
    return 0;
}

// The paired form (k_irb_thin_pair: two frames per wave) is the LAUNCH's choice, not the plan's: the planned line stays what it is, and a thin
// block has no packed image that a later change of FFGPU_THIN_PAIR could mismatch.  Columns per lane: the fewest of 3, 4, 5 that divide the row
// and put it into 32 lanes (160 pixels: 5); none: the single form.
// (Five columns of 8 input channels do not fit the register file -- <8,8,4,5> and <8,8,8,5> spill even with the residual row read late --
// so those two are not built: such a block keeps the single form.)
static constexpr bool thin_pair_built(int ic, int ncp) { return !(ic == 8 && ncp == 5); }
static int thin_pair_ncp(int W, int ic)
{
    for (int nc = 3; nc <= 5; nc++)
        if (W % nc == 0 && W / nc <= 32) return thin_pair_built(ic, nc) ? nc : 0;
    return 0;
}

// What launch_irb_thin launches for a planned thin block, pure host arithmetic (ffgpu_irb_thin_launch_line; tests/test_thin_pair_host.py enumerates it).
// The paired form where a column count exists, the batch has a pair, the executor runs several chains (FFGPU_CONCURRENT: alone the single form's
// twice as many waves fill the chip better) and FFGPU_THIN_PAIR is not 0.  Pairing halves the waves, so its band is thin_band's for ceil(N / 2)
// pairs -- 8 rows at batch 64, the same 640 waves -- unless FFGPU_THIN_BAND says otherwise; the single form keeps the plan's band and grid.
struct ThinForm { int ncp, band, nbands; long ntasks; int grid; };    // ncp 0: k_irb_thin
static ThinForm thin_form(const IrbDesc &d)
{
    ThinForm f;
    const int ncp = thin_pair_ncp(d.W, d.ic);
    const bool pair = ncp && d.N >= 2 && (d.flags & FFGPU_CONCURRENT) && knob(K_THIN_PAIR) != 0;
    const int units = pair ? (d.N + 1) / 2 : d.N;
    f.ncp = pair ? ncp : 0;
    f.band = pair ? knob_or(K_THIN_BAND, thin_band(units, d.H)) : d.plan.band;
    f.nbands = (d.H + f.band - 1) / f.band;
    f.ntasks = (long)units * f.nbands;
    f.grid = pair ? (int)((f.ntasks + 3) / 4) : d.plan.grid;
    return f;
}

template <int IC, int EC, int OC>
static int irb_thin_pair_launch(const ThinP &p, const ThinForm &f, hipStream_t s)
{
    if (f.ncp == 3) hipLaunchKernelGGL((k_irb_thin_pair<IC, EC, OC, 3>), dim3((unsigned)f.grid), dim3(256), 0, s, p);
    else if (f.ncp == 4) hipLaunchKernelGGL((k_irb_thin_pair<IC, EC, OC, 4>), dim3((unsigned)f.grid), dim3(256), 0, s, p);
    else if constexpr (thin_pair_built(IC, 5)) hipLaunchKernelGGL((k_irb_thin_pair<IC, EC, OC, 5>), dim3((unsigned)f.grid), dim3(256), 0, s, p);
    else { ffgpu_set_error("irb_thin_pair: no instantiation for %d columns per lane of %d channels", f.ncp, IC); return -1; }
    LAUNCH_OK("irb_thin_pair");
    return 0;
}

typedef int (*IrbThinLaunch)(const ThinP &, const IrbPlan &, hipStream_t);
typedef int (*IrbThinPairLaunch)(const ThinP &, const ThinForm &, hipStream_t);
struct IrbThinKernel { int IC, OC; IrbThinLaunch launch; IrbThinPairLaunch pair; };
static const IrbThinKernel irb_thin_kernels[] = { { 8, 4, irb_thin_launch<8, 8, 4>, irb_thin_pair_launch<8, 8, 4> }, { 4, 4, irb_thin_launch<4, 8, 4>, irb_thin_pair_launch<4, 8, 4> },
                                                  { 8, 8, irb_thin_launch<8, 8, 8>, irb_thin_pair_launch<8, 8, 8> }, { 4, 8, irb_thin_launch<4, 8, 8>, irb_thin_pair_launch<4, 8, 8> } };

static int launch_irb_thin(const IrbDesc &d, hipStream_t s)
{
    ThinP p = thin_params(d);
    const ThinForm f = thin_form(d);
    if (f.ncp) { p.band = f.band; p.nbands = f.nbands; p.ntasks = f.ntasks; }
    for (const IrbThinKernel &k : irb_thin_kernels)
        if (k.IC == d.ic && k.OC == d.oc) return f.ncp ? k.pair(p, f, s) : k.launch(p, d.plan, s);
    ffgpu_set_error("irb_thin: no instantiation for %d -> 8 -> %d channels", d.ic, d.oc);
    return -1;
}

// one line per launch of a planned thin block: the form (thin<IC,8,OC> or thin_pair<IC,8,OC,NC>) and the launch's own shape
int ffgpu_irb_thin_launch_line(const IrbDesc &d, char *buf, size_t cap)
{
    if (d.plan.family != IRB_THIN) return snprintf(buf, cap, "unsupported");
    const ThinForm f = thin_form(d);
    char key[48];
    if (f.ncp) snprintf(key, sizeof key, "thin_pair<%d,8,%d,%d>", d.ic, d.oc, f.ncp);
    else snprintf(key, sizeof key, "thin<%d,8,%d>", d.ic, d.oc);
    return snprintf(buf, cap, "%s W=%d H=%d N=%d band=%d nbands=%d ntasks=%ld grid=%d block=256", key, d.W, d.H, d.N, f.band, f.nbands, f.ntasks, f.grid);
}

// ---- streaming stride-2 form (ffgpu_irb_thin_s2.inc): the 4 -> 24 -> 8 block of a 160-pixel plane on the vector ALU.  Like the paired thin form it is the
// LAUNCH's choice, not the plan's: the block stays planned as the wave form (plan line, packed image and instantiation list are what they were), and the
// streaming kernel reads the filter rows, not the image, so a later change of FFGPU_THIN_S2 cannot mismatch anything.
// Taken where the block is stride 2 with (ic, ec, oc) = (4, 24, 8) on an even-width plane, a row of the output fits 32 lanes at NC = 3 columns per lane
// (and has three columns), the batch has at least two frames, the block has no residual, the executor runs several chains (FFGPU_CONCURRENT), the activations are the thin family's and
// FFGPU_THIN_S2 is not 0.  (NC = 4 -- 20 lanes, three frames -- needs 90 registers more than the file has and is not built.)
// Band: output rows per wave; the longest of 2, 4, 8, 16 that leaves the launch THIN_S2_WAVES waves (4 rows at batch 64, 640 waves: 213.9 k frames/s against 212.3 k at 8 rows and 202.5 k
// at 16, profiles/thin_s2_ab.txt), unless FFGPU_THIN_S2_BAND names one.  The rule is fitted to that one batch: smaller batches get 2 rows by it (a halo row per four expanded rows
// instead of one per eight), and neither 2 rows nor any other batch has been measured.
#define THIN_S2_NC 3
#define THIN_S2_WAVES 640
struct ThinS2Form { bool on; int lpr, F, band, nbands; long ntasks; int grid; };
static ThinS2Form thin_s2_form(const IrbDesc &d)
{
    ThinS2Form f{};
    const int lpr = (d.OW + THIN_S2_NC - 1) / THIN_S2_NC;
    f.on = d.stride == 2 && d.ic == 4 && d.ec == 24 && d.oc == 8 && d.W % 2 == 0 && d.OW == d.W / 2 && d.OH == (d.H + 1) / 2 && d.OW >= THIN_S2_NC && lpr <= 32 &&
           d.N >= 2 && (d.flags & FFGPU_CONCURRENT) && !d.residual &&
           (size_t)d.ic * d.N * d.H * d.W < (1u << 30) &&                    // 32-bit offsets (the wave plan's own condition)
           d.act1 != 3 && d.actd != 3 && d.act2 != 3 && knob(K_THIN_S2) != 0;
    if (!f.on) return f;
    f.lpr = lpr; f.F = 64 / lpr;
    const int groups = (d.N + f.F - 1) / f.F;
    int band = 2;
    while (band < 16 && (long)groups * d.OH >= (long)THIN_S2_WAVES * band * 2) band *= 2;
    if (const int kb = knob(K_THIN_S2_BAND); kb > 0) band = kb;
    f.band = band;
    f.nbands = (d.OH + f.band - 1) / f.band;
    f.ntasks = (long)groups * f.nbands;
    f.grid = (int)((f.ntasks + 3) / 4);
    return f;
}

static int launch_irb_thin_s2(const IrbDesc &d, const ThinS2Form &f, hipStream_t s)
{
    ThinS2P p;
    p.in = d.in; p.out = d.out; p.w1 = d.w1; p.wd = d.wd; p.w2 = d.w2;
    p.W = d.W; p.H = d.H; p.N = d.N; p.OW = d.OW; p.OH = d.OH;
    p.lpr = f.lpr; p.F = f.F; p.band = f.band; p.nbands = f.nbands;
    p.act1 = act_slope(d.act1); p.actd = act_slope(d.actd); p.act2 = act_slope(d.act2);
    p.ntasks = f.ntasks;
    if (!p.in || !p.out || !p.w1 || !p.wd || !p.w2) { ffgpu_set_error("irb_thin_s2: no tensors or filter rows"); return -1; }
    hipLaunchKernelGGL((k_irb_thin_s2<4, 24, 8, THIN_S2_NC>), dim3((unsigned)f.grid), dim3(256), 0, s, p);
    LAUNCH_OK("irb_thin_s2");
    return 0;
}

// ---- wave-autonomous form (ffgpu_irb_wave.inc, ffgpu_irb_wave2.inc): every instantiation that exists, shape test, tile / split choice, launch shape
typedef int (*IrbwLaunch)(const IrbwP &, const IrbPlan &, hipStream_t);
// S: stride; NSI: input strips per wave; NSO: output strips per wave (2: k_irbw2); big: the 256-register budget; x3: expand GEMM as split-bf16 products;
// xl: the split tile once per workgroup in LDS; gate: the switch that lets the planner consider the shape at all (K_NONE: always)
struct IrbwKernel { int KS1, OT, S, NSI, NSO; bool big, x3, xl; Knob gate; IrbwLaunch launch; };
// (entries in the order the instantiations have always been named in, which is the order the compiler emits them in: listings of two builds compare line by line)
#define IRBW_K(ks1, ot, st, nsi, gate) \
    { ks1, ot, st, nsi, 1, true, false, false, gate, irb_launch_t<IrbwP, k_irbw<ks1, ot, st, nsi, true>> }, \
    { ks1, ot, st, nsi, 1, false, false, false, gate, irb_launch_t<IrbwP, k_irbw<ks1, ot, st, nsi, false>> }
static const IrbwKernel irbw_kernels[] = {
    { 2, 1, 1, 3, 2, true, true, false, K_NONE, irb_launch_t<IrbwP, k_irbw2<2, 3, true>> }, { 4, 1, 1, 3, 2, true, true, false, K_NONE, irb_launch_t<IrbwP, k_irbw2<4, 3, true>> },
    { 2, 1, 1, 3, 2, true, false, false, K_NONE, irb_launch_t<IrbwP, k_irbw2<2, 3, false>> }, { 4, 1, 1, 3, 2, true, false, false, K_NONE, irb_launch_t<IrbwP, k_irbw2<4, 3, false>> },
    { 12, 3, 1, 2, 1, true, true, true, K_NONE, irb_launch_t<IrbwP, k_irbw<12, 3, 1, 2, true, true, true>> },
    { 4, 2, 2, 4, 1, true, true, false, K_NONE, irb_launch_t<IrbwP, k_irbw<4, 2, 2, 4, true, true>> },
    { 6, 2, 1, 2, 1, true, true, false, K_NONE, irb_launch_t<IrbwP, k_irbw<6, 2, 1, 2, true, true>> },
    IRBW_K(1, 1, 1, 2, K_NONE), IRBW_K(2, 1, 1, 2, K_NONE), IRBW_K(4, 1, 1, 2, K_NONE), IRBW_K(2, 2, 1, 2, K_NONE), IRBW_K(4, 2, 1, 2, K_NONE),
    IRBW_K(6, 2, 1, 2, K_NONE), IRBW_K(12, 3, 1, 2, K_NONE), IRBW_K(1, 1, 2, 3, K_NONE), IRBW_K(2, 1, 2, 3, K_NONE), IRBW_K(4, 2, 2, 4, K_NONE),
    IRBW_K(6, 3, 2, 3, K_IRBW_S2_633),
    IRBW_K(1, 1, 2, 4, K_IRBW_S2_NSI4), IRBW_K(2, 1, 2, 4, K_IRBW_S2_NSI4),     // four-strip halo for the thin stride-2 blocks (12 of 16 output quads instead of 8)
};
#undef IRBW_K
static const int irbw_nkernels = (int)(sizeof irbw_kernels / sizeof irbw_kernels[0]);

// a single-strip fp32 instantiation of the shape exists and its switch, if it has one, lets the planner take it
static bool irbw_has_kernel(int KS1, int OT, int S, int NSI)
{
    for (const IrbwKernel &k : irbw_kernels)
        if (k.KS1 == KS1 && k.OT == OT && k.S == S && k.NSI == NSI && k.NSO == 1 && !k.x3) return k.gate == K_NONE || knob(k.gate) != 0;
    return false;
}

static long irbw_ntiles(const IrbDesc &d, int TWq, int TH) { return (long)d.N * ((d.OW + 4 * TWq - 1) / (4 * TWq)) * ((d.OH + TH - 1) / TH); }

static bool irbw_pick(const IrbDesc &d, IrbPlan &c)
{
    if (knob(K_NO_IRBW)) return false;
    if (d.stride != 1 && d.stride != 2) return false;
    if (d.act1 == 3 || d.actd == 3 || d.act2 == 3 || d.res_act == 3) return false;
    if ((size_t)d.ic * d.N * d.H * d.W >= (1u << 30) || (size_t)d.oc * d.N * d.OH * d.OW >= (1u << 30)) return false;   // 32-bit byte offsets
    const int S = d.stride;
    c.KS1 = ((d.ic + 3) & ~3) / 4; c.OT = (d.oc + 15) / 16; c.ngroups = (d.ec + 15) / 16;
    // output tile of TWq quads x TH rows (<= 16 quads) whose halo fits NSI strips: fewest expand strips over the plane
    double best = 1e30;
    for (int TWq = 1; TWq <= 8; TWq++) {
        if (TWq > 1 && (TWq - 1) * 4 >= d.OW) break;
        for (int TH = 1; TWq * TH <= 16 && TH <= d.OH + 1; TH++) {
            const int EW = S == 1 ? 4 * TWq + 4 : 8 * TWq + 4, EH = S * (TH - 1) + 3;
            int NSI = (EW * EH + 63) / 64;
            if (NSI < 2) NSI = 2;
            if (S == 2 && NSI < 3) NSI = 3;
            if (NSI > 4 || !irbw_has_kernel(c.KS1, c.OT, S, NSI)) continue;
            const long tiles = irbw_ntiles(d, TWq, TH) / d.N;
            // cycles per group, roughly; wide halo rows (EW floats contiguous in memory) load and store better than
            // tall narrow tiles with the same strip count (profiles/r01_g_irbw_sweep.txt: 20x3 beats 8x8 on 80x80 and 40x40)
            const double cost = (double)tiles * (NSI * (c.KS1 * 128.0 + 500.0) + 4 * (220.0 + c.OT * 128.0)) * (1.0 + 12.0 / EW);
            if (cost < best) { best = cost; c.TWq = TWq; c.TH = TH; c.EW = EW; c.EH = EH; c.NSI = NSI; }
        }
    }
    if (best > 1e29) return false;
    const int ft = knob(K_IRBW_TWQ), fh = knob(K_IRBW_TH);
    if (ft > 0 && fh > 0 && ft * fh <= 16) {
        const int EW = S == 1 ? 4 * ft + 4 : 8 * ft + 4, EH = S * (fh - 1) + 3;
        if (EW * EH <= c.NSI * 64) { c.TWq = ft; c.TH = fh; c.EW = EW; c.EH = EH; }
    }
    const long ntiles = irbw_ntiles(d, c.TWq, c.TH);
    const int regs = c.NSI * c.KS1 * 4 + c.OT * 16 + 2 * (c.KS1 + 4 * c.OT) + 76;                     // rough VGPR need
    c.big = regs > 124;
    // (the BIG instantiation of a shape whose second set of expand accumulators fits is the software-pipelined form;
    //  it buys a lone wave nothing and costs the many-round launches occupancy, so it is not forced: FFGPU_IRBW_BIG=1)
    if (const int f = knob(K_IRBW_BIG); f >= 0) c.big = f != 0;                 // tuning only
    if (const int f = S == 2 && c.KS1 == 1 ? knob(K_IRBW_BIG_S2K1) : -1; f >= 0) c.big = f != 0;   // tuning only: the 160 -> 80 block alone (40 bytes of scratch at 128 registers)
    // waves sharing a tile: one wave per tile when that already gives every SIMD a wave or more (tools/tune_irbw.py:
    // the split only pays on the small planes), else the smallest split that does
    // With several chains in flight (FFGPU_CONCURRENT) other launches fill the SIMDs, and what counts is the work per
    // wave that a split repeats (input tile, constants, reduction): 4 waves on the 10x10 planes and 2 on the 20x20 ones
    // instead of 8 and 4 -- 3.5 % more frames/s with four chains, 4 % fewer with one.
    const bool conc = (d.flags & FFGPU_CONCURRENT) != 0;
    const int x3_mask = knob(K_IRBW_X3);                            // one bit per shape that has a split-bf16 expand
    const int gmax = std::min(8, c.ngroups);
    int G = 1;
    for (int g = 1; g <= gmax; g++) {
        const size_t slot = (size_t)c.OT * 1024, ereg = (size_t)g * 16 * c.NSI * 64;
        if (g > 1 && ereg / slot < (size_t)(g + 1) / 2) continue;                                      // reduction must fit the E slices
        G = g;
        if (ntiles * g >= knob_or(K_IRBW_GWAVES, conc ? 500 : 1200)) break;
    }
    if (!conc && G > 1 && G < gmax && c.ngroups % G != 0 && (c.ngroups + G) / (G + 1) <= (c.ngroups + G - 1) / G) G++;   // same trips per wave, better balance
    // measured exceptions (profiles/r01_g_irbw_sweep.txt, batch 64): four waves on the 20x20 blocks (3, 2, 2, 2 groups
    // each) beat three by 8 %
    if (d.stride == 1 && c.ngroups == 9 && ntiles >= 400 && ntiles < 512 && gmax >= 4 && !conc && !knob(K_IRBW_NOEXC)) G = 4;
    if (const int f = ntiles >= 256 && ntiles < 1100 ? knob(K_IRBW_G_MID) : 0; f > 0) G = std::min(gmax, f);
    // the LDS-resident split tile (XL, 48 input channels) makes a wave's share of a tile cheaper: with several chains in flight seven waves
    // (two groups each of the 10x10 blocks' fourteen) beat four by 1.3 % (profiles/r04: 193.8 k against 191.3 k frames/s, eight: 193.4 k)
    const bool xl_ok = S == 1 && c.KS1 == 12 && c.OT == 3 && c.NSI == 2 && c.big && ((x3_mask >> 3) & 1) != 0;
    if (xl_ok && conc && ntiles < 256) G = std::min(gmax, knob(K_IRBW_G_XL));
    if (const int f = ntiles < 256 ? knob(K_IRBW_G_SMALL) : 0; f > 0) G = std::min(gmax, f);          // tuning only (wins over the XL choice)
    const int fg = knob(K_IRBW_G);                      // an explicit FFGPU_IRBW_G wins over everything
    if (fg >= 1 && fg <= gmax) G = fg;
    c.G = G;
    c.NSO = 1;
    // single-strip kernel, 24 input channels (the 20x20 blocks): expand GEMM as split-bf16 products (bit 2 of FFGPU_IRBW_X3)
    c.x3 = S == 1 && c.KS1 == 6 && c.OT == 2 && c.NSI == 2 && c.big && ((x3_mask >> 2) & 1) != 0;
    // ... the 40 -> 20 stride-2 block (16 input channels, four-strip halo), bit 4
    if (S == 2 && c.KS1 == 4 && c.OT == 2 && c.NSI == 4 && c.big && ((x3_mask >> 4) & 1) != 0) c.x3 = true;
    // ... and 48 input channels with the groups split over G waves (the 10x10 blocks): the split tile lives once per workgroup in LDS (bit 3)
    c.xl = xl_ok && G > 1;
    if (c.xl) c.x3 = true;
    // two output strips per wave (ffgpu_irb_wave2.inc): one wave per tile, <= 16 output channels, stride 1 -- when a tile
    // of up to 32 quads with a three-strip halo covers the plane with clearly fewer expand strips
    if (G == 1 && S == 1 && c.OT == 1 && (c.KS1 == 2 || c.KS1 == 4) && knob(K_IRBW_NSO) == 2) {
        double best2 = 1e30; int tw2 = 0, th2 = 0;
        for (int TWq = 1; TWq <= 8; TWq++) {
            if (TWq > 1 && (TWq - 1) * 4 >= d.OW) break;
            for (int TH = 1; TWq * TH <= 32 && TH <= d.OH + 1; TH++) {
                if (TWq * TH <= 16 || TWq * ((TH + 1) / 2) > 16) continue;                            // a lane owns a quad in each row of a row pair
                const int EW = 4 * TWq + 4, EH = TH + 2;
                if (EW * EH > 192) continue;                                                           // three strips
                const long tiles = irbw_ntiles(d, TWq, TH) / d.N;
                const double cost = (double)tiles * (3 * (c.KS1 * 128.0 + 500.0) + 2 * 4 * (220.0 + 128.0)) * (1.0 + 12.0 / EW);
                if (cost < best2) { best2 = cost; tw2 = TWq; th2 = TH; }
            }
        }
        const int f2t = knob(K_IRBW2_TWQ), f2h = knob(K_IRBW2_TH);
        if (f2t > 0 && f2h > 0 && f2t * ((f2h + 1) / 2) <= 16 && (4 * f2t + 4) * (f2h + 2) <= 192) { tw2 = f2t; th2 = f2h; best2 = 0; }
        const long nt2 = tw2 ? irbw_ntiles(d, tw2, th2) : 0;
        if (tw2 && best2 < 0.93 * best && nt2 >= knob(K_IRBW2_MIN_TILES)) {
            c.NSO = 2; c.TWq = tw2; c.TH = th2; c.EW = 4 * tw2 + 4; c.EH = th2 + 2; c.NSI = 3; c.big = true; c.WPB = 4; c.xl = false;
            // the expand GEMM as exact split-bf16 products on the bf16 matrix cores (ffgpu_irb_wave.inc "X3"); FFGPU_IRBW_X3=0: fp32 MFMAs
            c.x3 = irbw_x3_has(c.KS1) && ((x3_mask >> (c.KS1 == 2 ? 0 : 1)) & 1) != 0;   // (bit 0: 8 input channels, bit 1: 16)
        }
    }
    // tiles per workgroup (G == 1): whichever of 4 / 8 waves lets more waves share a CU's 160 KB of LDS
    {
        const size_t cs = ((size_t)c.ngroups * 224 + c.OT * 32) * sizeof(float), slice = (size_t)16 * c.NSI * 64 * sizeof(float);
        const int cap = c.big ? 12 : 16;                                                               // VGPR-limited waves per CU
        const int w4 = std::min(cap, (int)(IRB_LDS_MAX / (cs + 4 * slice)) * 4), w8 = std::min(cap, (int)(IRB_LDS_MAX / (cs + 8 * slice)) * 8);
        c.WPB = G > 1 ? G : (w4 >= w8 ? 4 : 8);                                                       // tie: the finer granule (1.3 % with four chains in flight)
        const int fw = knob(K_IRBW_WPB);
        if (G == 1 && fw >= 1 && fw <= 8) c.WPB = fw;
    }
    return true;
}

static void irbw_layout(const IrbPlan &c, int &o_w2, int &o_cs, int &cs_floats, int &total)
{
    o_w2 = c.x3 ? c.ngroups * irbw_x3_nm(c.KS1) * 256 : c.ngroups * c.KS1 * 64;
    o_cs = o_w2 + c.ngroups * 4 * c.OT * 64;
    cs_floats = c.ngroups * 16 * 14 + c.OT * 32;
    total = o_cs + cs_floats;
}

// the parameter block of a planned k_irbw / k_irbw2 launch: arithmetic on the descriptor and the plan
static IrbwP irbw_params(const IrbDesc &d)
{
    const IrbPlan &c = d.plan;
    IrbwP p;
    p.in = d.in; p.out = d.out; p.residual = d.residual; p.pk = d.pk;
    p.N = d.N; p.H = d.H; p.W = d.W; p.OH = d.OH; p.OW = d.OW; p.ic = d.ic; p.ec = d.ec; p.oc = d.oc;
    p.act1 = act_slope(d.act1); p.actd = act_slope(d.actd); p.act2 = act_slope(d.act2); p.res_act = act_slope(d.res_act);
    p.TWq = c.TWq; p.TH = c.TH; p.EW = c.EW; p.EH = c.EH;
    p.tiles_x = (d.OW + 4 * c.TWq - 1) / (4 * c.TWq); p.tiles_y = (d.OH + c.TH - 1) / c.TH;
    p.ntiles = (long)d.N * p.tiles_x * p.tiles_y;
    p.ngroups = c.ngroups; p.G = c.G; p.WPB = c.WPB;
    p.half_last = c.half; p.xcd = c.xcd;
    int total;
    irbw_layout(c, p.o_w2, p.o_cs, p.cs_floats, total);
    p.red_cap = c.region / (c.OT * 1024);
    p.xl_off = p.cs_floats + c.region;
    p.in_elems = (unsigned)((size_t)d.ic * d.N * d.H * d.W);
    p.vec = d.OW % 4 == 0 ? 4 : (d.OW % 2 == 0 ? 2 : 1);
    p.m_ew = (unsigned)(((1ULL << 32) + c.EW - 1) / c.EW);
    p.m_tx = umulhi_magic(p.tiles_x); p.m_ty = umulhi_magic(p.tiles_y); p.m_twq = umulhi_magic(p.TWq);
    p.dbg_t = nullptr;
    return p;
}

static bool irb_plan_wave(IrbDesc &d)
{
    IrbPlan &c = d.plan;
    if (!irbw_pick(d, c)) return false;
    c.family = IRB_WAVE;
    // a last group of at most 8 real channels in the single-strip kernel: packed into registers 0 / 1, the other half of its work skipped (ffgpu_irb_wave.inc irbw_chan)
    const int r = d.ec & 15;
    c.half = c.NSO == 1 && r >= 1 && r <= 8 && knob(K_IRBW_HALF) != 0;
    { const int x = knob(K_IRBW_XCD); c.xcd = c.G > 1 ? (x >> 1) & 1 : x & 1; }        // bit 0: one wave per tile, bit 1: group-split launches
    const IrbwP p = irbw_params(d);                                  // (the reduction region follows)
    c.pack_floats = p.o_cs + p.cs_floats;
    if (p.ntiles * std::max(p.tiles_x, p.tiles_y) >= (1L << 32) || p.ntiles >= (1L << 31)) { ffgpu_set_error("irbw: too many tiles for 32-bit index arithmetic"); return false; }
    // floats behind the shared constants: the waves' E slices, later the partial sums of the group split -- room for all
    // G of them when the launch leaves the CU's LDS to one workgroup anyway (no folding rounds: two barriers fewer)
    const int waves = c.G > 1 ? c.G : c.WPB;
    size_t region = (size_t)waves * 16 * c.NSI * 64;
    if (c.G > 1 && !knob(K_IRBW_FOLD)) {
        const size_t want = (size_t)c.G * c.OT * 1024;
        if (want > region && (p.cs_floats + want) * sizeof(float) <= 150 * 1024 && p.ntiles <= 512) region = want;
    }
    c.region = (int)region;
    c.lds = (int)(((size_t)p.cs_floats + region + (c.xl ? (size_t)c.NSI * 4 * 64 * IRBW_XL_DW : 0)) * sizeof(float));
    c.grid = (int)(c.G > 1 ? p.ntiles : (p.ntiles + c.WPB - 1) / c.WPB);
    c.block = waves * 64;
    for (int i = 0; i < irbw_nkernels; i++) {
        const IrbwKernel &k = irbw_kernels[i];
        if (k.KS1 == c.KS1 && k.OT == c.OT && k.S == d.stride && k.NSI == c.NSI && k.NSO == c.NSO && k.big == (c.big != 0) && k.x3 == (c.x3 != 0) && k.xl == (c.xl != 0)) { c.inst = i; return true; }
    }
    ffgpu_set_error("irbw: no instantiation for KS1=%d OT=%d S=%d NSI=%d NSO=%d big=%d x3=%d xl=%d", c.KS1, c.OT, d.stride, c.NSI, c.NSO, c.big, c.x3, c.xl);
    return false;
}

// ---- first layer + first thin block as one kernel (ffgpu_front.inc): the planner asks, then launches; the block's plan says that it is thin, and how many rows a wave takes
bool ffgpu_front_ok(const ConvDesc &c, const IrbDesc &d)
{
    return c.fs == 3 && c.stride == 2 && c.pad == 1 && c.groups == 1 && c.ic == 3 && c.oc == 8 && !c.residual && c.act != 3 &&
           c.iw == 2 * c.ow && c.ih == 2 * c.oh && c.ow % 4 == 0 && c.ow / 4 <= 64 && c.in_cs % 4 == 0 && c.in_ns % 4 == 0 &&
           3 * c.in_cs < (1L << 30) && c.out == d.in && d.plan.family == IRB_THIN && d.ic == 8 && d.ec == 8 && d.oc == 4 && !d.residual &&
           d.W == c.ow && d.H == c.oh && d.N == c.N &&
           (long)c.N * c.oh * c.ow >= knob(K_FRONT_MIN_PX) && !knob(K_NO_FRONT);
}

// form IN_U8: the frames of this forward are u8 BGR images described by the executor's parameter block (c.in_ind IS that block: its
// first member is the fp32 frame pointer the IN_F32 form reads)
// three columns per lane (54 of 64 lanes on a 160-pixel row instead of 40) where the row fits a wave that way; FFGPU_FRONT_NC=4: the round-1 form.
// ONE form for u8 and fp32 frames: each form sits within tolerance of the reference, but the two are not bit-identical to each other, and the same frames
// must give the same records whichever way they arrive (tests/test_gpu_round3.py::test_u8_frames_into_the_first_kernel)
int ffgpu_front_nc(const IrbDesc &d)
{
    return knob(K_FRONT_NC) == 3 && d.W >= 6 && (d.W + 2) / 3 <= 64 ? 3 : 4;
}

// forms IN_BGR_FRAMES / IN_NV12_FRAMES (the resizing forms): u8 frames of any size described one by one by the parameter block's frames_tab.  Three
// columns per lane only: the four-column form of the gather does not fit a wave's registers, so the executor stages those frames (ffgpu_front_nc == 4) instead.
// Which route NV12 frames take on plans that have the fused form: FFGPU_NV12_FRONT=1 the NV12 form of k_front, =0 staging (k_input4, ffgpu_input.inc);
// unset: FFGPU_NV12_FRONT_DEFAULT, the outcome of tools/nv12_frames_bench.py (DESIGN 5.15: fused only if it beats staging at four chains by more
// than the spread of the repeats).  Read at every call: it selects between two graphs, it changes neither.
#define FFGPU_NV12_FRONT_DEFAULT 0
bool ffgpu_front_nv12_fused() { return knob_or(K_NV12_FRONT, FFGPU_NV12_FRONT_DEFAULT) != 0; }

// the launch shape of k_front for a planned thin block: rows per wave, bands per frame, waves, workgroups of four waves
struct FrontGeom { int band, nbands, ntasks, grid; };
static FrontGeom front_geom(const IrbDesc &d)
{
    FrontGeom g;
    g.band = d.plan.front_band;
    g.nbands = (d.H + g.band - 1) / g.band;
    g.ntasks = d.N * g.nbands;
    g.grid = (g.ntasks + 3) / 4;
    return g;
}

// One line per launch of k_front (the probe behind ffgpu_front_plan_text): the instantiation ffgpu_launch_front dispatches to for `form` -- the template
// arguments OC, U8, NC, RS, NV -- and the launch shape; "staged" where the form has no instantiation for the plane (the resizing forms at four columns per lane)
int ffgpu_front_plan_line(const IrbDesc &d, InputForm form, char *buf, size_t cap)
{
    const bool resize = form == IN_BGR_FRAMES || form == IN_NV12_FRAMES;
    const int nc = ffgpu_front_nc(d);
    if (resize && nc != 3) return snprintf(buf, cap, "staged");
    const FrontGeom g = front_geom(d);
    return snprintf(buf, cap, "front<4,%d,%d,%d,%d> W=%d H=%d N=%d band=%d nbands=%d ntasks=%d grid=%d block=256",
                    form != IN_F32, nc, resize, form == IN_NV12_FRAMES, d.W, d.H, d.N, g.band, g.nbands, g.ntasks, g.grid);
}

int ffgpu_launch_front(const ConvDesc &c, const IrbDesc &d, InputForm form, hipStream_t s)
{
    const bool u8 = form == IN_U8, resize = form == IN_BGR_FRAMES || form == IN_NV12_FRAMES;
    if (!ffgpu_front_ok(c, d)) { ffgpu_set_error("front: unsupported layer pair"); return -1; }
    if ((u8 || resize) && !c.in_ind) { ffgpu_set_error("front: the u8 form needs the executor's parameter block"); return -1; }
    const int nc = ffgpu_front_nc(d);
    if (resize && nc != 3) { ffgpu_set_error("front: the resizing form has three columns per lane only (plane width %d)", d.W); return -1; }
    FrontP p;
    p.in = c.in; p.in_ind = c.in_ind; p.prm = reinterpret_cast<const ExecParams *>(c.in_ind); p.out = d.out; p.f0 = c.filt; p.w1 = d.w1; p.wd = d.wd; p.w2 = d.w2;
    p.in_cs = c.in_cs; p.in_ns = c.in_ns;
    p.W = d.W; p.H = d.H; p.N = d.N;
    const FrontGeom g = front_geom(d);
    p.band = g.band; p.nbands = g.nbands; p.ntasks = g.ntasks;
    p.act0 = act_slope(c.act); p.act1 = act_slope(d.act1); p.actd = act_slope(d.actd); p.act2 = act_slope(d.act2);
    const dim3 grid((unsigned)g.grid);
    if (form == IN_NV12_FRAMES) {
        hipLaunchKernelGGL((k_front<4, true, 3, true, true>), grid, dim3(256), 0, s, p);
    } else if (resize) {
        hipLaunchKernelGGL((k_front<4, true, 3, true>), grid, dim3(256), 0, s, p);
    } else if (nc == 3) {
        if (u8) hipLaunchKernelGGL((k_front<4, true, 3>), grid, dim3(256), 0, s, p);
        else    hipLaunchKernelGGL((k_front<4, false, 3>), grid, dim3(256), 0, s, p);
    } else {
        if (u8) hipLaunchKernelGGL((k_front<4, true>), grid, dim3(256), 0, s, p);
        else    hipLaunchKernelGGL((k_front<4, false>), grid, dim3(256), 0, s, p);   // (8 output channels would need 20 more registers than a wave has)
    }
    LAUNCH_OK("front");
    return 0;
}

// ---- workgroup form (ffgpu_irb.inc): the fallback
// expanded channels per chunk: 16 keeps the LDS footprint small (more workgroups per CU), 32 halves the chunk count
static int irb_ech(const IrbDesc &d)
{
    const int force = knob(K_IRB_ECH);
    if (force == 16 || force == 32) return d.ec <= 16 ? 16 : force;
    if (d.ec <= 16) return 16;
    // measured (profiles/r01_irb_tile_sweep.txt): short K loops gain more from the extra workgroups per CU
    if ((d.stride == 2 && d.OW >= 64) || (d.stride == 1 && d.OW >= 32 && d.OW < 64 && d.ec <= 48)) return 16;
    return 32;
}

static int irb_chunk_floats(int k4, int ECH, int OT)
{
    return (k4 * ECH + ECH * OT * 16 + ECH * IRB_TAPP + ECH * 2 + 3) & ~3;
}

// wbufs = chunk-constant buffers in LDS: nchunks (resident), 2 (streamed through registers) or 1 (single chunk)
static size_t irb_lds_floats(int k4, int ECH, int OT, int NPin, int wbufs)
{
    return (size_t)k4 * NPin + (size_t)ECH * NPin + NPin + (size_t)wbufs * irb_chunk_floats(k4, ECH, OT) + OT * 32 + 2 * (size_t)NPin;
}

// Keep every chunk's constants in LDS when that costs no co-resident workgroup: the streamed alternative pays one
// global-load latency per chunk per tile, which is most of the run time of the small-plane blocks.
static int irb_wbufs(int k4, int ECH, int OT, int NPin, int nchunks, long ntiles)
{
    if (nchunks == 1) return 1;
    const int resident = knob(K_IRB_RESIDENT);
    if (resident == 0) return 2;
    const size_t a = irb_lds_floats(k4, ECH, OT, NPin, 2) * sizeof(float), b = irb_lds_floats(k4, ECH, OT, NPin, nchunks) * sizeof(float);
    if (b > IRB_LDS_MAX - 8 * 1024) return 2;
    const int want = (int)std::min(4L, (ntiles + 255) / 256);      // workgroups per CU the launch can use at all
    const int bpa = std::min(want, (int)(IRB_LDS_MAX / a)), bpb = std::min(want, (int)(IRB_LDS_MAX / b));
    return (bpb >= bpa || bpb >= 2 || resident == 2) ? nchunks : 2;
}

static void irb_geometry(const IrbDesc &d, int TH, int TW, int NF, IrbP &p)
{
    const int S = d.stride;
    p.TH = TH; p.TW = TW; p.TWq = (TW + 3) / 4; p.NF = NF;
    p.EH = (TH - 1) * S + 3;
    int ew = (p.TWq * 4 - 1) * S + 3;                 // columns a full (padded) quad row can touch
    p.EW = (ew + 3) & ~3;
    p.NPin = (NF * p.EH * p.EW + 63) & ~63;
    p.NPout = NF * TH * p.TWq * 4;
    p.tiles_x = (d.OW + TW - 1) / TW; p.tiles_y = (d.OH + TH - 1) / TH;
}

static bool irb_pick_tile(const IrbDesc &d, int ECH, IrbP &best)
{
    const int k4 = (d.ic + 3) & ~3, OT = (d.oc + 15) / 16;
    const int nchunks = (d.ec + ECH - 1) / ECH;
    const int force_tw = knob(K_IRB_TW);
    double best_score = -1.0;
    // measured preferences (tools/tune_irb.py, batch 64, profiles/r01_irb_tile_sweep.txt); the scored search
    // below is the fallback for shapes the table does not fit
    {
        int TW, TH;
        if (d.stride == 1) {
            if (d.OW >= 64)      { TW = d.ec <= 16 ? 32 : 16; TH = 16; }
            else if (d.OW >= 32) { TW = d.ec <= 48 ? 32 : 16; TH = d.ec <= 48 ? 10 : 8; }
            else                 { TW = d.OW; TH = 5; }
        } else {
            if (d.OW >= 64)      { TW = 16; TH = 10; }
            else if (d.OW >= 32) { TW = 8; TH = 10; }
            else if (d.OW > 10)  { TW = d.OW; TH = 5; }
            else                 { TW = d.OW; TH = 4; }
        }
        if (TH > d.OH) TH = d.OH;
        IrbP p;
        irb_geometry(d, TH, TW, 1, p);
        const size_t lds = irb_lds_floats(k4, ECH, OT, p.NPin, nchunks > 1 ? 2 : 1) * sizeof(float);
        if (!force_tw && !knob(K_IRB_NOTABLE) && TW <= d.OW && p.NPout <= 512 && p.NPin <= 1024 && lds <= 150 * 1024) {
            best = p;
            return true;
        }
    }
    const int force_th = knob(K_IRB_TH), force_nf = knob(K_IRB_NF);
    const int tws[4] = { d.OW <= 24 ? d.OW : 16, 32, 8, force_tw };
    for (int twi = 0; twi < 4; twi++) {
        const int TW = tws[twi];
        if (TW < 1 || (TW > d.OW && twi > 0) || (force_tw && TW != force_tw)) continue;
        for (int TH = 1; TH <= 32; TH++) {
            if (TH > d.OH) break;
            if (force_th ? TH != force_th : (TH != d.OH && TH != (d.OH + 1) / 2 && TH != 16 && TH != 8 && TH != 4 && TH != 5 && TH != 10)) continue;
            for (int NF = 1; NF <= 4; NF *= 2) {
                if (force_nf && NF != force_nf) continue;
                if (NF > 1 && (TH < d.OH || TW < d.OW)) continue;      // several frames only for whole planes
                if (NF > d.N) continue;
                IrbP p;
                irb_geometry(d, TH, TW, NF, p);
                if (p.NPout > 512 || p.NPin > 1024) continue;
                const size_t lds = irb_lds_floats(k4, ECH, OT, p.NPin, nchunks > 1 ? 2 : 1) * sizeof(float);
                if (lds > 150 * 1024) continue;
                const long nblocks = (long)p.tiles_x * p.tiles_y * ((d.N + NF - 1) / NF);
                const double useful = (double)NF * TH * TW;
                const double work_eff = useful * d.stride * d.stride / p.NPin;            // expand work that is not halo / padding
                const double lane_eff = useful / (((p.NPout + 63) / 64) * 64.0);
                const double edge_eff = ((double)d.OW * d.OH) / ((double)p.tiles_x * TW * p.tiles_y * TH);
                const double fill = nblocks >= 512 ? 1.0 : (nblocks >= 256 ? 0.9 : nblocks / 256.0 * 0.9);
                const int bpc = (int)(160 * 1024 / lds);
                const double occ = bpc >= 3 ? 1.0 : (bpc == 2 ? 0.9 : 0.7);               // workgroups per CU hide each other's load phase
                const double score = work_eff * lane_eff * edge_eff * fill * occ;
                if (score > best_score) { best_score = score; best = p; }
            }
        }
    }
    return best_score > 0;
}

typedef int (*IrbLaunch)(const IrbP &, const IrbPlan &, hipStream_t);
struct IrbKernel { int MT, OT, S, NW; IrbLaunch launch; };          // NW waves per workgroup: 8 with one pixel strip per wave, 4 with two
#define IRB_K(mt, ot) { mt, ot, 1, 8, irb_launch_t<IrbP, k_irb<mt, ot, 1, 1, 8>> }, { mt, ot, 2, 8, irb_launch_t<IrbP, k_irb<mt, ot, 1, 2, 8>> }, \
                      { mt, ot, 1, 4, irb_launch_t<IrbP, k_irb<mt, ot, 2, 1, 4>> }, { mt, ot, 2, 4, irb_launch_t<IrbP, k_irb<mt, ot, 2, 2, 4>> }
static const IrbKernel irb_kernels[] = { IRB_K(1, 1), IRB_K(1, 2), IRB_K(1, 3), IRB_K(2, 1), IRB_K(2, 2), IRB_K(2, 3) };
#undef IRB_K

// the parameter block of a planned k_irb launch: arithmetic on the descriptor and the plan's tile, chunk size, KS, wbufs and red_off
static IrbP irb_params(const IrbDesc &d)
{
    const IrbPlan &c = d.plan;
    IrbP p;
    irb_geometry(d, c.TH, c.TW, c.NF, p);
    p.in = d.in; p.out = d.out; p.residual = d.residual; p.pk = d.pk;
    p.N = d.N; p.H = d.H; p.W = d.W; p.OH = d.OH; p.OW = d.OW; p.ic = d.ic; p.ec = d.ec; p.oc = d.oc; p.stride = d.stride;
    p.act1 = act_slope(d.act1); p.actd = act_slope(d.actd); p.act2 = act_slope(d.act2); p.res_act = act_slope(d.res_act);
    p.k4 = (d.ic + 3) & ~3; p.ECH = c.ECH; p.nchunks = (d.ec + c.ECH - 1) / c.ECH; p.CH = irb_chunk_floats(p.k4, c.ECH, c.OT);
    p.vec_store = (d.OW % 4 == 0) && (p.TW % 4 == 0);
    p.dbg_skip = knob(K_IRB_SKIP); p.dbg_t = nullptr;
    p.ntiles = p.tiles_x * p.tiles_y * ((d.N + p.NF - 1) / p.NF);
    p.KS = c.KS; p.red_off = c.red_off;
    p.resident = p.nchunks > 1 && c.wbufs == p.nchunks;
    const int nsi = p.NPin / 64;
    p.inv_nsi = (65536 + nsi - 1) / nsi;
    return p;
}

static bool irb_plan_wg(IrbDesc &d)
{
    IrbPlan &c = d.plan;
    if (d.stride != 1 && d.stride != 2) return false;
    if (d.oc > 48 || d.ic > 64 || d.ec < 1) return false;
    if (d.act1 == 3 || d.actd == 3 || d.act2 == 3 || d.res_act == 3) return false;
    if (((long)d.H * d.W) % 4 || ((long)d.OH * d.OW) % 4) return false;      // CNHW planes stay 16-byte aligned
    IrbP p;
    c.ECH = irb_ech(d); c.OT = (d.oc + 15) / 16;
    if (!irb_pick_tile(d, c.ECH, p)) return false;
    c.family = IRB_WG; c.TH = p.TH; c.TW = p.TW; c.NF = p.NF;
    p = irb_params(d);                                               // (KS, wbufs and red_off follow)
    c.pack_floats = (int)(((size_t)p.nchunks * p.CH + c.OT * 32 + 63) & ~(size_t)63);
    const int nso = (p.NPout + 63) / 64, nsi = p.NPin / 64;
    c.NW = knob(K_IRB_NW) == 4 ? 4 : 8;                  // waves per workgroup
    c.KS = 1;
    while (c.KS * 2 * nso <= c.NW && c.KS < 4) c.KS *= 2;            // idle waves take slices of the channel loop
    if (knob(K_IRB_NOKS)) c.KS = 1;
    c.wbufs = irb_wbufs(p.k4, p.ECH, c.OT, p.NPin, p.nchunks, p.ntiles);
    for (int wi = 0; wi < p.k4 * nsi; wi++)
        if (((wi * p.inv_nsi) >> 16) != wi / nsi) { ffgpu_set_error("irb: strip reciprocal inexact (k4 %d, %d strips)", p.k4, nsi); return false; }
    size_t lds = irb_lds_floats(p.k4, p.ECH, c.OT, p.NPin, c.wbufs) * sizeof(float);
    for (;; c.KS /= 2) {                                             // reduce-scatter scratch: alias In..E when it fits, else append
        const size_t need = c.KS > 1 ? (size_t)c.KS * nso * c.OT * 1024 : 0;
        // (a workgroup that runs a single tile is done with Msk and the chunk constants too by then)
        const size_t alias_cap = (size_t)(p.k4 + p.ECH) * p.NPin + (p.ntiles <= 256 ? (size_t)p.NPin + (size_t)c.wbufs * p.CH : 0);
        if (need <= alias_cap) break;
        if (lds + need * sizeof(float) <= IRB_LDS_MAX) { c.red_off = (int)(lds / sizeof(float)); lds += need * sizeof(float); break; }
    }
    const int bpc = std::max(1, std::min(4, (int)(IRB_LDS_MAX / lds)));
    c.lds = (int)lds; c.grid = (int)std::min(256L * bpc, (long)p.ntiles); c.block = c.NW * 64;
    for (int i = 0; i < (int)(sizeof irb_kernels / sizeof irb_kernels[0]); i++)
        if (irb_kernels[i].MT == c.ECH / 16 && irb_kernels[i].OT == c.OT && irb_kernels[i].S == d.stride && irb_kernels[i].NW == c.NW) { c.inst = i; return true; }
    return false;                                                    // (unreachable: ECH is 16 or 32, OT <= 3)
}

bool ffgpu_irb_plan(IrbDesc &d)
{
    IrbPlan &c = d.plan;
    c = IrbPlan{};
    if (irb_thin_ok(d)) {
        const int band = thin_band(d.N, d.H);
        c.family = IRB_THIN; c.pack_floats = 64;
        c.band = knob_or(K_THIN_BAND, band); c.front_band = knob_or(K_FRONT_BAND, band);
        c.grid = (int)((thin_params(d).ntasks + 3) / 4); c.block = 256;
        return true;
    }
    if (irb_plan_wave(d)) return true;
    c = IrbPlan{};
    if (irb_plan_wg(d)) return true;
    c = IrbPlan{};
    return false;
}

static bool irb_planned(const IrbDesc &d, const char *who)
{
    if (d.plan.family == IRB_NONE) ffgpu_set_error("%s: the block has no plan (ffgpu_irb_plan has not run on it, or refused it)", who);
    return d.plan.family != IRB_NONE;
}

size_t ffgpu_irb_pack_floats(const IrbDesc &d) { return irb_planned(d, "irb_pack_floats") ? (size_t)d.plan.pack_floats : 0; }

int ffgpu_irb_pack(const IrbDesc &d, float *pk, hipStream_t s)
{
    const IrbPlan &c = d.plan;
    if (!irb_planned(d, "irb_pack")) return -1;
    if (c.family == IRB_THIN) return 0;
    if (c.family == IRB_WAVE) {
        IrbwPackP q; q.w1 = d.w1; q.wd = d.wd; q.w2 = d.w2; q.pk = pk; q.ic = d.ic; q.ec = d.ec; q.oc = d.oc;
        q.k4 = (d.ic + 3) & ~3; q.OT = c.OT; q.ngroups = c.ngroups; q.x3 = c.x3; q.half = c.half;
        hipLaunchKernelGGL(k_irbw_pack, dim3((c.pack_floats + 255) / 256), dim3(256), 0, s, q);
        LAUNCH_OK("irbw_pack");
        return 0;
    }
    IrbPackP q;
    q.w1 = d.w1; q.wd = d.wd; q.w2 = d.w2; q.pk = pk;
    q.ic = d.ic; q.ec = d.ec; q.oc = d.oc;
    q.k4 = (d.ic + 3) & ~3; q.ECH = c.ECH; q.MT = c.ECH / 16; q.OT = c.OT; q.nchunks = (d.ec + c.ECH - 1) / c.ECH; q.CH = irb_chunk_floats(q.k4, c.ECH, c.OT);
    const int total = q.nchunks * q.CH + q.OT * 32;
    hipLaunchKernelGGL(k_irb_pack, dim3((total + 255) / 256), dim3(256), 0, s, q);
    LAUNCH_OK("irb_pack");
    return 0;
}

// One canonical line per planned block (the probe behind ffgpu_irb_plan_text, tests/test_irb_choice.py; FFGPU_VERBOSE_IRB prints it per launch): family and instantiation, every scalar of
// the parameter block the launch would pass, the launch shape, `half` and the size of the packed image
// the head of that line: one key per instantiation.  ffgpu_irb_keys walks the same three tables with the same three formatters, so a row added to a table is in the list
static int irb_thin_key(int ic, int oc, char *key, size_t cap) { return snprintf(key, cap, "thin<%d,8,%d>", ic, oc); }
static int irbw_key(const IrbwKernel &k, char *key, size_t cap)
{
    if (k.NSO == 2) return snprintf(key, cap, "irbw2<%d,%d%s>", k.KS1, k.NSI, k.x3 ? ",x3" : "");
    return snprintf(key, cap, "irbw<%d,%d,%d,%d%s%s%s>", k.KS1, k.OT, k.S, k.NSI, k.big ? ",big" : "", k.x3 ? ",x3" : "", k.xl ? ",xl" : "");
}
static int irb_key(const IrbKernel &k, char *key, size_t cap) { return snprintf(key, cap, "irb<%d,%d,%d,%d,%d>", k.MT, k.OT, k.S, k.NW == 8 ? 1 : 2, k.NW); }

// every instantiation the three families have, one key per line (ffgpu_irb_instantiations): thin, then irbw_kernels[], then irb_kernels[] (both wave counts are rows of it)
int ffgpu_irb_keys(char *buf, size_t cap)
{
    size_t n = 0;
    char key[48];
    auto put = [&]() { n += (size_t)snprintf(n < cap ? buf + n : nullptr, n < cap ? cap - n : 0, "%s\n", key); };
    for (const IrbThinKernel &k : irb_thin_kernels) { irb_thin_key(k.IC, k.OC, key, sizeof key); put(); }
    for (const IrbwKernel &k : irbw_kernels) { irbw_key(k, key, sizeof key); put(); }
    for (const IrbKernel &k : irb_kernels) { irb_key(k, key, sizeof key); put(); }
    return (int)n;
}

int ffgpu_irb_plan_line(const IrbDesc &d, char *buf, size_t cap)
{
    const IrbPlan &c = d.plan;
    char key[48];
    if (c.family == IRB_THIN) {
        const ThinP p = thin_params(d);
        irb_thin_key(d.ic, d.oc, key, sizeof key);
        return snprintf(buf, cap, "%s W=%d H=%d N=%d band=%d nbands=%d act=%g,%g,%g,%g ntasks=%ld lds=%d grid=%d block=%d half=%d pack=%d",
                        key, p.W, p.H, p.N, p.band, p.nbands, p.act1, p.actd, p.act2, p.res_act, p.ntasks, c.lds, c.grid, c.block, c.half, c.pack_floats);
    }
    if (c.family == IRB_WAVE) {
        const IrbwP p = irbw_params(d);
        const IrbwKernel &k = irbw_kernels[c.inst];
        irbw_key(k, key, sizeof key);
        return snprintf(buf, cap, "%s N=%d H=%d W=%d OH=%d OW=%d ic=%d ec=%d oc=%d act=%g,%g,%g,%g tile=%d,%d,%d,%d tiles=%d,%d,%ld ngroups=%d G=%d WPB=%d o_w2=%d o_cs=%d cs_floats=%d "
                        "xl_off=%d red_cap=%d in_elems=%u vec=%d half_last=%d m=%u,%u,%u,%u xcd=%d lds=%d grid=%d block=%d half=%d pack=%d",
                        key, p.N, p.H, p.W, p.OH, p.OW, p.ic, p.ec, p.oc, p.act1, p.actd, p.act2, p.res_act, p.TWq, p.TH, p.EW, p.EH, p.tiles_x, p.tiles_y, p.ntiles, p.ngroups, p.G, p.WPB,
                        p.o_w2, p.o_cs, p.cs_floats, p.xl_off, p.red_cap, p.in_elems, p.vec, p.half_last, p.m_ew, p.m_tx, p.m_ty, p.m_twq, p.xcd, c.lds, c.grid, c.block, c.half, c.pack_floats);
    }
    if (c.family == IRB_WG) {
        const IrbP p = irb_params(d);
        const IrbKernel &k = irb_kernels[c.inst];
        irb_key(k, key, sizeof key);
        return snprintf(buf, cap, "%s N=%d H=%d W=%d OH=%d OW=%d ic=%d ec=%d oc=%d stride=%d act=%g,%g,%g,%g tile=%d,%d,%d,%d,%d,%d NPin=%d NPout=%d tiles=%d,%d,%d "
                        "k4=%d nchunks=%d ECH=%d CH=%d KS=%d red_off=%d vec_store=%d resident=%d inv_nsi=%d lds=%d grid=%d block=%d half=%d pack=%d",
                        key, p.N, p.H, p.W, p.OH, p.OW, p.ic, p.ec, p.oc, p.stride, p.act1, p.actd, p.act2, p.res_act, p.TH, p.TW, p.TWq, p.NF, p.EH, p.EW,
                        p.NPin, p.NPout, p.tiles_x, p.tiles_y, p.ntiles, p.k4, p.nchunks, p.ECH, p.CH, p.KS, p.red_off, p.vec_store, p.resident, p.inv_nsi, c.lds, c.grid, c.block, c.half, c.pack_floats);
    }
    return snprintf(buf, cap, "unsupported");
}

// one line per launch of a planned block that the streaming stride-2 form may take: the form (thin_s2<4,24,8,3>, or the planned key where the launch
// follows the plan), frames per wave, band (rows per task), tasks and grid -- pure host arithmetic (ffgpu_irb_s2_launch_text; tests/test_thin_s2_host.py)
int ffgpu_irb_s2_launch_line(const IrbDesc &d, char *buf, size_t cap)
{
    const IrbPlan &c = d.plan;
    char key[48];
    if (c.family == IRB_NONE) return snprintf(buf, cap, "unsupported");
    if (c.family == IRB_THIN) {
        const ThinP p = thin_params(d);
        irb_thin_key(d.ic, d.oc, key, sizeof key);
        return snprintf(buf, cap, "%s frames=1 band=%d tasks=%ld grid=%d block=%d", key, p.band, p.ntasks, c.grid, c.block);
    }
    if (const ThinS2Form f = thin_s2_form(d); f.on)
        return snprintf(buf, cap, "thin_s2<%d,%d,%d,%d> frames=%d band=%d tasks=%ld grid=%d block=256 W=%d H=%d N=%d lanes=%d nbands=%d",
                        d.ic, d.ec, d.oc, THIN_S2_NC, f.F, f.band, f.ntasks, f.grid, d.W, d.H, d.N, f.lpr, f.nbands);
    long tiles;
    if (c.family == IRB_WAVE) { irbw_key(irbw_kernels[c.inst], key, sizeof key); tiles = irbw_params(d).ntiles; }
    else { irb_key(irb_kernels[c.inst], key, sizeof key); tiles = irb_params(d).ntiles; }
    return snprintf(buf, cap, "%s frames=%d band=%d tasks=%ld grid=%d block=%d", key, c.family == IRB_WG ? c.NF : 1, c.TH, tiles, c.grid, c.block);
}

int ffgpu_launch_irb(const IrbDesc &d, hipStream_t s)
{
    const IrbPlan &c = d.plan;
    if (!irb_planned(d, "irb")) return -1;
    if (knob(K_VERBOSE_IRB)) { char line[1024]; ffgpu_irb_plan_line(d, line, sizeof line); fprintf(stderr, "%s\n", line); }
    if (c.family == IRB_THIN) return launch_irb_thin(d, s);
    if (const ThinS2Form f = thin_s2_form(d); f.on) return launch_irb_thin_s2(d, f, s);      // the launch's choice; the plan and its image stay the wave form's
    if (!d.pk) { ffgpu_set_error("irb: constants not packed"); return -1; }
    return c.family == IRB_WAVE ? irbw_kernels[c.inst].launch(irbw_params(d), c, s) : irb_kernels[c.inst].launch(irb_params(d), c, s);
}

// ---- a run of blocks on one small plane as one launch (ffgpu_irb_stage.inc).  The run is described by its blocks' own descriptors: each keeps the plan
// ffgpu_irb_plan gave it and the image ffgpu_irb_pack wrote for that plan, and the stage kernel reads those images.  It takes a run only where every
// block's plan is the XL form with seven waves and unfolded partial sums -- the summation order the stage kernel reproduces bit for bit.
static bool irb_stage_params(const IrbDesc *blocks, int B, IrbStageP &p, size_t &lds)
{
    if (B < 2 || B > IRBS_MAXB) return false;
    const IrbDesc &d0 = blocks[0];
    for (int b = 0; b < B; b++) {
        const IrbDesc &d = blocks[b];
        const IrbPlan &c = d.plan;
        if (d.ic != 48 || d.ec != 224 || d.oc != 48 || d.stride != 1 || d.OH != d.H || d.OW != d.W) return false;
        if (d.N != d0.N || d.H != d0.H || d.W != d0.W || d.act1 != d0.act1 || d.actd != d0.actd) return false;
        if (act_slope(d.act2) != 1.f || act_slope(d.res_act) != 1.f) return false;
        if (c.family != IRB_WAVE || !c.xl || !c.x3 || c.half || c.G != IRBS_WAVES || c.KS1 != 12 || c.OT != 3 || c.ngroups != 2 * IRBS_WAVES) return false;
        if (c.region / (c.OT * 1024) < c.G) return false;                  // (k_irbw would fold the upper waves' sums onto the lower ones first)
    }
    const int plane = d0.H * d0.W, TWq = (d0.W + 3) / 4;
    if (plane > 128 || TWq * d0.H > 32) return false;                      // two expand strips, two strips of output quads
    p = IrbStageP{};
    p.B = B; p.N = d0.N; p.H = d0.H; p.W = d0.W;
    p.act1 = act_slope(d0.act1); p.actd = act_slope(d0.actd);
    p.TWq = TWq; p.P = 4 * TWq + 2; p.EP = p.P * (d0.H + 2);
    int total;
    irbw_layout(d0.plan, p.o_w2, p.o_cs, p.cs_floats, total);
    if (p.cs_floats > 2 * IRBS_WAVES * 64 * 4) return false;
    p.e_off = p.cs_floats;
    p.e_slice = std::max(16 * p.EP, 2048);                                 // 8 pair planes; a reduction pass parks 2 x 4 rows of 256 floats
    p.xi_off = p.e_off + IRBS_WAVES * p.e_slice;
    p.f_off = p.xi_off + 2 * 4 * 64 * IRBW_XL_DW;
    lds = (size_t)(p.f_off + 48 * plane) * sizeof(float);
    p.m_w = umulhi_magic(d0.W); p.m_twq = umulhi_magic(TWq); p.m_plane = umulhi_magic(plane);
    return lds <= IRB_LDS_MAX;
}

bool ffgpu_irb_stage_ok(const IrbDesc *blocks, int B)
{
    IrbStageP p; size_t lds;
    return irb_stage_params(blocks, B, p, lds);
}

// (the probe behind ffgpu_irb_stage_plan_text, tests/test_irb_stage_plan.py) wanted: the executor's own conditions hold
int ffgpu_irb_stage_line(const IrbDesc *blocks, int B, bool wanted, char *buf, size_t cap)
{
    IrbStageP p; size_t lds;
    if (!wanted || !irb_stage_params(blocks, B, p, lds)) return snprintf(buf, cap, "blocks B=%d launches=%d", B, B);
    return snprintf(buf, cap, "stage B=%d launches=1 N=%d H=%d W=%d act=%g,%g TWq=%d P=%d EP=%d o_w2=%d o_cs=%d cs_floats=%d e_off=%d e_slice=%d xi_off=%d f_off=%d m=%u,%u,%u lds=%zu grid=%d block=%d",
                    p.B, p.N, p.H, p.W, p.act1, p.actd, p.TWq, p.P, p.EP, p.o_w2, p.o_cs, p.cs_floats, p.e_off, p.e_slice, p.xi_off, p.f_off, p.m_w, p.m_twq, p.m_plane, lds, p.N, IRBS_WAVES * 64);
}

int ffgpu_launch_irb_stage(const IrbDesc *blocks, int B, hipStream_t s)
{
    IrbStageP p; size_t lds;
    if (!irb_stage_params(blocks, B, p, lds)) { ffgpu_set_error("irb_stage: the run of %d blocks does not fit the stage kernel", B); return -1; }
    p.in = blocks[0].in; p.out = blocks[B - 1].out;
    for (int b = 0; b < B; b++) {
        if (!blocks[b].pk) { ffgpu_set_error("irb_stage: constants not packed"); return -1; }
        p.pk[b] = blocks[b].pk;
    }
    if (!p.in || !p.out) { ffgpu_set_error("irb_stage: no tensors"); return -1; }
    if (lds_allow((const void *)k_irb_stage, lds, "irb_stage")) return -1;
    hipLaunchKernelGGL(k_irb_stage, dim3((unsigned)p.N), dim3(IRBS_WAVES * 64), lds, s, p);
    LAUNCH_OK("irb_stage");
    return 0;
}
