// ffgpu_knobs.hpp -- every environment variable the device library reads: ONE table (name, how its value is parsed, its default, what it is
// for, one line of text) and the only functions that call getenv.  Plain C++17 with no HIP in it; both translation units include it.
//
// Kinds (how a value is parsed):
//   INT   unset or empty: the default; otherwise atoi
//   ON    atoi != 0 (unset, empty, "0", "abc": off)
//   SET   present at all, an empty value included ("0" is ON: FFGPU_NO_U8_FRONT=0 stages the frames)
//   TEXT  the string itself
// Defaults: a number, stated here and nowhere else, or KNOB_COMPUTED -- the default depends on the shape or the build, and the reader passes it
// (knob_or).  Classes: PRODUCT (a switch an integrator may set: INTEGRATION.md section 6 describes it), TUNING (moves a threshold or forces a
// choice AUTO makes; for the tools and the sweeps), TEST (forces a path the tests must reach), LAB (diagnostics, and what only a lab build has).
//
// The rule for WHEN: a knob is read where it is used, each time it is used -- nothing is cached per process, nothing is snapshot when the library
// loads or an executor is created, so a process that changes its environment sees the change at the next read.  What must not change under a
// packed image or a captured graph is frozen in the plan, not in the environment: ConvDesc::kernel / nsplit / x3_mt, IrbDesc::plan, a graph's launch list.
#pragma once
#include <assert.h>
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>

enum KnobKind { KNOB_INT, KNOB_ON, KNOB_SET, KNOB_TEXT };
enum KnobClass { KNOB_PRODUCT, KNOB_TUNING, KNOB_TEST, KNOB_LAB };
#define KNOB_COMPUTED INT_MIN

// X(id, name, kind, default, class, text): K_<id> is the index
#define FFGPU_KNOBS_MAIN(X) \
    /* ---- the executor (ffgpu_exec.hip, ffgpu_node.inc) */ \
    X(COMPAT_V6,         "FFCNN_COMPAT_V6",         ON,   0,             PRODUCT, "the reference's v6 behaviour for 5x5 filters (executors and groupconv)") \
    X(NO_GRAPH,          "FFGPU_NO_GRAPH",          ON,   0,             PRODUCT, "eager launches instead of a captured graph (as the flag FFGPU_NO_GRAPH)") \
    X(BF16_PW,           "FFGPU_BF16_PW",           ON,   0,             PRODUCT, "opt-in bf16 inputs for compute-bound pointwise layers; own tolerance (as the flag)") \
    X(NO_FUSE,           "FFGPU_NO_FUSE",           ON,   0,             PRODUCT, "one kernel per layer: no fused blocks, no concat in place, no residual in the conv epilogue (as the flag)") \
    X(BRANCH,            "FFGPU_BRANCH",            ON,   0,             PRODUCT, "first detection head as a parallel graph branch instead of in line") \
    X(DWPW,              "FFGPU_DWPW",              ON,   0,             PRODUCT, "the heads' depthwise + pointwise pairs as one kernel (measured slower)") \
    X(NO_U8_FRONT,       "FFGPU_NO_U8_FRONT",       SET,  0,             PRODUCT, "u8 frames through the staging kernel and the fp32 first kernel even where they could go straight in") \
    X(NV12_FRONT,        "FFGPU_NV12_FRONT",        INT,  KNOB_COMPUTED, PRODUCT, "1: NV12 frames into the NV12 form of k_front where the plan has it, 0: staged; default: the build's measured choice") \
    X(VERBOSE,           "FFGPU_VERBOSE",           SET,  0,             PRODUCT, "print every error to stderr as it is set") \
    X(NODE_PACK_BOXES,   "FFGPU_NODE_PACK_BOXES",   INT,  0,             PRODUCT, "room per frame in a shard's packed record block; 0 or less: 16, the constant of the same name in ffgpu_node.inc") \
    X(NO_IRB,            "FFGPU_NO_IRB",            ON,   0,             TUNING,  "no fused inverted-residual blocks: their three layers as three kernels") \
    X(IRB_MIN_EC,        "FFGPU_IRB_MIN_EC",        INT,  24,            TUNING,  "fewest expanded channels of a block the planner fuses (thin blocks apart)") \
    X(IRB_STAGE,         "FFGPU_IRB_STAGE",         INT,  1,             TUNING,  "runs of 48 -> 224 -> 48 blocks on a small plane as one launch in FFGPU_CONCURRENT executors of 32 frames or more (0: one launch per block)") \
    X(SPLIT_PARTS,       "FFGPU_SPLIT_PARTS",       INT,  2,             TUNING,  "parallel chains of an FFGPU_SPLIT2 executor: 2, 4 or 8 (where the batch divides)") \
    X(NO_INDIRECT,       "FFGPU_NO_INDIRECT",       ON,   0,             TEST,    "the first kernel takes the input address from its arguments, not the parameter block: graphs keyed by input pointer") \
    /* ---- which kernel AUTO takes for a convolution (conv_pick and its *_auto) */ \
    X(FORCE_GENERIC,     "FFGPU_FORCE_GENERIC",     INT,  0,             PRODUCT, "the reference-order generic kernel for every convolution") \
    X(PW_X3,             "FFGPU_PW_X3",             INT,  1,             PRODUCT, "0: never pick the split-bf16 pointwise kernel k_pw_x3") \
    X(PWX3_MIN_IC,       "FFGPU_PWX3_MIN_IC",       INT,  192,           TUNING,  "k_pw_x3: fewest input channels AUTO takes it for") \
    X(PWX3_MIN_OC,       "FFGPU_PWX3_MIN_OC",       INT,  256,           TUNING,  "k_pw_x3: fewest output channels") \
    X(PWX3_MIN_P,        "FFGPU_PWX3_MIN_P",        INT,  65536,         TUNING,  "k_pw_x3: fewest pixels") \
    X(PWX3_MT,           "FFGPU_PWX3_MT",           INT,  0,             TUNING,  "k_pw_x3: 16-row blocks per wave, 1 / 2 / 4 (0: 4)") \
    X(PW_X3T,            "FFGPU_PW_X3T",            INT,  1,             PRODUCT, "0: never pick the tiled split-bf16 GEMM k_pw_x3t") \
    X(PWX3T_MIN_IC,      "FFGPU_PWX3T_MIN_IC",      INT,  128,           TUNING,  "k_pw_x3t: fewest input channels AUTO takes it for") \
    X(PWX3T_MIN_OC,      "FFGPU_PWX3T_MIN_OC",      INT,  192,           TUNING,  "k_pw_x3t: fewest output channels") \
    X(PWX3T_MIN_P,       "FFGPU_PWX3T_MIN_P",       INT,  65536,         TUNING,  "k_pw_x3t: fewest pixels") \
    X(PWXT_TM,           "FFGPU_PWXT_TM",           INT,  256,           TUNING,  "k_pw_x3t: channels per workgroup tile, 256 or 128 (frozen with a plan: ConvDesc::x3_mt)") \
    X(PWXT_NARROW,       "FFGPU_PWXT_NARROW",       INT,  1,             TUNING,  "k_pw_x3t: 0 switches the narrow tiles of the partial last round off") \
    X(PWXT_PERSIST,      "FFGPU_PWXT_PERSIST",      INT,  0,             TUNING,  "k_pw_x3t: persistent workgroups over the main tiles") \
    X(PWXT_NT,           "FFGPU_PWXT_NT",           INT,  -1,            TUNING,  "k_pw_x3t: non-temporal output stores never (0) / always (1); -1: outputs of 128 MB and more") \
    X(PWXT_DBG,          "FFGPU_PWXT_DBG",          INT,  0,             LAB,     "k_pw_x3t: ablation mask handed to the kernel (wrong results)") \
    X(PW_X3S,            "FFGPU_PW_X3S",            INT,  1,             PRODUCT, "0: never pick the pointwise form of k_conv_x3 (pw_x3s)") \
    X(PWX3S_MIN_IC,      "FFGPU_PWX3S_MIN_IC",      INT,  96,            TUNING,  "pw_x3s: fewest input channels AUTO takes it for") \
    X(PWX3S_MIN_OC,      "FFGPU_PWX3S_MIN_OC",      INT,  64,            TUNING,  "pw_x3s: fewest output channels") \
    X(PWX3S_MIN_WGS,     "FFGPU_PWX3S_MIN_WGS",     INT,  64,            TUNING,  "pw_x3s: fewest workgroups") \
    X(IG_X3,             "FFGPU_IG_X3",             INT,  1,             PRODUCT, "0: never pick the split-bf16 dense 3x3 kernel k_conv_x3") \
    X(IGX3_S2,           "FFGPU_IGX3_S2",           INT,  1,             TUNING,  "k_conv_x3: 0 keeps the stride-2 layers on the fp32 implicit GEMM") \
    X(IGX3_NW,           "FFGPU_IGX3_NW",           INT,  0,             TUNING,  "k_conv_x3: waves per workgroup, 4 or 8 (0: 8 at stride 2, else 4)") \
    X(IGX3_MT,           "FFGPU_IGX3_MT",           INT,  0,             TUNING,  "k_conv_x3: 16-row blocks per wave, 1 / 2 / 4 (0: by shape; frozen with a plan: ConvDesc::x3_mt)") \
    X(IGX3_MT4_WGS,      "FFGPU_IGX3_MT4_WGS",      INT,  192,           TUNING,  "k_conv_x3: fewest workgroups that four blocks per wave must leave") \
    X(IGX3_MIN_IC,       "FFGPU_IGX3_MIN_IC",       INT,  16,            TUNING,  "k_conv_x3: fewest input channels AUTO takes it for") \
    X(IGX3_MIN_WGS,      "FFGPU_IGX3_MIN_WGS",      INT,  160,           TUNING,  "k_conv_x3: fewest workgroups AUTO takes it for") \
    X(PWG_MIN_OC,        "FFGPU_PWG_MIN_OC",        INT,  128,           TUNING,  "k_pw_gemm32: fewest output channels AUTO takes it for") \
    X(PWG_MIN_IC,        "FFGPU_PWG_MIN_IC",        INT,  64,            TUNING,  "k_pw_gemm32: fewest input channels") \
    X(NO_PW_GEMM,        "FFGPU_NO_PW_GEMM",        INT,  0,             PRODUCT, "never pick k_pw_gemm32: k_pw_mfma instead") \
    X(NO_IGEMM,          "FFGPU_NO_IGEMM",          INT,  0,             TUNING,  "never pick the implicit GEMMs (k_conv_igemm, the dense form of k_conv_x3)") \
    X(NO_GROUP_THIN,     "FFGPU_NO_GROUP_THIN",     INT,  0,             TUNING,  "never pick k_conv_thin for grouped layers of few channels per group") \
    X(NO_DW_PAIR,        "FFGPU_NO_DW_PAIR",        INT,  0,             PRODUCT, "depthwise layers on k_dw_lds instead of k_dw_pair") \
    X(NO_CONV_FIRST,     "FFGPU_NO_CONV_FIRST",     INT,  0,             PRODUCT, "the first layer on the dense small-channel kernel instead of k_conv_first") \
    X(CONV_FIRST_MIN_PX, "FFGPU_CONV_FIRST_MIN_PX", INT,  262144,        TUNING,  "k_conv_first: fewest output pixels of the batch") \
    X(NO_POOL2X2,        "FFGPU_NO_POOL2X2",        INT,  0,             TEST,    "2x2 / stride 2 max pooling on the general pool kernel") \
    /* ---- launch shapes of the convolution kernels */ \
    X(IGEMM_NOVEC,       "FFGPU_IGEMM_NOVEC",       INT,  0,             TUNING,  "k_conv_igemm: no vector form of the gather") \
    X(IGEMM_SPLIT,       "FFGPU_IGEMM_SPLIT",       INT,  0,             TUNING,  "k_conv_igemm: split-K factor 1 .. 16 (0: by tile count; frozen with a plan: ConvDesc::nsplit)") \
    X(DW_U,              "FFGPU_DW_U",              INT,  4,             TUNING,  "k_dw3_stream: rows per step, 1 / 2 / 4") \
    X(DW_BAND,           "FFGPU_DW_BAND",           INT,  4,             TUNING,  "k_dw3_stream: rows per wave task (0: enough tasks to fill the chip)") \
    X(DW_NT,             "FFGPU_DW_NT",             INT,  -1,            PRODUCT, "k_dw3_stream: stream past the caches never (0) / always (1); -1: outputs of 128 MB and more") \
    X(DW_XCD,            "FFGPU_DW_XCD",            INT,  0,             TUNING,  "k_dw3_stream: walk the tasks XCD by XCD") \
    X(DWP_NI,            "FFGPU_DWP_NI",            INT,  0,             TUNING,  "k_dw_pair: frames per workgroup, at most (0: by shape)") \
    X(DWL_BH,            "FFGPU_DWL_BH",            INT,  0,             TUNING,  "k_dw_lds: rows per band (0: by shape)") \
    X(DWL_NPL,           "FFGPU_DWL_NPL",           INT,  0,             TUNING,  "k_dw_lds: planes per item (0: by shape)") \
    X(PWG_WM,            "FFGPU_PWG_WM",            INT,  0,             TUNING,  "k_pw_gemm32: waves per workgroup, 4 or 8 (0: 8 from 248 output channels; part of the packed image)") \
    X(PWG_NARROW,        "FFGPU_PWG_NARROW",        INT,  1,             TUNING,  "k_pw_gemm32: 0 switches the narrow tiles of the partial last round off") \
    X(PWG_DBG,           "FFGPU_PWG_DBG",           INT,  0,             LAB,     "k_pw_gemm32: ablation mask handed to the kernel (wrong results)") \
    /* ---- fused blocks: what ffgpu_irb_plan decides (frozen in IrbDesc::plan), then the launch's diagnostics */ \
    X(NO_THIN,           "FFGPU_NO_THIN",           INT,  0,             PRODUCT, "8-channel blocks on the wave kernel instead of k_irb_thin") \
    X(THIN_BAND,         "FFGPU_THIN_BAND",         INT,  KNOB_COMPUTED, TUNING,  "k_irb_thin: rows per wave; default by batch and height (thin_band)") \
    X(THIN_PAIR,         "FFGPU_THIN_PAIR",         INT,  1,             TUNING,  "k_irb_thin: 0 keeps FFGPU_CONCURRENT executors off the paired form (two frames per wave, 3 / 4 / 5 columns per lane); read at launch") \
    X(THIN_S2,           "FFGPU_THIN_S2",           INT,  1,             TUNING,  "k_irb_thin_s2: 0 keeps FFGPU_CONCURRENT executors off the streaming form of the stride-2 block 4 -> 24 -> 8 (the planned wave kernel instead); read at launch") \
    X(THIN_S2_BAND,      "FFGPU_THIN_S2_BAND",      INT,  0,             TUNING,  "k_irb_thin_s2: output rows per wave (0: by batch and height, thin_s2_form); read at launch") \
    X(SPARSE_HEAD,       "FFGPU_SPARSE_HEAD",       INT,  1,             TUNING,  "k_conv_x3: 0 keeps FFGPU_CONCURRENT executors off the sparse form of the pointwise layer in front of a yolo head (a box pass over all pixels, then the class rows of the quads whose objectness can pass; the dense launch instead); read when an executor is created") \
    X(FRONT_BAND,        "FFGPU_FRONT_BAND",       INT,  KNOB_COMPUTED, TUNING,  "k_front: rows per wave; default as FFGPU_THIN_BAND") \
    X(NO_FRONT,          "FFGPU_NO_FRONT",          INT,  0,             PRODUCT, "layers 0-3 as k_conv_first + k_irb_thin instead of k_front") \
    X(FRONT_MIN_PX,      "FFGPU_FRONT_MIN_PX",      INT,  262144,        TUNING,  "k_front: fewest output pixels of the batch") \
    X(FRONT_NC,          "FFGPU_FRONT_NC",          INT,  3,             PRODUCT, "k_front: output columns per lane, 3 where a row fits a wave that way, or 4") \
    X(NO_IRBW,           "FFGPU_NO_IRBW",           INT,  0,             PRODUCT, "fused blocks on the workgroup kernel k_irb instead of the wave-autonomous k_irbw") \
    X(IRBW_S2_633,       "FFGPU_IRBW_S2_633",       INT,  1,             TUNING,  "k_irbw: 0 hides the stride-2 form for 24 input / 48 output channels from the planner") \
    X(IRBW_S2_NSI4,      "FFGPU_IRBW_S2_NSI4",      INT,  0,             TUNING,  "k_irbw: 1 lets the planner take the four-strip halo for the thin stride-2 blocks") \
    X(IRBW_TWQ,          "FFGPU_IRBW_TWQ",          INT,  0,             TUNING,  "k_irbw: tile width in quads (with FFGPU_IRBW_TH; 0: searched)") \
    X(IRBW_TH,           "FFGPU_IRBW_TH",           INT,  0,             TUNING,  "k_irbw: tile height (with FFGPU_IRBW_TWQ; 0: searched)") \
    X(IRBW_BIG,          "FFGPU_IRBW_BIG",          INT,  -1,            TUNING,  "k_irbw: the 256-register form never (0) / always (1); -1: by register need") \
    X(IRBW_BIG_S2K1,     "FFGPU_IRBW_BIG_S2K1",     INT,  -1,            TUNING,  "k_irbw: as FFGPU_IRBW_BIG for the stride-2 blocks of at most 4 input channels alone") \
    X(IRBW_GWAVES,       "FFGPU_IRBW_GWAVES",       INT,  KNOB_COMPUTED, TUNING,  "k_irbw: waves a launch wants before the group split stops; default 1200, 500 with FFGPU_CONCURRENT") \
    X(IRBW_NOEXC,        "FFGPU_IRBW_NOEXC",        INT,  0,             TUNING,  "k_irbw: without the measured exception (four waves on the 20x20 blocks)") \
    X(IRBW_G_MID,        "FFGPU_IRBW_G_MID",        INT,  0,             TUNING,  "k_irbw: group split for 256 .. 1099 tiles (0: as computed)") \
    X(IRBW_X3,           "FFGPU_IRBW_X3",           INT,  30,            PRODUCT, "fused blocks: expand GEMM as split-bf16 products, one bit per shape: 0: 8 input channels, 1: 16, 2: 24, 3: 48 (split tile in LDS), 4: the 40 -> 20 stride-2 block") \
    X(IRBW_G_XL,         "FFGPU_IRBW_G_XL",         INT,  7,             TUNING,  "k_irbw: group split of the LDS-resident form with several chains in flight") \
    X(IRBW_G_SMALL,      "FFGPU_IRBW_G_SMALL",      INT,  0,             TUNING,  "k_irbw: group split under 256 tiles (0: as computed)") \
    X(IRBW_G,            "FFGPU_IRBW_G",            INT,  0,             TUNING,  "k_irbw: group split, wins over everything (0: as computed)") \
    X(IRBW_NSO,          "FFGPU_IRBW_NSO",          INT,  2,             TUNING,  "k_irbw2: anything but 2 keeps the planner off the two-strip kernel") \
    X(IRBW2_TWQ,         "FFGPU_IRBW2_TWQ",         INT,  0,             TUNING,  "k_irbw2: tile width in quads (with FFGPU_IRBW2_TH; 0: searched)") \
    X(IRBW2_TH,          "FFGPU_IRBW2_TH",          INT,  0,             TUNING,  "k_irbw2: tile height (with FFGPU_IRBW2_TWQ; 0: searched)") \
    X(IRBW2_MIN_TILES,   "FFGPU_IRBW2_MIN_TILES",   INT,  768,           TUNING,  "k_irbw2: fewest tiles the planner takes it for") \
    X(IRBW_WPB,          "FFGPU_IRBW_WPB",          INT,  0,             TUNING,  "k_irbw: tiles per workgroup without a group split, 1 .. 8 (0: 4 or 8 by LDS)") \
    X(IRBW_HALF,         "FFGPU_IRBW_HALF",         INT,  1,             PRODUCT, "0: a last group of at most 8 real expanded channels is computed as a whole group") \
    X(IRBW_XCD,          "FFGPU_IRBW_XCD",          INT,  3,             PRODUCT, "fused blocks walk their tiles XCD by XCD; bit 0: one-wave-per-tile launches, bit 1: group-split launches") \
    X(IRBW_FOLD,         "FFGPU_IRBW_FOLD",         INT,  0,             TUNING,  "k_irbw: never widen the reduction region to all G partial sums (folding rounds)") \
    X(IRB_ECH,           "FFGPU_IRB_ECH",           INT,  0,             TUNING,  "k_irb: expanded channels per chunk, 16 or 32 (0: by shape)") \
    X(IRB_RESIDENT,      "FFGPU_IRB_RESIDENT",      INT,  1,             TUNING,  "k_irb: every chunk's constants in LDS never (0) / where it costs no workgroup (1) / wherever they fit (2)") \
    X(IRB_TW,            "FFGPU_IRB_TW",            INT,  0,             TUNING,  "k_irb: tile width (0: the measured table, then the search)") \
    X(IRB_TH,            "FFGPU_IRB_TH",            INT,  0,             TUNING,  "k_irb: tile height for the search (0: any)") \
    X(IRB_NF,            "FFGPU_IRB_NF",            INT,  0,             TUNING,  "k_irb: frames per tile for the search, 1 / 2 / 4 (0: any)") \
    X(IRB_NOTABLE,       "FFGPU_IRB_NOTABLE",       INT,  0,             TUNING,  "k_irb: skip the measured table of tiles, search") \
    X(IRB_NW,            "FFGPU_IRB_NW",            INT,  8,             TUNING,  "k_irb: waves per workgroup, 8 or 4") \
    X(IRB_NOKS,          "FFGPU_IRB_NOKS",          INT,  0,             TUNING,  "k_irb: idle waves take no slices of the channel loop") \
    X(IRB_SKIP,          "FFGPU_IRB_SKIP",          INT,  0,             LAB,     "k_irb: ablation mask, 1 no input loads, 2 no expand, 4 no depthwise / project, 8 no stores (wrong results)") \
    X(IRB_TRACE,         "FFGPU_IRB_TRACE",         INT,  0,             LAB,     "lab builds with -DIRB_TRACE=1: every fused-block launch is followed by its in-kernel timeline on stderr") \
    X(VERBOSE_IRB,       "FFGPU_VERBOSE_IRB",       INT,  0,             LAB,     "print the plan line of every fused-block launch to stderr")

// what only a lab build has: not a byte of it in the product library (tests/test_cabi_exports.py)
#ifdef FFGPU_DIAG
#define FFGPU_KNOBS_DIAG(X) \
    X(DBG_SKIP,          "FFGPU_DBG_SKIP",          TEXT, 0,             LAB,     "make DIAG=1: \"lo:hi\" drops the launches of layers lo .. hi (wrong results)") \
    X(DBG_KEEP,          "FFGPU_DBG_KEEP",          TEXT, 0,             LAB,     "make DIAG=1: \"lo:hi\" drops every launch but those of layers lo .. hi (wrong results)")
#else
#define FFGPU_KNOBS_DIAG(X)
#endif
#if defined(XT_TRACE) && XT_TRACE
#define FFGPU_KNOBS_XT(X) \
    X(PWXT_TRACE,        "FFGPU_PWXT_TRACE",        TEXT, 0,             LAB,     "builds with -DXT_TRACE=1: file that one traced k_pw_x3t launch dumps its per-tile timeline to")
#else
#define FFGPU_KNOBS_XT(X)
#endif
#define FFGPU_KNOBS(X) FFGPU_KNOBS_MAIN(X) FFGPU_KNOBS_DIAG(X) FFGPU_KNOBS_XT(X)

struct KnobRow { const char *name; KnobKind kind; int dflt; KnobClass cls; const char *text; };
#define X(id, name, kind, dflt, cls, text) K_##id,
enum Knob { FFGPU_KNOBS(X) K_COUNT, K_NONE = -1 };
#undef X
#define X(id, name, kind, dflt, cls, text) { name, KNOB_##kind, dflt, KNOB_##cls, text },
static constexpr KnobRow ffgpu_knob_rows[K_COUNT] = { FFGPU_KNOBS(X) };
#undef X

// ---- the accessors: one parser per kind
static inline int knob_int_(const KnobRow &r, int dflt) { const char *v = getenv(r.name); return v && *v ? atoi(v) : dflt; }
// an INT knob with its table default, or an ON knob (0 / 1)
static inline int knob(Knob k)
{
    const KnobRow &r = ffgpu_knob_rows[k];
    assert((r.kind == KNOB_INT && r.dflt != KNOB_COMPUTED) || r.kind == KNOB_ON);
    if (r.kind == KNOB_INT) return knob_int_(r, r.dflt);
    const char *v = getenv(r.name);
    return v && atoi(v) != 0;
}
// an INT knob whose default the caller computes
static inline int knob_or(Knob k, int dflt)
{
    const KnobRow &r = ffgpu_knob_rows[k];
    assert(r.kind == KNOB_INT && r.dflt == KNOB_COMPUTED);
    return knob_int_(r, dflt);
}
static inline bool knob_set(Knob k) { assert(ffgpu_knob_rows[k].kind == KNOB_SET); return getenv(ffgpu_knob_rows[k].name) != nullptr; }
static inline const char *knob_text(Knob k) { assert(ffgpu_knob_rows[k].kind == KNOB_TEXT); return getenv(ffgpu_knob_rows[k].name); }

// One line per row (ffgpu_knobs_text): name, kind, default or "computed", class, the value a read returns now -- TEXT: set / unset; a computed
// default: the number in the environment, or "default" -- and the row's text.  Returns the length the whole table needs, as snprintf does.
static inline int ffgpu_knobs_lines(char *buf, size_t cap)
{
    static const char *const kinds[] = { "INT", "ON", "SET", "TEXT" }, *const classes[] = { "product", "tuning", "test", "lab" };
    size_t n = 0;
    if (cap) buf[0] = 0;
    for (int k = 0; k < K_COUNT; k++) {
        const KnobRow &r = ffgpu_knob_rows[k];
        const char *const env = getenv(r.name);
        char dflt[16] = "-", val[16];
        if (r.kind == KNOB_INT && r.dflt == KNOB_COMPUTED) snprintf(dflt, sizeof dflt, "computed");
        else if (r.kind != KNOB_TEXT) snprintf(dflt, sizeof dflt, "%d", r.dflt);
        if (r.kind == KNOB_TEXT) snprintf(val, sizeof val, env ? "set" : "unset");
        else if (r.kind == KNOB_SET) snprintf(val, sizeof val, "%d", (int)knob_set((Knob)k));
        else if (r.kind == KNOB_INT && r.dflt == KNOB_COMPUTED && !(env && *env)) snprintf(val, sizeof val, "default");
        else snprintf(val, sizeof val, "%d", r.kind == KNOB_INT && r.dflt == KNOB_COMPUTED ? knob_or((Knob)k, 0) : knob((Knob)k));
        n += (size_t)snprintf(n < cap ? buf + n : nullptr, n < cap ? cap - n : 0, "%s %s %s %s %s %s\n", r.name, kinds[r.kind], dflt, classes[r.cls], val, r.text);
    }
    return (int)n;
}
