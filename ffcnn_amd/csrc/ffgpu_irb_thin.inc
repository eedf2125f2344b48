// ffgpu_irb_thin.inc -- the THIN inverted-residual blocks of yolo-fastest (8 expanded channels at 160x160:
// layers 1-3 and 4-8) as one streaming kernel, no LDS, no MFMA.
//
//     1x1 expand (IC -> EC, act1) -> depthwise 3x3 s1 p1 (actd) -> 1x1 project (EC -> OC, act2) [+ residual]
//
// With so few channels the three layers are pure bandwidth (48 B of traffic per pixel once fused, 160 B as
// three kernels) and the matrix cores would run 50-75 % empty, so this kernel is the streaming design of
// ffgpu_dw_stream.inc with the two pointwise layers folded in:
//   * a wave owns a frame's row segment: lane -> 4 columns; it walks DOWN a band of rows;
//   * per new input row: IC 16-byte loads, the expand is IC*EC*4 VALU FMAs per lane (taps are wave-uniform
//     scalars), the result is zeroed outside the image (the depthwise layer pads the EXPANDED tensor);
//   * an expanded row is never stored: channel by channel it is folded at once into the depthwise sums of the THREE
//     output rows it touches -- the row above gets its last tap row (and is then scaled, activated and projected), the
//     row itself its middle one, the row below its first -- which is the reference's tap order per output (w0..w8) and
//     leaves two partial rows (2 x EC x 4 px) in registers instead of three expanded ones; +-1 column taps come from the
//     neighbour lanes by DPP wave shifts, once per expanded value;
//   * projection + shortcut happen in registers; one 16-byte store per output channel;
//   * the 200-odd filter taps / scales sit in LDS (staged once per workgroup) and are read as broadcast 16-byte
//     ds_reads: as global loads (the compiler cannot keep that many in SGPRs, and cannot prove the output does not alias
//     them) every channel of every row waited for an L2 round trip -- the kernel ran at a third of its ALU time;
//   * the input row of the NEXT step is in flight while this step's depthwise / projection work runs.
// The PAIRED form (k_irb_thin_pair) puts a row of TWO frames side by side in the wave: NC = 3, 4 or 5 columns per lane, at most 32
// lanes per row; lanes 0-31 walk frame 2m, lanes 32-63 frame 2m + 1, on the same band and row index, so that everything wave-uniform
// stays wave-uniform and a 160-pixel row (5 columns, 32 lanes) leaves no lane idle.  Per output the arithmetic is the single form's,
// operation for operation; only the lane that holds a pixel changes.  Both kernels are ffgpu_irb_thin_body.inc.
// Restates conv-v6.c:46-91 / 96-229 / 46-91 and ffcnn.c:418-423 (same tap order per layer).
struct ThinP {
    const float *in; float *out; const float *residual;
    const float *w1, *wd, *w2;       // filter rows (conv.h layout): w1 [EC][k4+4], wd [EC][16], w2 [OC][EC4+4]
    int W, H, N;                     // plane geometry (W % 4 == 0, W/4 <= 64), frames
    int band, nbands;
    float act1, actd, act2, res_act; // slopes: act(x) = max(x, slope x)
    long ntasks;                     // N * nbands (the paired form: ceil(N / 2) * nbands)
};

typedef float v2f_t __attribute__((ext_vector_type(2)));

// one frame per wave, four columns per lane
template <int IC, int EC, int OC>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) k_irb_thin(ThinP p)
{
    constexpr int NC = 4 + 0 * IC;                  // (value-dependent, so that the other forms' branches are discarded, not checked)
    constexpr bool PAIR = IC < 0;
#include "ffgpu_irb_thin_body.inc"
}

// two frames per wave, NC columns per lane (W % NC == 0, W / NC <= 32); ntasks = ceil(N / 2) * nbands
template <int IC, int EC, int OC, int NC>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) k_irb_thin_pair(ThinP p)
{
    constexpr bool PAIR = NC > 0;
#include "ffgpu_irb_thin_body.inc"
}
