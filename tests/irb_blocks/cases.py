"""The table of fused-block test cases: at least two per instantiation key (ffgpu_irb_instantiations), found by a search with the host-only planner probe
(ffgpu_irb_plan_text).  tests/test_irb_blocks_ref.py holds the table to its purpose without a GPU -- every case plans onto its declared key, the keys are
exactly the library's list, the structural conditions below hold in the plan lines, and the fp32 reference chain meets the error criterion against
float64 -- and tests/irb_blocks/test_gpu_kernels.py runs every case on the device.

  tiny    the smallest block that reaches the key: batch <= 2, plane <= 24 x 24
  tiled   N = 2 or 3, plane <= 48 x 48, at least two tiles in x and in y with a ragged last tile in both, at least three 16-channel groups with a ragged
          last one, a ragged oc, a residual on every other case (thin blocks have 8 expanded channels and one row per wave: bands take the place of tiles)
  act     one tiled case per family under (1,1,0,0), (1,2,2,1), (0,2,1,2) and (2,1,0,2), with a residual
  relu    one tiled case per family with act1 = actd = relu and res_act = linear, then relu: a NaN, a +Inf and a -Inf planted in the input, bias' = -Inf
          on one expanded channel, zero weights on the +Inf channel (plant())

A shape is (N, W, H, ic, ec, oc, stride); acts is (act1, actd, act2, res_act) in the numbering of utils.h (0 linear, 1 relu, 2 leaky); env holds the
planner switches the case runs under -- every other planner switch is unset (test_irb_choice.knob_names: the library's own table)."""
import collections
import functools

import numpy as np

from irb_blocks import blockref

Case = collections.namedtuple("Case", "id key kind shape acts res env")
DEFAULT_ACTS = (2, 2, 0, 0)

# (key, kind, shape, residual, switches)
TABLE = [
    ("thin<8,8,4>", "tiny", (2, 16, 12, 8, 8, 4, 1), False, {}),
    ("thin<8,8,4>", "tiled", (2, 12, 11, 8, 8, 4, 1), True, {}),
    ("thin<4,8,4>", "tiny", (2, 16, 12, 4, 8, 4, 1), True, {}),
    ("thin<4,8,4>", "tiled", (2, 12, 11, 4, 8, 4, 1), False, {}),
    ("thin<8,8,8>", "tiny", (2, 16, 12, 8, 8, 8, 1), False, {}),
    ("thin<8,8,8>", "tiled", (2, 12, 11, 8, 8, 8, 1), True, {}),
    ("thin<4,8,8>", "tiny", (2, 16, 12, 4, 8, 8, 1), True, {}),
    ("thin<4,8,8>", "tiled", (2, 12, 11, 4, 8, 8, 1), False, {}),
    ("irbw2<2,3,x3>", "tiny", (1, 9, 7, 7, 8, 4, 1), False, {"FFGPU_IRBW2_MIN_TILES": "1", "FFGPU_IRBW_G": "1", "FFGPU_IRBW_X3": "31"}),
    ("irbw2<2,3,x3>", "tiled", (2, 23, 19, 7, 37, 13, 1), True, {"FFGPU_IRBW2_MIN_TILES": "1", "FFGPU_IRBW_G": "1", "FFGPU_IRBW_X3": "31"}),
    ("irbw2<4,3,x3>", "tiny", (1, 9, 7, 13, 8, 4, 1), True, {"FFGPU_IRBW2_MIN_TILES": "1", "FFGPU_IRBW_G": "1"}),
    ("irbw2<4,3,x3>", "tiled", (2, 23, 19, 13, 37, 13, 1), False, {"FFGPU_IRBW2_MIN_TILES": "1", "FFGPU_IRBW_G": "1"}),
    ("irbw2<2,3>", "tiny", (1, 9, 7, 7, 8, 4, 1), False, {"FFGPU_IRBW2_MIN_TILES": "1", "FFGPU_IRBW_G": "1"}),
    ("irbw2<2,3>", "tiled", (2, 23, 19, 7, 37, 13, 1), True, {"FFGPU_IRBW2_MIN_TILES": "1", "FFGPU_IRBW_G": "1"}),
    ("irbw2<4,3>", "tiny", (1, 9, 7, 13, 8, 4, 1), True, {"FFGPU_IRBW2_MIN_TILES": "1", "FFGPU_IRBW_G": "1", "FFGPU_IRBW_X3": "0"}),
    ("irbw2<4,3>", "tiled", (2, 23, 19, 13, 37, 13, 1), False, {"FFGPU_IRBW2_MIN_TILES": "1", "FFGPU_IRBW_G": "1", "FFGPU_IRBW_X3": "0"}),
    ("irbw<12,3,1,2,big,x3,xl>", "tiny", (1, 9, 7, 45, 20, 40, 1), False, {}),
    ("irbw<12,3,1,2,big,x3,xl>", "tiled", (2, 23, 19, 45, 43, 43, 1), True, {}),
    ("irbw<4,2,2,4,big,x3>", "tiny", (1, 9, 7, 13, 8, 24, 2), True, {}),
    ("irbw<4,2,2,4,big,x3>", "tiled", (3, 21, 17, 13, 37, 27, 2), False, {"FFGPU_IRBW_TWQ": "2", "FFGPU_IRBW_TH": "4", "FFGPU_IRBW_G": "1"}),
    ("irbw<6,2,1,2,big,x3>", "tiny", (1, 9, 7, 21, 8, 24, 1), False, {}),
    ("irbw<6,2,1,2,big,x3>", "tiled", (2, 23, 19, 21, 43, 27, 1), True, {}),
    ("irbw<1,1,1,2,big>", "tiny", (1, 9, 7, 3, 8, 4, 1), True, {"FFGPU_IRBW_BIG": "1"}),
    ("irbw<1,1,1,2,big>", "tiled", (2, 23, 19, 3, 37, 13, 1), False, {"FFGPU_IRBW_G": "3", "FFGPU_IRBW_FOLD": "1", "FFGPU_IRBW_BIG": "1"}),
    ("irbw<1,1,1,2>", "tiny", (1, 9, 7, 3, 8, 4, 1), False, {}),
    ("irbw<1,1,1,2>", "tiled", (3, 30, 26, 3, 43, 13, 1), True, {"FFGPU_IRBW_G": "1"}),
    ("irbw<2,1,1,2,big>", "tiny", (1, 9, 7, 7, 8, 4, 1), True, {"FFGPU_IRBW_BIG": "1"}),
    ("irbw<2,1,1,2,big>", "tiled", (2, 23, 19, 7, 37, 13, 1), False, {"FFGPU_IRBW_BIG": "1"}),
    ("irbw<2,1,1,2>", "tiny", (1, 9, 7, 7, 8, 4, 1), False, {}),
    ("irbw<2,1,1,2>", "tiled", (2, 23, 19, 7, 43, 13, 1), True, {"FFGPU_IRBW_G": "3", "FFGPU_IRBW_FOLD": "1"}),
    ("irbw<4,1,1,2,big>", "tiny", (1, 9, 7, 13, 8, 4, 1), True, {}),
    ("irbw<4,1,1,2,big>", "tiled", (3, 30, 26, 13, 37, 13, 1), False, {"FFGPU_IRBW_G": "1"}),
    ("irbw<4,1,1,2>", "tiny", (1, 9, 7, 13, 8, 4, 1), False, {"FFGPU_IRBW_BIG": "0"}),
    ("irbw<4,1,1,2>", "tiled", (2, 23, 19, 13, 43, 13, 1), True, {"FFGPU_IRBW_BIG": "0"}),
    ("irbw<2,2,1,2,big>", "tiny", (1, 9, 7, 7, 8, 24, 1), True, {}),
    ("irbw<2,2,1,2,big>", "tiled", (2, 23, 19, 7, 37, 27, 1), False, {"FFGPU_IRBW_G": "3", "FFGPU_IRBW_FOLD": "1"}),
    ("irbw<2,2,1,2>", "tiny", (1, 9, 7, 7, 8, 24, 1), False, {"FFGPU_IRBW_BIG": "0"}),
    ("irbw<2,2,1,2>", "tiled", (3, 30, 26, 7, 43, 27, 1), True, {"FFGPU_IRBW_G": "1", "FFGPU_IRBW_BIG": "0"}),
    ("irbw<4,2,1,2,big>", "tiny", (1, 9, 7, 13, 8, 24, 1), True, {}),
    ("irbw<4,2,1,2,big>", "tiled", (2, 23, 19, 13, 37, 27, 1), False, {}),
    ("irbw<4,2,1,2>", "tiny", (1, 9, 7, 13, 8, 24, 1), False, {"FFGPU_IRBW_BIG": "0"}),
    ("irbw<4,2,1,2>", "tiled", (2, 23, 19, 13, 43, 27, 1), True, {"FFGPU_IRBW_G": "3", "FFGPU_IRBW_FOLD": "1", "FFGPU_IRBW_BIG": "0"}),
    ("irbw<6,2,1,2,big>", "tiny", (1, 9, 7, 21, 8, 24, 1), True, {"FFGPU_IRBW_X3": "0"}),
    ("irbw<6,2,1,2,big>", "tiled", (3, 30, 26, 21, 37, 27, 1), False, {"FFGPU_IRBW_G": "1", "FFGPU_IRBW_X3": "0"}),
    ("irbw<6,2,1,2>", "tiny", (1, 9, 7, 21, 8, 24, 1), False, {"FFGPU_IRBW_BIG": "0"}),
    ("irbw<6,2,1,2>", "tiled", (2, 23, 19, 21, 43, 27, 1), True, {"FFGPU_IRBW_BIG": "0"}),
    ("irbw<12,3,1,2,big>", "tiny", (1, 9, 7, 45, 8, 40, 1), True, {}),
    ("irbw<12,3,1,2,big>", "tiled", (2, 23, 19, 45, 37, 43, 1), False, {"FFGPU_IRBW_G": "3", "FFGPU_IRBW_FOLD": "1", "FFGPU_IRBW_X3": "0"}),
    ("irbw<12,3,1,2>", "tiny", (1, 9, 7, 45, 8, 40, 1), False, {"FFGPU_IRBW_BIG": "0"}),
    ("irbw<12,3,1,2>", "tiled", (3, 30, 26, 45, 43, 43, 1), True, {"FFGPU_IRBW_G": "1", "FFGPU_IRBW_BIG": "0"}),
    ("irbw<1,1,2,3,big>", "tiny", (1, 9, 7, 3, 8, 4, 2), True, {"FFGPU_IRBW_BIG": "1"}),
    ("irbw<1,1,2,3,big>", "tiled", (2, 22, 13, 3, 37, 13, 2), False, {"FFGPU_IRBW_TWQ": "2", "FFGPU_IRBW_TH": "4", "FFGPU_IRBW_BIG": "1"}),
    ("irbw<1,1,2,3>", "tiny", (1, 9, 7, 3, 8, 4, 2), False, {}),
    ("irbw<1,1,2,3>", "tiled", (2, 22, 13, 3, 43, 13, 2), True, {"FFGPU_IRBW_TWQ": "2", "FFGPU_IRBW_TH": "4", "FFGPU_IRBW_G": "3", "FFGPU_IRBW_FOLD": "1"}),
    ("irbw<2,1,2,3,big>", "tiny", (1, 9, 7, 7, 8, 4, 2), True, {}),
    ("irbw<2,1,2,3,big>", "tiled", (3, 21, 17, 7, 37, 13, 2), False, {"FFGPU_IRBW_TWQ": "2", "FFGPU_IRBW_TH": "4", "FFGPU_IRBW_G": "1"}),
    ("irbw<2,1,2,3>", "tiny", (1, 9, 7, 7, 8, 4, 2), False, {"FFGPU_IRBW_BIG": "0"}),
    ("irbw<2,1,2,3>", "tiled", (2, 22, 13, 7, 43, 13, 2), True, {"FFGPU_IRBW_TWQ": "2", "FFGPU_IRBW_TH": "4", "FFGPU_IRBW_BIG": "0"}),
    ("irbw<4,2,2,4,big>", "tiny", (1, 9, 7, 13, 8, 24, 2), True, {"FFGPU_IRBW_X3": "0"}),
    ("irbw<4,2,2,4,big>", "tiled", (2, 22, 13, 13, 37, 27, 2), False, {"FFGPU_IRBW_TWQ": "2", "FFGPU_IRBW_TH": "4", "FFGPU_IRBW_G": "3", "FFGPU_IRBW_FOLD": "1", "FFGPU_IRBW_X3": "0"}),
    ("irbw<4,2,2,4>", "tiny", (1, 9, 7, 13, 8, 24, 2), False, {"FFGPU_IRBW_BIG": "0"}),
    ("irbw<4,2,2,4>", "tiled", (3, 21, 17, 13, 43, 27, 2), True, {"FFGPU_IRBW_TWQ": "2", "FFGPU_IRBW_TH": "4", "FFGPU_IRBW_G": "1", "FFGPU_IRBW_BIG": "0"}),
    ("irbw<6,3,2,3,big>", "tiny", (1, 9, 7, 21, 8, 40, 2), True, {}),
    ("irbw<6,3,2,3,big>", "tiled", (2, 22, 13, 21, 37, 43, 2), False, {"FFGPU_IRBW_TWQ": "2", "FFGPU_IRBW_TH": "4"}),
    ("irbw<6,3,2,3>", "tiny", (1, 9, 7, 21, 8, 40, 2), False, {"FFGPU_IRBW_BIG": "0"}),
    ("irbw<6,3,2,3>", "tiled", (2, 22, 13, 21, 43, 43, 2), True, {"FFGPU_IRBW_TWQ": "2", "FFGPU_IRBW_TH": "4", "FFGPU_IRBW_G": "3", "FFGPU_IRBW_FOLD": "1", "FFGPU_IRBW_BIG": "0"}),
    ("irbw<1,1,2,4,big>", "tiny", (2, 22, 13, 3, 8, 4, 2), True, {"FFGPU_IRBW_S2_NSI4": "1", "FFGPU_IRBW_BIG": "1"}),
    ("irbw<1,1,2,4,big>", "tiled", (2, 45, 41, 3, 37, 13, 2), False, {"FFGPU_IRBW_S2_NSI4": "1", "FFGPU_IRBW_BIG": "1"}),
    ("irbw<1,1,2,4>", "tiny", (2, 22, 13, 3, 8, 4, 2), False, {"FFGPU_IRBW_S2_NSI4": "1"}),
    ("irbw<1,1,2,4>", "tiled", (2, 45, 41, 3, 43, 13, 2), True, {"FFGPU_IRBW_S2_NSI4": "1"}),
    ("irbw<2,1,2,4,big>", "tiny", (2, 22, 13, 7, 8, 4, 2), True, {"FFGPU_IRBW_S2_NSI4": "1"}),
    ("irbw<2,1,2,4,big>", "tiled", (2, 45, 41, 7, 37, 13, 2), False, {"FFGPU_IRBW_S2_NSI4": "1"}),
    ("irbw<2,1,2,4>", "tiny", (2, 22, 13, 7, 8, 4, 2), False, {"FFGPU_IRBW_S2_NSI4": "1", "FFGPU_IRBW_BIG": "0"}),
    ("irbw<2,1,2,4>", "tiled", (2, 45, 41, 7, 43, 13, 2), True, {"FFGPU_IRBW_S2_NSI4": "1", "FFGPU_IRBW_BIG": "0"}),
    ("irb<1,1,1,1,8>", "tiny", (2, 16, 12, 21, 8, 4, 1), True, {}),
    ("irb<1,1,1,1,8>", "tiled", (2, 22, 14, 3, 37, 13, 1), False, {"FFGPU_NO_IRBW": "1", "FFGPU_NO_THIN": "1", "FFGPU_IRB_NW": "8", "FFGPU_IRB_TW": "8", "FFGPU_IRB_TH": "4", "FFGPU_IRB_RESIDENT": "0", "FFGPU_IRB_ECH": "16"}),
    ("irb<1,1,2,1,8>", "tiny", (2, 16, 12, 13, 8, 4, 2), False, {}),
    ("irb<1,1,2,1,8>", "tiled", (2, 24, 20, 3, 37, 13, 2), True, {"FFGPU_NO_IRBW": "1", "FFGPU_NO_THIN": "1", "FFGPU_IRB_NW": "8", "FFGPU_IRB_TW": "8", "FFGPU_IRB_TH": "4", "FFGPU_IRB_ECH": "16"}),
    ("irb<1,1,1,2,4>", "tiny", (2, 16, 12, 3, 8, 4, 1), True, {"FFGPU_NO_IRBW": "1", "FFGPU_NO_THIN": "1", "FFGPU_IRB_NW": "4"}),
    ("irb<1,1,1,2,4>", "tiled", (2, 36, 34, 3, 37, 13, 1), False, {"FFGPU_NO_IRBW": "1", "FFGPU_NO_THIN": "1", "FFGPU_IRB_NW": "4", "FFGPU_IRB_RESIDENT": "0"}),
    ("irb<1,1,2,2,4>", "tiny", (2, 16, 12, 3, 8, 4, 2), False, {"FFGPU_NO_IRBW": "1", "FFGPU_NO_THIN": "1", "FFGPU_IRB_NW": "4"}),
    ("irb<1,1,2,2,4>", "tiled", (2, 40, 36, 3, 37, 13, 2), True, {"FFGPU_NO_IRBW": "1", "FFGPU_NO_THIN": "1", "FFGPU_IRB_NW": "4", "FFGPU_IRB_TW": "16", "FFGPU_IRB_TH": "8", "FFGPU_IRB_ECH": "16"}),
    ("irb<1,2,1,1,8>", "tiny", (2, 16, 12, 3, 8, 24, 1), True, {}),
    ("irb<1,2,1,1,8>", "tiled", (2, 22, 14, 3, 37, 27, 1), False, {"FFGPU_NO_IRBW": "1", "FFGPU_NO_THIN": "1", "FFGPU_IRB_NW": "8", "FFGPU_IRB_TW": "8", "FFGPU_IRB_TH": "4", "FFGPU_IRB_RESIDENT": "0", "FFGPU_IRB_ECH": "16"}),
    ("irb<1,2,2,1,8>", "tiny", (2, 16, 12, 3, 8, 24, 2), False, {}),
    ("irb<1,2,2,1,8>", "tiled", (2, 24, 20, 3, 37, 27, 2), True, {"FFGPU_NO_IRBW": "1", "FFGPU_NO_THIN": "1", "FFGPU_IRB_NW": "8", "FFGPU_IRB_TW": "8", "FFGPU_IRB_TH": "4", "FFGPU_IRB_ECH": "16"}),
    ("irb<1,2,1,2,4>", "tiny", (2, 16, 12, 3, 8, 24, 1), True, {"FFGPU_NO_IRBW": "1", "FFGPU_NO_THIN": "1", "FFGPU_IRB_NW": "4"}),
    ("irb<1,2,1,2,4>", "tiled", (2, 38, 30, 3, 72, 27, 1), False, {"FFGPU_NO_IRBW": "1", "FFGPU_NO_THIN": "1", "FFGPU_IRB_NW": "4", "FFGPU_IRB_RESIDENT": "0", "FFGPU_IRB_ECH": "16"}),
    ("irb<1,2,2,2,4>", "tiny", (2, 16, 12, 3, 8, 24, 2), False, {"FFGPU_NO_IRBW": "1", "FFGPU_NO_THIN": "1", "FFGPU_IRB_NW": "4"}),
    ("irb<1,2,2,2,4>", "tiled", (2, 24, 20, 3, 37, 27, 2), True, {"FFGPU_NO_IRBW": "1", "FFGPU_NO_THIN": "1", "FFGPU_IRB_NW": "4", "FFGPU_IRB_TW": "8", "FFGPU_IRB_TH": "4", "FFGPU_IRB_ECH": "16"}),
    ("irb<1,3,1,1,8>", "tiny", (2, 16, 12, 3, 8, 40, 1), True, {}),
    ("irb<1,3,1,1,8>", "tiled", (2, 36, 34, 3, 37, 43, 1), False, {"FFGPU_NO_IRBW": "1", "FFGPU_NO_THIN": "1", "FFGPU_IRB_NW": "8", "FFGPU_IRB_RESIDENT": "0"}),
    ("irb<1,3,2,1,8>", "tiny", (2, 16, 12, 3, 8, 40, 2), False, {}),
    ("irb<1,3,2,1,8>", "tiled", (2, 40, 36, 3, 37, 43, 2), True, {"FFGPU_NO_IRBW": "1", "FFGPU_NO_THIN": "1", "FFGPU_IRB_NW": "8", "FFGPU_IRB_TW": "16", "FFGPU_IRB_TH": "8", "FFGPU_IRB_ECH": "16"}),
    ("irb<1,3,1,2,4>", "tiny", (2, 16, 12, 3, 8, 40, 1), True, {"FFGPU_NO_IRBW": "1", "FFGPU_NO_THIN": "1", "FFGPU_IRB_NW": "4"}),
    ("irb<1,3,1,2,4>", "tiled", (2, 22, 14, 3, 37, 43, 1), False, {"FFGPU_NO_IRBW": "1", "FFGPU_NO_THIN": "1", "FFGPU_IRB_NW": "4", "FFGPU_IRB_TW": "8", "FFGPU_IRB_TH": "4", "FFGPU_IRB_RESIDENT": "0", "FFGPU_IRB_ECH": "16"}),
    ("irb<1,3,2,2,4>", "tiny", (2, 16, 12, 3, 8, 40, 2), False, {"FFGPU_NO_IRBW": "1", "FFGPU_NO_THIN": "1", "FFGPU_IRB_NW": "4"}),
    ("irb<1,3,2,2,4>", "tiled", (2, 24, 20, 3, 37, 43, 2), True, {"FFGPU_NO_IRBW": "1", "FFGPU_NO_THIN": "1", "FFGPU_IRB_NW": "4", "FFGPU_IRB_TW": "8", "FFGPU_IRB_TH": "4", "FFGPU_IRB_ECH": "16"}),
    ("irb<2,1,1,1,8>", "tiny", (2, 16, 12, 21, 20, 4, 1), True, {}),
    ("irb<2,1,1,1,8>", "tiled", (2, 22, 14, 3, 72, 13, 1), False, {"FFGPU_NO_IRBW": "1", "FFGPU_NO_THIN": "1", "FFGPU_IRB_NW": "8", "FFGPU_IRB_TW": "8", "FFGPU_IRB_TH": "4", "FFGPU_IRB_RESIDENT": "0"}),
    ("irb<2,1,2,1,8>", "tiny", (2, 16, 12, 13, 20, 4, 2), False, {}),
    ("irb<2,1,2,1,8>", "tiled", (2, 24, 20, 3, 72, 13, 2), True, {"FFGPU_NO_IRBW": "1", "FFGPU_NO_THIN": "1", "FFGPU_IRB_NW": "8", "FFGPU_IRB_TW": "8", "FFGPU_IRB_TH": "4"}),
    ("irb<2,1,1,2,4>", "tiny", (2, 16, 12, 3, 20, 4, 1), True, {"FFGPU_NO_IRBW": "1", "FFGPU_NO_THIN": "1", "FFGPU_IRB_NW": "4"}),
    ("irb<2,1,1,2,4>", "tiled", (2, 36, 34, 3, 37, 13, 1), False, {"FFGPU_NO_IRBW": "1", "FFGPU_NO_THIN": "1", "FFGPU_IRB_NW": "4", "FFGPU_IRB_ECH": "32"}),
    ("irb<2,1,2,2,4>", "tiny", (2, 16, 12, 3, 20, 4, 2), False, {"FFGPU_NO_IRBW": "1", "FFGPU_NO_THIN": "1", "FFGPU_IRB_NW": "4"}),
    ("irb<2,1,2,2,4>", "tiled", (2, 40, 36, 3, 72, 13, 2), True, {"FFGPU_NO_IRBW": "1", "FFGPU_NO_THIN": "1", "FFGPU_IRB_NW": "4", "FFGPU_IRB_TW": "16", "FFGPU_IRB_TH": "8"}),
    ("irb<2,2,1,1,8>", "tiny", (2, 16, 12, 3, 20, 24, 1), True, {}),
    ("irb<2,2,1,1,8>", "tiled", (2, 22, 14, 3, 72, 27, 1), False, {"FFGPU_NO_IRBW": "1", "FFGPU_NO_THIN": "1", "FFGPU_IRB_NW": "8", "FFGPU_IRB_TW": "8", "FFGPU_IRB_TH": "4", "FFGPU_IRB_RESIDENT": "0"}),
    ("irb<2,2,2,1,8>", "tiny", (2, 16, 12, 3, 20, 24, 2), False, {}),
    ("irb<2,2,2,1,8>", "tiled", (2, 24, 20, 3, 72, 27, 2), True, {"FFGPU_NO_IRBW": "1", "FFGPU_NO_THIN": "1", "FFGPU_IRB_NW": "8", "FFGPU_IRB_TW": "8", "FFGPU_IRB_TH": "4"}),
    ("irb<2,2,1,2,4>", "tiny", (2, 16, 12, 3, 20, 24, 1), True, {"FFGPU_NO_IRBW": "1", "FFGPU_NO_THIN": "1", "FFGPU_IRB_NW": "4"}),
    ("irb<2,2,1,2,4>", "tiled", (2, 38, 30, 3, 72, 27, 1), False, {"FFGPU_NO_IRBW": "1", "FFGPU_NO_THIN": "1", "FFGPU_IRB_NW": "4", "FFGPU_IRB_RESIDENT": "0"}),
    ("irb<2,2,2,2,4>", "tiny", (2, 16, 12, 3, 20, 24, 2), False, {"FFGPU_NO_IRBW": "1", "FFGPU_NO_THIN": "1", "FFGPU_IRB_NW": "4"}),
    ("irb<2,2,2,2,4>", "tiled", (2, 24, 20, 3, 72, 27, 2), True, {"FFGPU_NO_IRBW": "1", "FFGPU_NO_THIN": "1", "FFGPU_IRB_NW": "4", "FFGPU_IRB_TW": "8", "FFGPU_IRB_TH": "4"}),
    ("irb<2,3,1,1,8>", "tiny", (2, 16, 12, 3, 20, 40, 1), True, {}),
    ("irb<2,3,1,1,8>", "tiled", (2, 36, 34, 3, 37, 43, 1), False, {"FFGPU_NO_IRBW": "1", "FFGPU_NO_THIN": "1", "FFGPU_IRB_NW": "8", "FFGPU_IRB_ECH": "32"}),
    ("irb<2,3,2,1,8>", "tiny", (2, 16, 12, 3, 20, 40, 2), False, {}),
    ("irb<2,3,2,1,8>", "tiled", (2, 24, 20, 3, 72, 43, 2), True, {"FFGPU_NO_IRBW": "1", "FFGPU_NO_THIN": "1", "FFGPU_IRB_NW": "8", "FFGPU_IRB_TW": "8", "FFGPU_IRB_TH": "4"}),
    ("irb<2,3,1,2,4>", "tiny", (2, 16, 12, 3, 20, 40, 1), True, {"FFGPU_NO_IRBW": "1", "FFGPU_NO_THIN": "1", "FFGPU_IRB_NW": "4"}),
    ("irb<2,3,1,2,4>", "tiled", (2, 22, 14, 3, 72, 43, 1), False, {"FFGPU_NO_IRBW": "1", "FFGPU_NO_THIN": "1", "FFGPU_IRB_NW": "4", "FFGPU_IRB_TW": "8", "FFGPU_IRB_TH": "4", "FFGPU_IRB_RESIDENT": "0"}),
    ("irb<2,3,2,2,4>", "tiny", (2, 16, 12, 3, 20, 40, 2), False, {"FFGPU_NO_IRBW": "1", "FFGPU_NO_THIN": "1", "FFGPU_IRB_NW": "4"}),
    ("irb<2,3,2,2,4>", "tiled", (2, 24, 20, 3, 72, 43, 2), True, {"FFGPU_NO_IRBW": "1", "FFGPU_NO_THIN": "1", "FFGPU_IRB_NW": "4", "FFGPU_IRB_TW": "8", "FFGPU_IRB_TH": "4"}),
]
# the one combination of the workgroup form that no per-key case shows: several frames per tile (NF > 1; whole planes only)
TABLE.append(("irb<1,1,1,1,8>", "tiny-nf", (2, 16, 12, 3, 8, 4, 1), True, {"FFGPU_NO_IRBW": "1", "FFGPU_NO_THIN": "1", "FFGPU_IRB_NOTABLE": "1", "FFGPU_IRB_NF": "2"}))

FAMILIES = {"thin": "thin<8,8,4>", "wave fp32": "irbw<4,2,1,2,big>", "wave x3": "irbw<6,2,1,2,big,x3>", "XL": "irbw<12,3,1,2,big,x3,xl>", "two-strip": "irbw2<4,3,x3>",
            "workgroup, 8 waves": "irb<2,2,1,1,8>", "workgroup, 4 waves": "irb<1,2,2,2,4>"}
ACT_SETS = [(1, 1, 0, 0), (1, 2, 2, 1), (0, 2, 1, 2), (2, 1, 0, 2)]
RELU_SETS = [(1, 1, 0, 0), (1, 1, 0, 1)]


def _cases():
    out = []
    tiled = {}
    for key, kind, shape, res, env in TABLE:
        out.append(Case("%s-%s" % (key, kind), key, kind, shape, DEFAULT_ACTS, res, dict(env)))
        if kind == "tiled":
            tiled[key] = out[-1]
    for fam, key in FAMILIES.items():
        c = tiled[key]
        for acts in ACT_SETS:
            out.append(c._replace(id="%s-act%d%d%d%d" % ((key,) + acts), kind="act", acts=acts, res=True))
        for acts in RELU_SETS:
            out.append(c._replace(id="%s-relu%d%d%d%d" % ((key,) + acts), kind="relu", acts=acts, res=True))
    assert len({c.id for c in out}) == len(out)
    return out


CASES = _cases()
IDS = [c.id for c in CASES]


def family(key):
    if key.startswith("thin<"):
        return "thin"
    if key.startswith("irbw2<"):
        return "two-strip"
    if key.startswith("irb<"):
        return "workgroup, %s waves" % key[:-1].split(",")[-1]
    return "XL" if ",xl" in key else ("wave x3" if ",x3" in key else "wave fp32")


def fields(line):
    """a plan line as a dict: key, and every name=value (a tuple where the value is a comma list)"""
    key, _, rest = line.partition(" ")
    d = {"key": key}
    for tok in rest.split():
        k, v = tok.split("=")
        vals = tuple(float(x) if "." in x or "e" in x else int(x) for x in v.split(","))
        d[k] = vals if len(vals) > 1 else vals[0]
    return d


def set_switches(monkeypatch, case):
    from test_irb_choice import knob_names
    names = knob_names()
    for v in names:
        monkeypatch.delenv(v, raising=False)
    for k, v in case.env.items():
        assert k in names, k
        monkeypatch.setenv(k, v)


def plan_line(probe, case):
    """under set_switches(case)"""
    return probe(tuple(case.shape) + tuple(case.acts))


def plant(case, x, f1, fd, f2):
    """the non-finite values of a relu case, in place.  In the reference (relu(NaN) = relu(-Inf) = 0):
      +Inf at one pixel of input channel 0, whose weights are zero (0 * Inf = NaN -> 0 after relu) except towards expanded channel 0, whose taps are made positive:
            that channel alone is +Inf in the pixel's neighbourhood, and the outputs there are +Inf (channel 0) and -Inf (channel 1) by the sign of w2
      -Inf at one pixel of the last input channel, in the last frame, under the random weights: several expanded channels are +Inf there, the project sums mix them: NaN
      NaN at pixel (0, 0) of a middle channel: every expanded channel is NaN there -> 0
      bias' = -Inf on expanded channel 1: -Inf or NaN before the activation everywhere -> 0 everywhere"""
    N, W, H, ic, ec, oc, stride = case.shape
    xf = x.reshape(ic, N, H, W)
    k4 = (ic + 3) & ~3
    xf[0, 0, H // 2, W // 2] = np.inf
    xf[ic - 1, N - 1, H - 1, W - 2] = -np.inf
    xf[ic // 2, 0, 0, 0] = np.nan
    f1[:, 0] = 0.0
    f1[0, 0] = 0.25
    f1[1, k4 + 1] = -np.inf
    fd[0, :9] = np.abs(fd[0, :9]) + np.float32(0.01)
    f2[0, 0], f2[1, 0] = 0.3, -0.3


@functools.lru_cache(maxsize=None)
def reference(i):
    """inputs and both references of CASES[i], computed once and shared (read only): x, f1, fd, f2, res (None without a residual), y32 (the fp32 chain), y64,
    ok (outputs that are finite in both), E_ref = max |y32 - y64| and ymax = max |y64| over ok"""
    from oracle import orc
    orc.build()
    c = CASES[i]
    x, f1, fd, f2, res = blockref.make_inputs(1000 + i, *c.shape)
    if c.kind == "relu":
        plant(c, x, f1, fd, f2)
    if not c.res:
        res = None
    y32 = blockref.chain32(orc, x, f1, fd, f2, res, *c.shape, c.acts)
    y64 = blockref.block64(x, f1, fd, f2, res, *c.shape, c.acts)
    ok = np.isfinite(y32) & np.isfinite(y64)
    r = dict(x=x, f1=f1, fd=fd, f2=f2, res=res, y32=y32, y64=y64, ok=ok, E_ref=float(np.abs(np.where(ok, y32 - np.where(ok, y64, 0), 0)).max()), ymax=float(np.abs(y64[ok]).max()))
    for a in (x, f1, fd, f2, res, y32, y64, ok):
        if a is not None:
            a.setflags(write=False)
    return r


# A row that passes everything else but exceeds the factor 2 of E_k <= factor * E_ref + 1e-6 gets its measured ratio times 1.5, at most 4, here -- with the
# measured value and the date beside it.  (None so far.)
FACTOR = {}
