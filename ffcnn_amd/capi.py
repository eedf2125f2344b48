"""ctypes mirror of include/ffcnn.h, include/conv.h and include/ffcnn_hip.h."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DATA = os.path.join(ROOT, "data")
CFG = os.path.join(DATA, "yolo-fastest-1.1.cfg")
WEIGHTS = os.path.join(DATA, "yolo-fastest-1.1.weights")

f32p = C.POINTER(C.c_float)


class FFGPU:
    MAX_DET = 128
    MERGE_LDS_SLOTS = 1024               # FFGPU_MERGE_LDS_SLOTS: unions up to this many boxes are merged in LDS (ffgpu_merge_tiles_dev)
    KEEP_ALL, COMPAT_V6, NO_GRAPH, NO_FUSE, HOST_DETS, SPLIT2, CONCURRENT, BF16_PW = 1, 2, 4, 8, 16, 32, 64, 128
    FEAT_FLAT, FEAT_MEAN, FEAT_MAX = 0, 1, 2                 # FFGPU_FEAT_* (ffgpu_feature_spec.pool)
    POST_NONE, POST_SOFTMAX, POST_L2 = 0, 1, 2               # FFGPU_POST_* (ffgpu_feature_spec.post)
    TOPK_MAX = 16                                            # FFGPU_TOPK_MAX
    RELABEL_KEEP_SCORE, RELABEL_LABEL_SCORE = 0, 1           # FFGPU_RELABEL_* (ffgpu_relabel_spec.score_mode)
    RELABEL_ENTRIES, RELABEL_MERGED = 0, 1                   # FFGPU_RELABEL_* (ffgpu_exec_relabel: which)
    K_AUTO, K_GENERIC, K_DW_STREAM, K_DW_LDS, K_PW_MFMA, K_PW_GEMM, _K6, K_DENSE_SMALL, K_IGEMM, K_PW_BF16, K_GROUP_THIN, K_PW_X3, K_CONV_X3, K_PW_X3T = range(14)


class LAYER(C.Structure):            # include/ffcnn.h (120 bytes)
    _fields_ = [("type", C.c_int), ("refcnt", C.c_int), ("data", f32p), ("filter", f32p),
                ("w", C.c_int), ("h", C.c_int), ("c", C.c_int), ("pad", C.c_int), ("stride", C.c_int),
                ("fn", C.c_int), ("fs", C.c_int), ("groups", C.c_int),
                ("batchnorm", C.c_int), ("activation", C.c_int),
                ("depend_list", C.c_int * 4), ("depend_num", C.c_int),
                ("class_num", C.c_int), ("anchor_list", (C.c_int * 2) * 3),
                ("ignore_thres", C.c_float), ("scale_x_y", C.c_float)]


class BBOX(C.Structure):             # 24 bytes
    _fields_ = [("type", C.c_int), ("score", C.c_float), ("x1", C.c_float), ("y1", C.c_float),
                ("x2", C.c_float), ("y2", C.c_float)]


class NET(C.Structure):              # 104 bytes
    _fields_ = [("layer_list", C.POINTER(LAYER)), ("layer_num", C.c_int),
                ("bbox_list", C.POINTER(BBOX)), ("bbox_num", C.c_int), ("bbox_max", C.c_int),
                ("s1", C.c_int), ("s2", C.c_int), ("weight_size", C.c_int),
                ("weight_buf", f32p), ("cnntempbuf", f32p), ("cnnbufsize", C.c_int),
                ("timeused", C.c_int * 8)]


class FrameDets(C.Structure):        # ffgpu_frame_dets
    _fields_ = [("count", C.c_int), ("ncand", C.c_int), ("overflow", C.c_int), ("nfull", C.c_int),
                ("box", BBOX * FFGPU.MAX_DET)]


class BgrFrame(C.Structure):         # ffgpu_bgr_frame (24 bytes): one u8 BGR frame of a mixed batch
    _fields_ = [("bgr", C.c_void_p), ("w", C.c_int), ("h", C.c_int), ("pitch", C.c_int), ("reserved", C.c_int)]


class Nv12Frame(C.Structure):        # ffgpu_nv12_frame (40 bytes): one NV12 frame (Y plane + interleaved U V plane) of a mixed batch
    _fields_ = [("y", C.c_void_p), ("uv", C.c_void_p), ("w", C.c_int), ("h", C.c_int), ("pitch_y", C.c_int), ("pitch_uv", C.c_int),
                ("matrix", C.c_int), ("reserved", C.c_int)]


class Tile(C.Structure):             # ffgpu_tile (16 bytes): batch entry t is a tile of picture `image` (-1: of none) with origin (x0, y0)
    _fields_ = [("image", C.c_int), ("x0", C.c_int), ("y0", C.c_int), ("reserved", C.c_int)]


class TileRect(C.Structure):         # ffgpu_tile_rect: one tile of a plan (ffgpu_tile_plan)
    _fields_ = [("x0", C.c_int), ("y0", C.c_int), ("w", C.c_int), ("h", C.c_int)]


class DrawStyle(C.Structure):        # ffgpu_draw_style (24 bytes): colour or palette (HOST bytes, 4 per entry) and thickness of the outlines
    _fields_ = [("color", C.c_ubyte * 4), ("palette", C.c_void_p), ("npalette", C.c_int), ("thickness", C.c_int)]


class CropSpec(C.Structure):         # ffgpu_crop_spec (72 bytes): which boxes become crops, the slots' geometry and form
    _fields_ = [("out_w", C.c_int), ("out_h", C.c_int), ("form", C.c_int), ("per_target", C.c_int), ("min_score", C.c_float), ("nclasses", C.c_int),
                ("classes", C.c_void_p), ("margin_num", C.c_int), ("margin_den", C.c_int), ("mean", C.c_float * 3), ("norm", C.c_float * 3),
                ("reserved", C.c_int)]


class Crop(C.Structure):             # ffgpu_crop (48 bytes): one entry of the crop table
    _fields_ = [("target", C.c_int), ("box", C.c_int), ("type", C.c_int), ("score", C.c_float), ("x0", C.c_int), ("y0", C.c_int), ("w", C.c_int),
                ("h", C.c_int), ("sw", C.c_int), ("sh", C.c_int), ("s1", C.c_int), ("s2", C.c_int)]


class TrackSpec(C.Structure):        # ffgpu_track_spec (32 bytes): the tracker's settings
    _fields_ = [("capacity", C.c_int), ("max_missed", C.c_int), ("min_hits", C.c_int), ("iou_thresh", C.c_float), ("min_score", C.c_float),
                ("birth_score", C.c_float), ("class_aware", C.c_int), ("reserved", C.c_int)]


class Track(C.Structure):            # ffgpu_track (48 bytes): one slot of a stream's state
    _fields_ = [("id", C.c_int), ("type", C.c_int), ("score", C.c_float), ("x1", C.c_float), ("y1", C.c_float), ("x2", C.c_float), ("y2", C.c_float),
                ("hits", C.c_int), ("missed", C.c_int), ("born", C.c_int), ("det", C.c_int), ("reserved", C.c_int)]


class FeatureSpec(C.Structure):      # ffgpu_feature_spec (16 bytes): which tensor, how it becomes a row, what is applied to the row
    _fields_ = [("layer", C.c_int), ("pool", C.c_int), ("post", C.c_int), ("reserved", C.c_int)]


class Label(C.Structure):            # ffgpu_label (8 bytes): one entry of a top-k row
    _fields_ = [("index", C.c_int), ("value", C.c_float)]


class RelabelSpec(C.Structure):      # ffgpu_relabel_spec (16 bytes): which labels are applied, and how
    _fields_ = [("min_value", C.c_float), ("type_base", C.c_int), ("score_mode", C.c_int), ("reserved", C.c_int)]


class Gallery(C.Structure):          # ffgpu_gallery (40 bytes): a host struct of device pointers
    _fields_ = [("d_rows", C.c_void_p), ("d_ids", C.c_void_p), ("d_head", C.c_void_p), ("row_stride", C.c_long), ("capacity", C.c_int), ("d", C.c_int)]


class RedactSpec(C.Structure):       # ffgpu_redact_spec (40 bytes): which boxes' regions are redacted, and how
    _fields_ = [("mode", C.c_int), ("cell", C.c_int), ("flags", C.c_int), ("nclasses", C.c_int), ("classes", C.c_void_p), ("min_score", C.c_float),
                ("margin_num", C.c_int), ("margin_den", C.c_int), ("color", C.c_ubyte * 4)]


class BlurSpec(C.Structure):         # ffgpu_blur_spec (40 bytes): which boxes' regions are blurred, and how far
    _fields_ = [("radius", C.c_int), ("passes", C.c_int), ("flags", C.c_int), ("nclasses", C.c_int), ("classes", C.c_void_p), ("min_score", C.c_float),
                ("margin_num", C.c_int), ("margin_den", C.c_int), ("reserved", C.c_int)]


class Zone(C.Structure):             # ffgpu_zone (96 bytes): one polygon of a scene
    _fields_ = [("x", C.c_float * 8), ("y", C.c_float * 8), ("nverts", C.c_int), ("dwell_frames", C.c_int), ("classes", C.c_uint * 4), ("reserved", C.c_int * 2)]


class Line(C.Structure):             # ffgpu_line (32 bytes): one directed segment A -> B of a scene
    _fields_ = [("ax", C.c_float), ("ay", C.c_float), ("bx", C.c_float), ("by", C.c_float), ("classes", C.c_uint * 4)]


class Scene(C.Structure):            # ffgpu_scene (1040 bytes): the zones and lines of one video stream
    _fields_ = [("zone", Zone * 8), ("line", Line * 8), ("nzones", C.c_int), ("nlines", C.c_int), ("anchor", C.c_int), ("reserved", C.c_int)]


class ZonesSpec(C.Structure):        # ffgpu_zones_spec (32 bytes): the zones pass's settings
    _fields_ = [("capacity", C.c_int), ("max_missed", C.c_int), ("identity", C.c_int), ("flags", C.c_int), ("min_score", C.c_float),
                ("gate_zone", C.c_uint), ("gate_line", C.c_uint), ("reserved", C.c_int)]


class ZoneSlot(C.Structure):         # ffgpu_zone_slot (64 bytes): one slot of a stream's state
    _fields_ = [("id", C.c_int), ("px", C.c_float), ("py", C.c_float), ("inside", C.c_int), ("last", C.c_int), ("reserved", C.c_int * 3), ("since", C.c_int * 8)]


class TextItem(C.Structure):         # ffgpu_text_item (64 bytes): one line of text of a target
    _fields_ = [("x", C.c_int), ("y", C.c_int), ("fg", C.c_ubyte * 4), ("bg", C.c_ubyte * 4), ("scale", C.c_ubyte), ("flags", C.c_ubyte), ("len", C.c_ubyte),
                ("reserved", C.c_ubyte), ("text", C.c_ubyte * 44)]


class CaptionSpec(C.Structure):      # ffgpu_caption_spec (48 bytes): which boxes are captioned, with which parts, in which colours
    _fields_ = [("min_score", C.c_float), ("flags", C.c_int), ("identity", C.c_int), ("scale", C.c_int), ("fg", C.c_ubyte * 4), ("color", C.c_ubyte * 4),
                ("palette", C.c_void_p), ("npalette", C.c_int), ("nnames", C.c_int), ("d_names", C.c_void_p)]


class SegItem(C.Structure):          # ffgpu_seg_item (32 bytes): one segment of a target
    _fields_ = [("x0", C.c_int), ("y0", C.c_int), ("x1", C.c_int), ("y1", C.c_int), ("color", C.c_ubyte * 4), ("thickness", C.c_ubyte), ("dash", C.c_ubyte),
                ("flags", C.c_ubyte), ("reserved", C.c_ubyte), ("reserved2", C.c_int * 2)]


class OutlineSpec(C.Structure):      # ffgpu_outline_spec (40 bytes): which parts of a scene are outlined, and how
    _fields_ = [("flags", C.c_int), ("thickness", C.c_int), ("line_dash", C.c_int), ("marker", C.c_int), ("color", C.c_ubyte * 4), ("alarm", C.c_ubyte * 4),
                ("palette", C.c_void_p), ("npalette", C.c_int), ("reserved", C.c_int)]


class TrailPoint(C.Structure):       # ffgpu_trail_point (12 bytes): an anchor and the frame it was seen in
    _fields_ = [("x", C.c_int), ("y", C.c_int), ("frame", C.c_int)]


class TrailSlot(C.Structure):        # ffgpu_trail_slot (416 bytes): one slot of a stream's trails state
    _fields_ = [("id", C.c_int), ("last", C.c_int), ("n", C.c_int), ("head", C.c_int), ("cx", C.c_int), ("cy", C.c_int), ("reserved", C.c_int * 2),
                ("ring", TrailPoint * 32)]


class TrailsSpec(C.Structure):       # ffgpu_trails_spec (64 bytes): the trails pass's settings
    _fields_ = [("capacity", C.c_int), ("max_missed", C.c_int), ("identity", C.c_int), ("flags", C.c_int), ("min_score", C.c_float), ("anchor", C.c_int),
                ("points", C.c_int), ("min_move", C.c_int), ("thickness", C.c_int), ("coast_dash", C.c_int), ("color", C.c_ubyte * 4), ("reserved0", C.c_int),
                ("palette", C.c_void_p), ("npalette", C.c_int), ("reserved", C.c_int)]


class HeatSpec(C.Structure):         # ffgpu_heat_spec (56 bytes): the heat accumulate pass's settings
    _fields_ = [("gw", C.c_int), ("gh", C.c_int), ("cell_log2", C.c_int), ("mode", C.c_int), ("flags", C.c_int), ("anchor", C.c_int), ("spread", C.c_int),
                ("gain", C.c_int), ("decay_shift", C.c_int), ("min_score", C.c_float), ("classes", C.c_void_p), ("nclasses", C.c_int), ("reserved", C.c_int)]


class HeatBlendSpec(C.Structure):    # ffgpu_heat_blend_spec (48 bytes): how a stream's grid is shown in its frames
    _fields_ = [("gw", C.c_int), ("gh", C.c_int), ("cell_log2", C.c_int), ("full_scale", C.c_int), ("floor", C.c_int), ("opacity", C.c_int),
                ("sampling", C.c_int), ("flags", C.c_int), ("palette", C.c_void_p), ("reserved", C.c_int * 2)]


class MotionSpec(C.Structure):       # ffgpu_motion_spec (64 bytes): the motion maps' settings, read by the update and by the gate
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("cell_log2", C.c_int), ("threshold", C.c_int), ("learn_shift", C.c_int), ("learn_shift_changed", C.c_int),
                ("min_pixels", C.c_int), ("cover", C.c_int), ("warmup", C.c_int), ("flags", C.c_int), ("min_score", C.c_float), ("nclasses", C.c_int),
                ("classes", C.c_void_p), ("reserved", C.c_int * 2)]


class PreviewPane(C.Structure):      # ffgpu_preview_pane (32 bytes): a source region of a frame and the pane of a destination surface it is scaled into
    _fields_ = [("sx", C.c_int), ("sy", C.c_int), ("sw", C.c_int), ("sh", C.c_int), ("dx", C.c_int), ("dy", C.c_int), ("dw", C.c_int), ("dh", C.c_int)]


class PreviewSpec(C.Structure):      # ffgpu_preview_spec (16 bytes): how a pane is filled, and what its bars take
    _fields_ = [("fit", C.c_int), ("flags", C.c_int), ("fill", C.c_ubyte * 4), ("reserved", C.c_int)]


class WarpMesh(C.Structure):         # ffgpu_warp_mesh (24 bytes): a mesh of source positions, mh rows of mw (x, y) pairs of int32 in 1 / 256 source pixel
    _fields_ = [("xy", C.c_void_p), ("mw", C.c_int), ("mh", C.c_int), ("cell", C.c_int), ("reserved", C.c_int)]


class WarpSpec(C.Structure):         # ffgpu_warp_spec (16 bytes): how a position is sampled, and what a tap outside the source frame is
    _fields_ = [("filter", C.c_int), ("border", C.c_int), ("fill", C.c_ubyte * 4), ("reserved", C.c_int)]


class WarpLens(C.Structure):         # ffgpu_warp_lens (120 bytes): a lens model for ffgpu_warp_mesh_lens
    _fields_ = [("model", C.c_int), ("reserved", C.c_int), ("dst", C.c_double * 4), ("src", C.c_double * 4), ("k", C.c_double * 4), ("p", C.c_double * 2)]


WARP_MESH_ONE, WARP_SUB = 256, 32                                                      # FFGPU_WARP_MESH_ONE, _SUB
WARP_BILINEAR, WARP_NEAREST = 0, 1                                                     # FFGPU_WARP_* (ffgpu_warp_spec.filter)
WARP_FILL, WARP_CLAMP = 0, 1                                                           # FFGPU_WARP_* (ffgpu_warp_spec.border)
WARP_MAX_SIDE, WARP_MAX_JOBS = 8192, 4096                                              # FFGPU_WARP_MAX_SIDE, _MAX_JOBS
WARP_LENS_BROWN, WARP_LENS_EQUIDISTANT = 0, 1                                          # FFGPU_WARP_LENS_* (ffgpu_warp_lens.model)
PREVIEW_STRETCH, PREVIEW_FIT = 0, 1                                                 # FFGPU_PREVIEW_* (ffgpu_preview_spec.fit)
PREVIEW_KEEP_BARS = 1                                                                  # FFGPU_PREVIEW_KEEP_BARS (ffgpu_preview_spec.flags)
PREVIEW_MAX_SIDE, PREVIEW_MAX_PANES = 8192, 4096                                       # FFGPU_PREVIEW_MAX_SIDE, _MAX_PANES
MOTION_DETS, MOTION_ROW, MOTION_WORDS, MOTION_MAX_SIDE = 128, 16, 8, 8192                # FFGPU_MOTION_DETS, _ROW, _WORDS, _MAX_SIDE
MOTION_GATE_INVERT = 1                                                                 # FFGPU_MOTION_GATE_INVERT (ffgpu_motion_spec.flags)
MOTION_ENTRIES, MOTION_MERGED = 0, 1                                                   # FFGPU_MOTION_* (ffgpu_exec_motion_gate: which)
MOTION_ROW_HEADER = ("frame", "changed", "active", "x0", "y0", "x1", "y1", "warm")
MOTION_WORDS_HEADER = ("considered", "dropped", "outside", "moving", "warm", "frames")
MOTION_STATE_HEADER = 16                                                               # bytes in front of a stream's plane
HEAT_MAX, HEAT_DETS, HEAT_ROW = 2 ** 31 - 1, 128, 8                                    # FFGPU_HEAT_MAX, _DETS, _ROW
HEAT_ANCHOR, HEAT_BOX = 0, 1                                                           # FFGPU_HEAT_* (ffgpu_heat_spec.mode)
HEAT_NEAREST, HEAT_SMOOTH = 0, 1                                                       # FFGPU_HEAT_* (ffgpu_heat_blend_spec.sampling)
HEAT_RAMP_ALPHA = 1                                                                    # FFGPU_HEAT_RAMP_ALPHA (ffgpu_heat_blend_spec.flags)
HEAT_ENTRIES, HEAT_MERGED = 0, 1                                                       # FFGPU_HEAT_* (ffgpu_exec_heat: which)
HEAT_ROW_HEADER = ("considered", "dropped", "outside", "frame", "peak", "saturated")
HEAT_STATE_HEADER = 16                                                                 # bytes in front of a stream's cells
TRAIL_POINTS, TRAILS_DETS, TRAILS_ROW = 32, 128, 16                                    # FFGPU_TRAIL_POINTS, FFGPU_TRAILS_DETS, _ROW
TRAILS_COAST, TRAILS_TAPER = 1, 2                                                      # FFGPU_TRAILS_* (ffgpu_trails_spec.flags)
TRAILS_ENTRIES, TRAILS_MERGED = 0, 1                                                   # FFGPU_TRAILS_* (ffgpu_exec_trails: which)
TRAILS_ROW_HEADER = ("considered", "known", "fresh", "refused", "duplicate", "anonymous", "dropped", "freed", "live", "frame", "appended", "drawn", "clipped")
TRAILS_STATE_HEADER = 16                                                               # bytes in front of a stream's slots
SEG_ITEMS, SEG_LIMIT, OUTLINE_FIXED = 512, 1 << 20, 80                                 # FFGPU_SEG_ITEMS, _LIMIT, FFGPU_OUTLINE_FIXED
OUTLINE_ZONES, OUTLINE_LINES, OUTLINE_TICKS, OUTLINE_MARKERS, OUTLINE_ALARM = 1, 2, 4, 8, 16   # FFGPU_OUTLINE_* (ffgpu_outline_spec.flags)
TEXT_MAX, TEXT_ITEMS, TEXT_OPAQUE = 44, 256, 1                                         # FFGPU_TEXT_MAX, _ITEMS, FFGPU_TEXT_OPAQUE (ffgpu_text_item.flags)
CAPTION_DETS = 128                                                                     # FFGPU_CAPTION_DETS
CAPTION_NAME, CAPTION_SCORE, CAPTION_ID, CAPTION_OPAQUE = 1, 2, 4, 8                   # FFGPU_CAPTION_* (ffgpu_caption_spec.flags)
CAPTION_ENTRIES, CAPTION_MERGED = 0, 1                                                 # FFGPU_CAPTION_* (ffgpu_exec_caption_bgr / _nv12: which)
SCENE_ZONES, SCENE_LINES, ZONE_VERTS, ZONES_DETS, ZONES_ROW = 8, 8, 8, 128, 64          # FFGPU_SCENE_ZONES, _LINES, FFGPU_ZONE_VERTS, FFGPU_ZONES_DETS, _ROW
ZONES_NONE, ZONES_TYPE, ZONES_IDS = 0, 1, 2                                            # FFGPU_ZONES_* (ffgpu_zones_spec.identity)
ZONES_GATE_INVERT = 1                                                                  # FFGPU_ZONES_GATE_INVERT (ffgpu_zones_spec.flags)
ZONES_ENTRIES, ZONES_MERGED = 0, 1                                                     # FFGPU_ZONES_* (ffgpu_exec_zones: which)
ZONES_EVENTS_HEADER = ("considered", "known", "fresh", "refused", "duplicate", "anonymous", "dropped", "freed", "live", "frame")   # the first ints of an event row
ZONES_STATE_HEADER = 144                                                               # bytes in front of a stream's slots
TRACK_DETS = 128                                                                       # FFGPU_TRACK_DETS
TRACK_ENTRIES, TRACK_MERGED = 0, 1                                                     # FFGPU_TRACK_* (ffgpu_exec_track: which)
TRACK_IDS_HEADER = ("considered", "matched", "born", "refused", "dropped", "freed", "live", "frame")   # the 8 ints in front of a row of ids
CROP_F32, CROP_U8 = 0, 1                                                               # FFGPU_CROP_* (ffgpu_crop_spec.form)
CROP_ENTRIES, CROP_MERGED = 0, 1                                                       # FFGPU_CROP_* (ffgpu_exec_crop_bgr / _nv12: which)
REDACT_FILL, REDACT_MOSAIC = 0, 1                                                     # FFGPU_REDACT_* (ffgpu_redact_spec.mode)
REDACT_OUTSIDE = 1                                                                     # FFGPU_REDACT_OUTSIDE (ffgpu_redact_spec.flags)
REDACT_ENTRIES, REDACT_MERGED = 0, 1                                                   # FFGPU_REDACT_* (ffgpu_exec_redact_bgr / _nv12: which)
BLUR_OUTSIDE = 1                                                                       # FFGPU_BLUR_OUTSIDE (ffgpu_blur_spec.flags)
BLUR_ENTRIES, BLUR_MERGED = 0, 1                                                       # FFGPU_BLUR_* (ffgpu_exec_blur_bgr / _nv12: which)
DRAW_ENTRIES, DRAW_MERGED = 0, 1                                                       # FFGPU_DRAW_* (ffgpu_exec_draw_bgr / _nv12: which)
YUV_BT601_LIMITED, YUV_BT601_FULL, YUV_BT709_LIMITED, YUV_BT709_FULL = 0, 1, 2, 3      # FFGPU_YUV_* (ffgpu_nv12_frame.matrix)

assert C.sizeof(LAYER) == 120 and C.sizeof(NET) == 104 and C.sizeof(BBOX) == 24
assert C.sizeof(FrameDets) == 16 + 24 * FFGPU.MAX_DET
assert C.sizeof(BgrFrame) == 24 and C.sizeof(Nv12Frame) == 40 and C.sizeof(Tile) == 16 and C.sizeof(TileRect) == 16
assert C.sizeof(DrawStyle) == 24 and C.sizeof(CropSpec) == 72 and C.sizeof(Crop) == 48
assert C.sizeof(TrackSpec) == 32 and C.sizeof(Track) == 48
assert C.sizeof(FeatureSpec) == 16 and C.sizeof(Label) == 8 and C.sizeof(RelabelSpec) == 16
assert C.sizeof(Gallery) == 40 and C.sizeof(RedactSpec) == 40 and C.sizeof(BlurSpec) == 40
assert C.sizeof(TextItem) == 64 and C.sizeof(CaptionSpec) == 48
assert C.sizeof(SegItem) == 32 and C.sizeof(OutlineSpec) == 40
assert C.sizeof(TrailPoint) == 12 and C.sizeof(TrailSlot) == 416 and C.sizeof(TrailsSpec) == 64
assert C.sizeof(HeatSpec) == 56 and C.sizeof(HeatBlendSpec) == 48
assert C.sizeof(MotionSpec) == 64
assert C.sizeof(Zone) == 96 and C.sizeof(Line) == 32 and C.sizeof(Scene) == 1040 and C.sizeof(ZonesSpec) == 32 and C.sizeof(ZoneSlot) == 64

BOX_DTYPE = np.dtype([("type", "<i4"), ("score", "<f4"), ("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4")])
DETS_DTYPE = np.dtype([("count", "<i4"), ("ncand", "<i4"), ("overflow", "<i4"), ("nfull", "<i4"),
                       ("box", BOX_DTYPE, (FFGPU.MAX_DET,))])
CROP_DTYPE = np.dtype([("target", "<i4"), ("box", "<i4"), ("type", "<i4"), ("score", "<f4"), ("x0", "<i4"), ("y0", "<i4"), ("w", "<i4"), ("h", "<i4"),
                       ("sw", "<i4"), ("sh", "<i4"), ("s1", "<i4"), ("s2", "<i4")])
TRACK_DTYPE = np.dtype([("id", "<i4"), ("type", "<i4"), ("score", "<f4"), ("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"),
                        ("hits", "<i4"), ("missed", "<i4"), ("born", "<i4"), ("det", "<i4"), ("reserved", "<i4")])
ZONE_SLOT_DTYPE = np.dtype([("id", "<i4"), ("px", "<f4"), ("py", "<f4"), ("inside", "<i4"), ("last", "<i4"), ("reserved", "<i4", (3,)), ("since", "<i4", (8,))])
TRAIL_POINT_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("frame", "<i4")])
TRAIL_SLOT_DTYPE = np.dtype([("id", "<i4"), ("last", "<i4"), ("n", "<i4"), ("head", "<i4"), ("cx", "<i4"), ("cy", "<i4"), ("reserved", "<i4", (2,)),
                             ("ring", TRAIL_POINT_DTYPE, (32,))])
LABEL_DTYPE = np.dtype([("index", "<i4"), ("value", "<f4")])
TEXT_ITEM_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("fg", "u1", (4,)), ("bg", "u1", (4,)), ("scale", "u1"), ("flags", "u1"), ("len", "u1"), ("reserved", "u1"),
                            ("text", "u1", (44,))])
SEG_ITEM_DTYPE = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("color", "u1", (4,)), ("thickness", "u1"), ("dash", "u1"), ("flags", "u1"),
                           ("reserved", "u1"), ("reserved2", "<i4", (2,))])

# every symbol include/*.h declares; tests check the built library exports all of them
EXPORTS = ["net_load", "net_free", "net_input", "net_forward", "net_dump", "net_profile", "groupconv",
           "ffgpu_device_count", "ffgpu_set_device", "ffgpu_last_error", "ffgpu_build_info",
           "ffgpu_net_weights_dev", "ffgpu_net_weights_commit",
           "ffgpu_exec_create", "ffgpu_exec_destroy", "ffgpu_exec_batch", "ffgpu_exec_arena_bytes",
           "ffgpu_exec_kernel_count", "ffgpu_exec_work_model", "ffgpu_exec_set_scale", "ffgpu_exec_forward_dev", "ffgpu_exec_forward_host",
           "ffgpu_exec_forward_bgr_dev", "ffgpu_exec_forward_bgr_frames_dev", "ffgpu_exec_forward_nv12_frames_dev", "ffgpu_exec_dets_dev", "ffgpu_exec_dets_host", "ffgpu_exec_set_ring", "ffgpu_exec_set_ring_strided", "ffgpu_exec_read_dets", "ffgpu_exec_read_layer", "ffgpu_exec_hash_layers",
           "ffgpu_exec_read_boxes", "ffgpu_exec_cand_capacity", "ffgpu_exec_graph_captures",
           "ffgpu_exec_profile", "ffgpu_exec_profile_steps", "ffgpu_exec_step_model", "ffgpu_groupconv_dev", "ffgpu_groupconv_kernel_name", "ffgpu_groupconv_time_dev", "ffgpu_irb_dev", "ffgpu_irb_flags_dev", "ffgpu_irb_plan_text", "ffgpu_irb_thin_launch_text", "ffgpu_irb_s2_launch_text", "ffgpu_sparse_head_dev", "ffgpu_sparse_head_launch_text", "ffgpu_irb_stage_plan_text", "ffgpu_front_plan_text", "ffgpu_irb_instantiations", "ffgpu_knobs_text", "ffgpu_dwpw_dev", "ffgpu_packed_records_bytes", "ffgpu_pack_records", "ffgpu_unpack_records",
           "ffgpu_shard_range", "ffgpu_node_create", "ffgpu_node_destroy", "ffgpu_node_ndev", "ffgpu_node_shard", "ffgpu_node_set_scale",
           "ffgpu_node_input_dev", "ffgpu_node_input_slot_dev", "ffgpu_node_depth", "ffgpu_node_rccl_ranks", "ffgpu_node_forward", "ffgpu_node_forward_host",
           "ffgpu_node_submit", "ffgpu_node_wait", "ffgpu_node_run",
           "ffgpu_merge_tiles_scratch_bytes", "ffgpu_merge_tiles_dev", "ffgpu_exec_merge_tiles", "ffgpu_exec_merged_dev", "ffgpu_exec_read_merged",
           "ffgpu_exec_read_merged_boxes", "ffgpu_tile_plan",
           "ffgpu_draw_boxes_bgr_dev", "ffgpu_draw_boxes_nv12_dev", "ffgpu_exec_draw_bgr", "ffgpu_exec_draw_nv12",
           "ffgpu_crop_table_bytes", "ffgpu_crop_slot_bytes", "ffgpu_crop_boxes_bgr_dev", "ffgpu_crop_boxes_nv12_dev", "ffgpu_exec_crop_bgr", "ffgpu_exec_crop_nv12",
           "ffgpu_crops_to_source_dev",
           "ffgpu_track_state_bytes", "ffgpu_track_reset_dev", "ffgpu_track_boxes_dev", "ffgpu_exec_track",
           "ffgpu_feature_dim", "ffgpu_exec_feature_dim", "ffgpu_features_dev", "ffgpu_exec_features", "ffgpu_topk_dev", "ffgpu_crops_relabel_dev",
           "ffgpu_exec_relabel",
           "ffgpu_match_workspace_bytes", "ffgpu_match_dev", "ffgpu_gallery_enroll_dev",
           "ffgpu_redact_boxes_bgr_dev", "ffgpu_redact_boxes_nv12_dev", "ffgpu_exec_redact_bgr", "ffgpu_exec_redact_nv12",
           "ffgpu_blur_boxes_bgr_dev", "ffgpu_blur_boxes_nv12_dev", "ffgpu_exec_blur_bgr", "ffgpu_exec_blur_nv12",
           "ffgpu_zones_state_bytes", "ffgpu_scene_check", "ffgpu_zones_reset_dev", "ffgpu_zones_boxes_dev", "ffgpu_exec_zones",
           "ffgpu_font_builtin", "ffgpu_draw_text_bgr_dev", "ffgpu_draw_text_nv12_dev", "ffgpu_caption_boxes_dev", "ffgpu_exec_caption_bgr", "ffgpu_exec_caption_nv12",
           "ffgpu_caption_scene_dev",
           "ffgpu_draw_segments_bgr_dev", "ffgpu_draw_segments_nv12_dev", "ffgpu_outline_spec_check", "ffgpu_outline_scene_dev",
           "ffgpu_trails_state_bytes", "ffgpu_trails_spec_check", "ffgpu_trails_reset_dev", "ffgpu_trails_boxes_dev", "ffgpu_exec_trails",
           "ffgpu_heat_state_bytes", "ffgpu_heat_spec_check", "ffgpu_heat_blend_spec_check", "ffgpu_heat_palette", "ffgpu_heat_reset_dev", "ffgpu_heat_boxes_dev",
           "ffgpu_exec_heat", "ffgpu_heat_blend_bgr_dev", "ffgpu_heat_blend_nv12_dev",
           "ffgpu_motion_state_bytes", "ffgpu_motion_spec_check", "ffgpu_motion_reset_dev", "ffgpu_motion_update_bgr_dev", "ffgpu_motion_update_nv12_dev",
           "ffgpu_motion_gate_dev", "ffgpu_exec_motion_gate",
           "ffgpu_preview_spec_check", "ffgpu_preview_rect", "ffgpu_preview_grid", "ffgpu_preview_tile", "ffgpu_preview_bgr_dev", "ffgpu_preview_nv12_dev",
           "ffgpu_warp_spec_check", "ffgpu_warp_mesh_size", "ffgpu_warp_mesh_orient", "ffgpu_warp_mesh_homography", "ffgpu_warp_mesh_lens", "ffgpu_warp_point",
           "ffgpu_warp_tile", "ffgpu_warp_bgr_dev", "ffgpu_warp_nv12_dev"]
# include/ffcnn_hip_diag.h (libffcnn_hip_diag.so: lab equipment, its own library)
DIAG_EXPORTS = ["ffgpu_membench", "ffgpu_pipe_probe", "ffgpu_pipe_probe2", "ffgpu_pipe_probe3", "ffgpu_mfma_floor", "ffgpu_diag_x3_term", "ffgpu_diag_xl_op", "ffgpu_clock_probe"]


def library_path():
    return os.environ.get("FFCNN_HIP_LIB") or os.path.join(HERE, "lib", "libffcnn_hip.so")     # (override: tuning builds)


def build_library(force=False):
    """Compile libffcnn_hip.so in-tree (gcc + hipcc --offload-arch=gfx950)."""
    cmd = ["make", "-C", os.path.join(HERE, "csrc")]
    if force:
        subprocess.check_call(cmd + ["clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
    return library_path()


_lib = None


def lib():
    """The loaded C-ABI library.  Raises if it was not built: there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise RuntimeError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(the HIP extension is the only compute path)" % path)
    L = C.CDLL(path)
    vp, i, sz = C.c_void_p, C.c_int, C.c_size_t
    L.net_load.restype = C.POINTER(NET)
    L.net_load.argtypes = [C.c_char_p, C.c_char_p, i, i]
    L.net_free.argtypes = [C.POINTER(NET)]
    L.net_input.argtypes = [C.POINTER(NET), vp, i, i, f32p, f32p]
    L.net_forward.argtypes = [C.POINTER(NET)]
    L.net_dump.argtypes = [C.POINTER(NET)]
    L.net_profile.argtypes = [C.POINTER(NET)]
    L.groupconv.argtypes = [f32p, f32p, f32p] + [i] * 12 + [C.POINTER(f32p), C.POINTER(i)]
    L.ffgpu_last_error.restype = C.c_char_p
    L.ffgpu_build_info.restype = C.c_char_p
    # a lab build (make DIAG=1: FFGPU_DBG_SKIP / FFGPU_DBG_KEEP drop launches, results are wrong by design) is only loaded when the caller says so
    if b" DIAG " in L.ffgpu_build_info() and os.environ.get("FFCNN_HIP_ALLOW_DIAG") != "1":
        raise RuntimeError("%s is a DIAG (lab) build of libffcnn_hip; set FFCNN_HIP_ALLOW_DIAG=1 to load it on purpose" % path)
    L.ffgpu_set_device.argtypes = [i]
    L.ffgpu_net_weights_dev.argtypes = [C.POINTER(NET), C.POINTER(vp), C.POINTER(sz)]
    L.ffgpu_net_weights_commit.argtypes = [C.POINTER(NET), vp]
    L.ffgpu_exec_create.restype = vp
    L.ffgpu_exec_create.argtypes = [C.POINTER(NET), i, i]
    L.ffgpu_exec_destroy.argtypes = [vp]
    L.ffgpu_exec_batch.argtypes = [vp]
    L.ffgpu_exec_arena_bytes.restype = sz
    L.ffgpu_exec_arena_bytes.argtypes = [vp]
    L.ffgpu_exec_kernel_count.argtypes = [vp]
    L.ffgpu_exec_work_model.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.ffgpu_exec_set_scale.argtypes = [vp, i, i]
    L.ffgpu_exec_forward_dev.argtypes = [vp, vp, vp]
    L.ffgpu_exec_forward_host.argtypes = [vp, f32p]
    L.ffgpu_exec_forward_bgr_dev.argtypes = [vp, vp, i, i, f32p, f32p, vp]
    L.ffgpu_exec_forward_bgr_frames_dev.argtypes = [vp, C.POINTER(BgrFrame), i, f32p, f32p, vp]
    L.ffgpu_exec_forward_nv12_frames_dev.argtypes = [vp, C.POINTER(Nv12Frame), i, f32p, f32p, vp]
    L.ffgpu_exec_dets_dev.argtypes = [vp, C.POINTER(vp), C.POINTER(sz)]
    L.ffgpu_exec_dets_host.restype = vp; L.ffgpu_exec_dets_host.argtypes = [vp]
    L.ffgpu_exec_set_ring.argtypes = [vp, vp, C.c_int]
    L.ffgpu_exec_set_ring_strided.argtypes = [vp, vp, C.c_int, C.c_int]
    L.ffgpu_exec_read_dets.argtypes = [vp, vp, i]
    L.ffgpu_exec_read_layer.argtypes = [vp, i, i, f32p, sz]
    L.ffgpu_exec_hash_layers.argtypes = [vp, vp, i]
    L.ffgpu_exec_profile.argtypes = [vp, vp, f32p]
    L.ffgpu_exec_profile_steps.argtypes = [vp, vp, C.POINTER(i), f32p, i]
    L.ffgpu_exec_step_model.argtypes = [vp, C.POINTER(i), C.POINTER(C.c_double), i]
    L.ffgpu_groupconv_dev.argtypes = [vp, vp, vp] + [i] * 15 + [vp]
    L.ffgpu_groupconv_kernel_name.restype = C.c_char_p
    L.ffgpu_groupconv_kernel_name.argtypes = [i] * 10
    L.ffgpu_groupconv_time_dev.restype = C.c_float
    L.ffgpu_groupconv_time_dev.argtypes = [vp, vp, vp] + [i] * 17 + [vp]
    L.ffgpu_irb_dev.restype = C.c_float
    L.ffgpu_irb_dev.argtypes = [vp] * 6 + [i] * 13 + [vp]
    L.ffgpu_irb_flags_dev.restype = C.c_float
    L.ffgpu_irb_flags_dev.argtypes = [vp] * 6 + [i] * 14 + [vp]
    L.ffgpu_irb_thin_launch_text.argtypes = [i] * 12 + [C.c_char_p, i]
    L.ffgpu_irb_s2_launch_text.argtypes = [i] * 12 + [C.c_char_p, i]
    L.ffgpu_sparse_head_dev.argtypes = [vp, vp, vp] + [i] * 6 + [C.c_float, vp, vp, vp]
    L.ffgpu_sparse_head_launch_text.argtypes = [i] * 6 + [C.c_char_p, i]
    L.ffgpu_irb_plan_text.argtypes = [i] * 12 + [C.c_char_p, i]
    L.ffgpu_irb_stage_plan_text.argtypes = [i] * 7 + [C.c_char_p, i]
    L.ffgpu_front_plan_text.argtypes = [i] * 4 + [C.c_char_p, i]
    L.ffgpu_irb_instantiations.argtypes = [C.c_char_p, i]
    L.ffgpu_knobs_text.argtypes = [C.c_char_p, i]
    L.ffgpu_exec_read_boxes.argtypes = [vp, i, vp, i]
    L.ffgpu_exec_cand_capacity.argtypes = [vp]
    L.ffgpu_exec_graph_captures.argtypes = [vp]
    L.ffgpu_dwpw_dev.restype = C.c_float
    L.ffgpu_dwpw_dev.argtypes = [vp] * 4 + [i] * 10 + [vp]
    L.ffgpu_packed_records_bytes.restype = C.c_size_t
    L.ffgpu_packed_records_bytes.argtypes = [i, i]
    L.ffgpu_pack_records.restype = i
    L.ffgpu_pack_records.argtypes = [vp, i, C.c_long, i, i, vp, vp]
    L.ffgpu_shard_range.argtypes = [i, i, i, C.POINTER(i), C.POINTER(i)]
    L.ffgpu_shard_range.restype = None
    L.ffgpu_node_create.restype = vp
    L.ffgpu_node_create.argtypes = [C.POINTER(NET), i, C.POINTER(i), i, i, i]
    L.ffgpu_node_destroy.argtypes = [vp]
    L.ffgpu_node_ndev.argtypes = [vp]
    L.ffgpu_node_shard.argtypes = [vp, i, C.POINTER(i), C.POINTER(i), C.POINTER(i)]
    L.ffgpu_node_set_scale.argtypes = [vp, i, i]
    L.ffgpu_node_input_dev.restype = vp
    L.ffgpu_node_input_dev.argtypes = [vp, i]
    L.ffgpu_node_input_slot_dev.restype = vp
    L.ffgpu_node_input_slot_dev.argtypes = [vp, i, i]
    L.ffgpu_node_depth.argtypes = [vp]
    if hasattr(L, "ffgpu_node_rccl_ranks"):                     # (absent from older tuning builds loaded through FFCNN_HIP_LIB)
        L.ffgpu_node_rccl_ranks.argtypes = [vp]
    L.ffgpu_node_submit.restype = C.c_long
    L.ffgpu_node_submit.argtypes = [vp, f32p]
    L.ffgpu_node_wait.argtypes = [vp, C.c_long, vp]
    L.ffgpu_node_run.argtypes = [vp, C.c_long, vp]
    L.ffgpu_unpack_records.argtypes = [vp, i, i, vp]
    L.ffgpu_node_forward.argtypes = [vp, vp]
    L.ffgpu_node_forward_host.argtypes = [vp, f32p, vp]
    L.ffgpu_merge_tiles_scratch_bytes.restype = sz
    L.ffgpu_merge_tiles_scratch_bytes.argtypes = [i, i]
    L.ffgpu_merge_tiles_dev.argtypes = [vp, vp, i, C.POINTER(Tile), i, i, C.c_float, i, vp, vp, vp, sz, vp]
    L.ffgpu_exec_merge_tiles.argtypes = [vp, C.POINTER(Tile), i, i, vp]
    L.ffgpu_exec_merged_dev.argtypes = [vp, C.POINTER(vp), C.POINTER(sz)]
    L.ffgpu_exec_read_merged.argtypes = [vp, vp, i]
    L.ffgpu_exec_read_merged_boxes.argtypes = [vp, i, vp, i]
    L.ffgpu_tile_plan.argtypes = [i] * 7 + [C.POINTER(TileRect), i]
    L.ffgpu_draw_boxes_bgr_dev.argtypes = [vp, vp, i, C.POINTER(i), C.POINTER(BgrFrame), i, C.POINTER(DrawStyle), vp]
    L.ffgpu_draw_boxes_nv12_dev.argtypes = [vp, vp, i, C.POINTER(i), C.POINTER(Nv12Frame), i, C.POINTER(DrawStyle), vp]
    L.ffgpu_exec_draw_bgr.argtypes = [vp, i, C.POINTER(BgrFrame), i, C.POINTER(DrawStyle), vp]
    L.ffgpu_exec_draw_nv12.argtypes = [vp, i, C.POINTER(Nv12Frame), i, C.POINTER(DrawStyle), vp]
    L.ffgpu_redact_boxes_bgr_dev.argtypes = [vp, vp, i, C.POINTER(i), C.POINTER(BgrFrame), i, C.POINTER(RedactSpec), vp]
    L.ffgpu_redact_boxes_nv12_dev.argtypes = [vp, vp, i, C.POINTER(i), C.POINTER(Nv12Frame), i, C.POINTER(RedactSpec), vp]
    L.ffgpu_exec_redact_bgr.argtypes = [vp, i, C.POINTER(BgrFrame), i, C.POINTER(RedactSpec), vp]
    L.ffgpu_exec_redact_nv12.argtypes = [vp, i, C.POINTER(Nv12Frame), i, C.POINTER(RedactSpec), vp]
    L.ffgpu_blur_boxes_bgr_dev.argtypes = [vp, vp, i, C.POINTER(i), C.POINTER(BgrFrame), C.POINTER(BgrFrame), i, C.POINTER(BlurSpec), vp]
    L.ffgpu_blur_boxes_nv12_dev.argtypes = [vp, vp, i, C.POINTER(i), C.POINTER(Nv12Frame), C.POINTER(Nv12Frame), i, C.POINTER(BlurSpec), vp]
    L.ffgpu_exec_blur_bgr.argtypes = [vp, i, C.POINTER(BgrFrame), C.POINTER(BgrFrame), i, C.POINTER(BlurSpec), vp]
    L.ffgpu_exec_blur_nv12.argtypes = [vp, i, C.POINTER(Nv12Frame), C.POINTER(Nv12Frame), i, C.POINTER(BlurSpec), vp]
    L.ffgpu_crop_table_bytes.restype = sz
    L.ffgpu_crop_table_bytes.argtypes = [i]
    L.ffgpu_crop_slot_bytes.restype = sz
    L.ffgpu_crop_slot_bytes.argtypes = [i, i, i]
    L.ffgpu_crop_boxes_bgr_dev.argtypes = [vp, vp, i, C.POINTER(i), C.POINTER(BgrFrame), i, C.POINTER(CropSpec), vp, vp, i, vp]
    L.ffgpu_crop_boxes_nv12_dev.argtypes = [vp, vp, i, C.POINTER(i), C.POINTER(Nv12Frame), i, C.POINTER(CropSpec), vp, vp, i, vp]
    L.ffgpu_exec_crop_bgr.argtypes = [vp, i, C.POINTER(BgrFrame), i, C.POINTER(CropSpec), vp, vp, i, vp]
    L.ffgpu_exec_crop_nv12.argtypes = [vp, i, C.POINTER(Nv12Frame), i, C.POINTER(CropSpec), vp, vp, i, vp]
    L.ffgpu_crops_to_source_dev.argtypes = [vp, i, vp, vp, i, vp, vp, vp]
    L.ffgpu_track_state_bytes.restype = sz
    L.ffgpu_track_state_bytes.argtypes = [i, i]
    L.ffgpu_track_reset_dev.argtypes = [vp, i, i, i, vp]
    L.ffgpu_track_boxes_dev.argtypes = [vp, vp, i, C.POINTER(i), C.POINTER(i), i, C.POINTER(TrackSpec), vp, i, vp, vp, vp, vp]
    L.ffgpu_exec_track.argtypes = [vp, i, C.POINTER(i), i, C.POINTER(TrackSpec), vp, i, vp, vp, vp, vp]
    L.ffgpu_zones_state_bytes.restype = sz
    L.ffgpu_zones_state_bytes.argtypes = [i, i]
    L.ffgpu_scene_check.argtypes = [C.POINTER(Scene), i]
    L.ffgpu_zones_reset_dev.argtypes = [vp, i, i, i, vp]
    L.ffgpu_zones_boxes_dev.argtypes = [vp, vp, i, C.POINTER(i), C.POINTER(i), i, C.POINTER(ZonesSpec), vp, vp, i, vp, vp, vp, vp, vp]
    L.ffgpu_exec_zones.argtypes = [vp, i, C.POINTER(i), i, C.POINTER(ZonesSpec), vp, vp, i, vp, vp, vp, vp, vp]
    L.ffgpu_font_builtin.restype = None
    L.ffgpu_font_builtin.argtypes = [vp]
    L.ffgpu_draw_text_bgr_dev.argtypes = [vp, i, vp, C.POINTER(BgrFrame), i, vp]
    L.ffgpu_draw_text_nv12_dev.argtypes = [vp, i, vp, C.POINTER(Nv12Frame), i, vp]
    L.ffgpu_caption_boxes_dev.argtypes = [vp, vp, i, C.POINTER(i), i, C.POINTER(CaptionSpec), vp, vp, i, vp]
    L.ffgpu_exec_caption_bgr.argtypes = [vp, i, C.POINTER(BgrFrame), i, C.POINTER(CaptionSpec), vp, vp, i, vp, vp]
    L.ffgpu_exec_caption_nv12.argtypes = [vp, i, C.POINTER(Nv12Frame), i, C.POINTER(CaptionSpec), vp, vp, i, vp, vp]
    L.ffgpu_caption_scene_dev.argtypes = [vp, vp, i, i, vp, i, C.POINTER(i), i, C.POINTER(CaptionSpec), vp, i, vp]
    L.ffgpu_draw_segments_bgr_dev.argtypes = [vp, i, C.POINTER(BgrFrame), i, vp]
    L.ffgpu_draw_segments_nv12_dev.argtypes = [vp, i, C.POINTER(Nv12Frame), i, vp]
    L.ffgpu_outline_spec_check.argtypes = [C.POINTER(OutlineSpec)]
    L.ffgpu_trails_state_bytes.restype = sz
    L.ffgpu_trails_state_bytes.argtypes = [i, i]
    L.ffgpu_trails_spec_check.argtypes = [C.POINTER(TrailsSpec)]
    L.ffgpu_trails_reset_dev.argtypes = [vp, i, i, i, vp]
    L.ffgpu_trails_boxes_dev.argtypes = [vp, vp, i, C.POINTER(i), C.POINTER(i), i, C.POINTER(TrailsSpec), vp, i, vp, vp, vp, i, i, i, vp]
    L.ffgpu_exec_trails.argtypes = [vp, i, C.POINTER(i), i, C.POINTER(TrailsSpec), vp, i, vp, vp, vp, i, i, i, vp]
    L.ffgpu_heat_state_bytes.restype = sz
    L.ffgpu_heat_state_bytes.argtypes = [i, i, i]
    L.ffgpu_heat_spec_check.argtypes = [C.POINTER(HeatSpec)]
    L.ffgpu_heat_blend_spec_check.argtypes = [C.POINTER(HeatBlendSpec)]
    L.ffgpu_heat_palette.argtypes = [i, vp]
    L.ffgpu_heat_reset_dev.argtypes = [vp, i, i, i, i, vp]
    L.ffgpu_heat_boxes_dev.argtypes = [vp, vp, i, C.POINTER(i), C.POINTER(i), i, C.POINTER(HeatSpec), vp, i, vp, vp]
    L.ffgpu_exec_heat.argtypes = [vp, i, C.POINTER(i), i, C.POINTER(HeatSpec), vp, i, vp, vp]
    L.ffgpu_heat_blend_bgr_dev.argtypes = [vp, i, C.POINTER(i), C.POINTER(BgrFrame), i, C.POINTER(HeatBlendSpec), vp]
    L.ffgpu_heat_blend_nv12_dev.argtypes = [vp, i, C.POINTER(i), C.POINTER(Nv12Frame), i, C.POINTER(HeatBlendSpec), vp]
    L.ffgpu_motion_state_bytes.restype = sz
    L.ffgpu_motion_state_bytes.argtypes = [i, i, i, i]
    L.ffgpu_motion_spec_check.argtypes = [C.POINTER(MotionSpec)]
    L.ffgpu_motion_reset_dev.argtypes = [vp, i, i, i, i, i, vp]
    L.ffgpu_motion_update_bgr_dev.argtypes = [C.POINTER(BgrFrame), i, C.POINTER(i), C.POINTER(MotionSpec), vp, i, vp, vp]
    L.ffgpu_motion_update_nv12_dev.argtypes = [C.POINTER(Nv12Frame), i, C.POINTER(i), C.POINTER(MotionSpec), vp, i, vp, vp]
    L.ffgpu_motion_gate_dev.argtypes = [vp, vp, i, C.POINTER(i), C.POINTER(i), i, C.POINTER(MotionSpec), vp, i, vp, vp, vp, vp]
    L.ffgpu_exec_motion_gate.argtypes = [vp, i, C.POINTER(i), i, C.POINTER(MotionSpec), vp, i, vp, vp, vp, vp]
    L.ffgpu_preview_spec_check.argtypes = [C.POINTER(PreviewSpec)]
    L.ffgpu_preview_rect.argtypes = [i, i, i, i, C.POINTER(PreviewPane), C.POINTER(PreviewSpec), i, C.POINTER(i)]
    L.ffgpu_preview_grid.argtypes = [i, i, i, i, i, i, C.POINTER(PreviewPane)]
    L.ffgpu_preview_tile.argtypes = [C.POINTER(i)]
    L.ffgpu_preview_bgr_dev.argtypes = [C.POINTER(BgrFrame), C.POINTER(BgrFrame), C.POINTER(PreviewPane), i, C.POINTER(PreviewSpec), vp]
    L.ffgpu_preview_nv12_dev.argtypes = [C.POINTER(Nv12Frame), C.POINTER(Nv12Frame), C.POINTER(PreviewPane), i, C.POINTER(PreviewSpec), vp]
    L.ffgpu_warp_spec_check.argtypes = [C.POINTER(WarpSpec)]
    L.ffgpu_warp_mesh_size.argtypes = [i, i, i, C.POINTER(i)]
    L.ffgpu_warp_mesh_orient.argtypes = [i, i, i, i, C.POINTER(i), vp]
    L.ffgpu_warp_mesh_homography.argtypes = [i, i, i, C.POINTER(C.c_double), vp]
    L.ffgpu_warp_mesh_lens.argtypes = [i, i, i, C.POINTER(WarpLens), vp]
    L.ffgpu_warp_point.argtypes = [C.POINTER(WarpMesh), i, i, i, i, C.POINTER(i)]
    L.ffgpu_warp_tile.argtypes = [C.POINTER(i)]
    L.ffgpu_warp_bgr_dev.argtypes = [C.POINTER(BgrFrame), C.POINTER(BgrFrame), C.POINTER(WarpMesh), i, C.POINTER(WarpSpec), vp]
    L.ffgpu_warp_nv12_dev.argtypes = [C.POINTER(Nv12Frame), C.POINTER(Nv12Frame), C.POINTER(WarpMesh), i, C.POINTER(WarpSpec), vp]
    L.ffgpu_outline_scene_dev.argtypes = [vp, vp, i, i, vp, i, C.POINTER(i), i, C.POINTER(OutlineSpec), vp, i, vp]
    L.ffgpu_feature_dim.argtypes = [i, i, i, i]
    L.ffgpu_exec_feature_dim.argtypes = [vp, C.POINTER(FeatureSpec)]
    L.ffgpu_features_dev.argtypes = [vp, i, i, i, i, i, i, vp, C.c_long, vp]
    L.ffgpu_exec_features.argtypes = [vp, C.POINTER(FeatureSpec), vp, C.c_long, vp]
    L.ffgpu_topk_dev.argtypes = [vp, i, i, C.c_long, i, vp, vp]
    L.ffgpu_crops_relabel_dev.argtypes = [vp, i, vp, i, vp, vp, i, C.POINTER(i), i, C.POINTER(RelabelSpec), vp, vp, vp]
    L.ffgpu_exec_relabel.argtypes = [vp, i, vp, i, vp, i, i, C.POINTER(RelabelSpec), vp, vp, vp]
    L.ffgpu_match_workspace_bytes.restype = sz
    L.ffgpu_match_workspace_bytes.argtypes = [i, i, i]
    L.ffgpu_match_dev.argtypes = [vp, i, C.c_long, C.POINTER(Gallery), i, vp, vp, C.c_long, vp, sz, vp]
    L.ffgpu_gallery_enroll_dev.argtypes = [C.POINTER(Gallery), vp, i, C.c_long, vp, i, C.c_float, vp, vp]
    _lib = L
    return L


_diag = None


def diag_path():
    return os.path.join(HERE, "lib", "libffcnn_hip_diag.so")


def diag():
    """libffcnn_hip_diag.so (include/ffcnn_hip_diag.h): HBM stream calibration and pipe probes; not the product."""
    global _diag
    if _diag is None:
        D = C.CDLL(diag_path())
        vp, i, sz = C.c_void_p, C.c_int, C.c_size_t
        D.ffgpu_membench.restype = C.c_float
        D.ffgpu_membench.argtypes = [vp, vp, sz, i, i, i, vp]
        D.ffgpu_pipe_probe.restype = C.c_float
        D.ffgpu_pipe_probe.argtypes = [i, i, i, i, vp]
        D.ffgpu_pipe_probe2.restype = C.c_float
        D.ffgpu_pipe_probe2.argtypes = [i, i, i, i, vp]
        D.ffgpu_pipe_probe3.restype = C.c_float
        D.ffgpu_pipe_probe3.argtypes = [i, i, i, i, i, vp]
        D.ffgpu_clock_probe.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        D.ffgpu_mfma_floor.restype = C.c_float
        D.ffgpu_mfma_floor.argtypes = [vp, i, i, i, vp]
        _diag = D
    return _diag


def load_bmp(path):
    """24-bit BMP -> (bgr rows top-down with stride ALIGN(3w,4), w, h); what the demo feeds net_input."""
    raw = open(path, "rb").read()
    w, h = int.from_bytes(raw[18:22], "little"), int.from_bytes(raw[22:26], "little")
    pitch = (w * 3 + 3) & ~3
    rows = np.frombuffer(raw, np.uint8, pitch * h, 54).reshape(h, pitch)[::-1]
    return np.ascontiguousarray(rows), w, h


def last_error():
    return lib().ffgpu_last_error().decode(errors="replace")


def _check(rc, what):
    if rc < 0:
        raise RuntimeError("%s failed: %s" % (what, last_error()))
    return rc


# ---- ffcnn.h mirror (same names / argument meaning as the reference) -------
def net_load(cfg=CFG, weights=WEIGHTS, inputw=0, inputh=0):
    """NET* or None (cfg unreadable, allocation failure, or no HIP device)."""
    p = lib().net_load(cfg.encode() if cfg else None, weights.encode() if weights else None, inputw, inputh)
    return p if p else None


def net_free(net):
    lib().net_free(net)


def net_input(net, bgr, w, h, mean=(0.0, 0.0, 0.0), norm=(1 / 255.0, 1 / 255.0, 1 / 255.0)):
    m, s = (C.c_float * 3)(*mean), (C.c_float * 3)(*norm)
    lib().net_input(net, bgr.ctypes.data, w, h, m, s)


def net_forward(net):
    lib().net_forward(net)


def net_dump(net):
    lib().net_dump(net)


def groupconv(x, filt, groups, pad, stride, fs, act):
    """conv.h drop-in with host arrays: x (ic, ih, iw), filt (fn, K4+4) -> (fn, oh, ow)."""
    ic, ih, iw = x.shape
    fn = filt.shape[0]
    oh, ow = (ih + 2 * pad - fs) // stride + 1, (iw + 2 * pad - fs) // stride + 1
    x = np.ascontiguousarray(x, np.float32)
    filt = np.ascontiguousarray(filt, np.float32)
    out = np.full((fn, oh, ow), np.nan, np.float32)
    buf, size = f32p(), C.c_int(0)
    lib().groupconv(x.ctypes.data_as(f32p), filt.ctypes.data_as(f32p), out.ctypes.data_as(f32p),
                    iw, ih, ic, groups, pad, stride, fs, fn, ow, oh, fn, act, C.byref(buf), C.byref(size))
    return out


def boxes_of(net):
    n = net.contents
    k = n.bbox_num
    if k <= 0:
        return np.zeros(0, BOX_DTYPE)
    return np.frombuffer((BBOX * k).from_address(C.addressof(n.bbox_list.contents)), BOX_DTYPE, k).copy()


# ---- convenience wrappers ---------------------------------------------------
class Net:
    """Owns a NET* (net_load/net_free) and exposes the layer table."""

    def __init__(self, cfg=CFG, weights=WEIGHTS, w=0, h=0):
        self.p = net_load(cfg, weights, w, h)
        if self.p is None:
            raise RuntimeError("net_load failed: %s" % last_error())
        self.n = self.p.contents

    def close(self):
        if self.p is not None:
            net_free(self.p)
            self.p = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def layer_num(self):
        return self.n.layer_num

    def layer(self, i):
        return self.n.layer_list[i]

    @property
    def input_shape(self):
        l0 = self.n.layer_list[0]
        return (l0.c, l0.h, l0.w)

    @property
    def input(self):
        return np.ctypeslib.as_array(self.n.layer_list[0].data, self.input_shape)

    def set_input_image(self, bgr, w, h, mean=(0.0, 0.0, 0.0), norm=(1 / 255.0,) * 3):
        self.input[...] = 0
        net_input(self.p, bgr, w, h, mean, norm)

    def forward(self):
        net_forward(self.p)

    @property
    def boxes(self):
        return boxes_of(self.p)

    def out_shape(self, i):
        o = self.n.layer_list[i + 1]
        return (o.c, o.h, o.w)

    def weights_host(self):
        return np.ctypeslib.as_array(self.n.weight_buf, (self.n.weight_size,))

    def weights_dev(self):
        ptr, nbytes = C.c_void_p(), C.c_size_t()
        _check(lib().ffgpu_net_weights_dev(self.p, C.byref(ptr), C.byref(nbytes)), "ffgpu_net_weights_dev")
        return ptr.value, nbytes.value

    def weights_commit(self, stream=None):
        _check(lib().ffgpu_net_weights_commit(self.p, stream), "ffgpu_net_weights_commit")

    def executor(self, batch, flags=0):
        return Executor(self, batch, flags)


class Executor:
    """A planned batched executor (ffgpu_exec_*)."""

    def __init__(self, net, batch, flags=0):
        self.net = net
        self.h = lib().ffgpu_exec_create(net.p, batch, flags)
        if not self.h:
            raise RuntimeError("ffgpu_exec_create failed: %s" % last_error())
        self.batch = batch
        self.flags = flags

    def close(self):
        if self.h:
            lib().ffgpu_exec_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def arena_bytes(self):
        return lib().ffgpu_exec_arena_bytes(self.h)

    @property
    def kernel_count(self):
        return lib().ffgpu_exec_kernel_count(self.h)

    def work_model(self):
        """(HBM bytes, flops) one forward of this plan must move / compute"""
        b, f = C.c_double(), C.c_double()
        _check(lib().ffgpu_exec_work_model(self.h, C.byref(b), C.byref(f)), "ffgpu_exec_work_model")
        return b.value, f.value

    def set_scale(self, s1, s2):
        _check(lib().ffgpu_exec_set_scale(self.h, s1, s2), "ffgpu_exec_set_scale")

    def forward_dev(self, dev_ptr, stream=None):
        _check(lib().ffgpu_exec_forward_dev(self.h, dev_ptr, stream), "ffgpu_exec_forward_dev")

    def forward_host(self, frames):
        frames = np.ascontiguousarray(frames, np.float32)
        assert frames.shape == (self.batch,) + self.net.input_shape, frames.shape
        _check(lib().ffgpu_exec_forward_host(self.h, frames.ctypes.data_as(f32p)), "ffgpu_exec_forward_host")

    def forward_bgr_dev(self, dev_ptr, w, h, mean=(0.0, 0.0, 0.0), norm=(1 / 255.0,) * 3, stream=None):
        m, s = (C.c_float * 3)(*mean), (C.c_float * 3)(*norm)
        _check(lib().ffgpu_exec_forward_bgr_dev(self.h, dev_ptr, w, h, m, s, stream), "ffgpu_exec_forward_bgr_dev")

    def forward_bgr_frames_dev(self, frames, mean=(0.0, 0.0, 0.0), norm=(1 / 255.0,) * 3, stream=None):
        """one forward of mixed-size u8 BGR frames (ffgpu_exec_forward_bgr_frames_dev): frames is a sequence of (ptr, w, h, pitch) tuples
        (pitch 0 = ALIGN(3 w, 4)) or torch.uint8 device tensors of shape (h, pitch) (w = pitch // 3) or (h, w, 3)"""
        arr = (BgrFrame * max(1, len(frames)))()
        for k, f in enumerate(frames):
            arr[k] = BgrFrame(*bgr_frame_desc(f))
        m, s = (C.c_float * 3)(*mean), (C.c_float * 3)(*norm)
        _check(lib().ffgpu_exec_forward_bgr_frames_dev(self.h, arr, len(frames), m, s, stream), "ffgpu_exec_forward_bgr_frames_dev")

    def forward_nv12_frames_dev(self, frames, mean=(0.0, 0.0, 0.0), norm=(1 / 255.0,) * 3, stream=None, matrix=0):
        """one forward of mixed-size NV12 frames (ffgpu_exec_forward_nv12_frames_dev): frames is a sequence of (y_ptr, uv_ptr or 0, w, h[, pitch_y,
        pitch_uv, matrix]) tuples or (Y, UV) pairs of torch.uint8 device tensors (Y: h x pitch_y, UV: ceil(h / 2) x pitch_uv); `matrix` (YUV_*) is
        the matrix of every frame that names none"""
        arr = (Nv12Frame * max(1, len(frames)))()
        for k, f in enumerate(frames):
            arr[k] = Nv12Frame(*nv12_frame_desc(f, matrix))
        m, s = (C.c_float * 3)(*mean), (C.c_float * 3)(*norm)
        _check(lib().ffgpu_exec_forward_nv12_frames_dev(self.h, arr, len(frames), m, s, stream), "ffgpu_exec_forward_nv12_frames_dev")

    def dets_dev(self):
        ptr, nbytes = C.c_void_p(), C.c_size_t()
        _check(lib().ffgpu_exec_dets_dev(self.h, C.byref(ptr), C.byref(nbytes)), "ffgpu_exec_dets_dev")
        return ptr.value, nbytes.value

    def dets_host(self):
        """numpy view of the pinned host mirror (FFGPU.HOST_DETS executors); valid after the stream is synchronised"""
        ptr = lib().ffgpu_exec_dets_host(self.h)
        if not ptr:
            raise RuntimeError("ffgpu_exec_dets_host: " + last_error())
        buf = (C.c_char * (DETS_DTYPE.itemsize * self.batch)).from_address(ptr)
        return np.frombuffer(buf, DETS_DTYPE, self.batch)

    def set_ring(self, dev_ptr, slots, slot_records=None):
        """forward k also writes its records into slot k % slots of the device buffer at dev_ptr (None detaches);
        slot_records: distance between slots in records (default: the batch)"""
        if slot_records is None:
            _check(lib().ffgpu_exec_set_ring(self.h, dev_ptr, slots), "ffgpu_exec_set_ring")
        else:
            _check(lib().ffgpu_exec_set_ring_strided(self.h, dev_ptr, slots, slot_records), "ffgpu_exec_set_ring_strided")

    def read_dets(self):
        out = np.zeros(self.batch, DETS_DTYPE)
        _check(lib().ffgpu_exec_read_dets(self.h, out.ctypes.data, self.batch), "ffgpu_exec_read_dets")
        return out

    def boxes(self, frame=0, dets=None):
        d = self.read_dets() if dets is None else dets
        return d[frame]["box"][: d[frame]["count"]].copy()

    def read_layer(self, layer, frame=0):
        shape = self.net.out_shape(layer) if layer >= 0 else self.net.input_shape
        out = np.empty(shape, np.float32)
        _check(lib().ffgpu_exec_read_layer(self.h, layer, frame, out.ctypes.data_as(f32p), out.size), "ffgpu_exec_read_layer")
        return out

    def hash_layers(self):
        """one 64-bit hash per layer over the layer's whole batch tensor (0: not materialised); FFGPU.KEEP_ALL executors"""
        out = np.zeros(self.net.layer_num, np.uint64)
        _check(lib().ffgpu_exec_hash_layers(self.h, out.ctypes.data, out.size), "ffgpu_exec_hash_layers")
        return out

    @property
    def cand_capacity(self):
        return lib().ffgpu_exec_cand_capacity(self.h)

    @property
    def graph_captures(self):
        return lib().ffgpu_exec_graph_captures(self.h)

    def read_boxes(self, frame=0):
        """every box of `frame` that survived NMS (the record keeps the first FFGPU.MAX_DET)"""
        out = np.zeros(max(1, self.cand_capacity), BOX_DTYPE)
        n = _check(lib().ffgpu_exec_read_boxes(self.h, frame, out.ctypes.data, out.size), "ffgpu_exec_read_boxes")
        return out[:n].copy()

    def merge_tiles(self, tiles, nimages, stream=None):
        """enqueue the merge of the last forward's boxes per picture behind it (ffgpu_exec_merge_tiles): tiles is one (image, x0, y0) per batch
        entry (image -1: the entry is no tile) or a Tile array"""
        _check(lib().ffgpu_exec_merge_tiles(self.h, tile_table(tiles), len(tiles), nimages, stream), "ffgpu_exec_merge_tiles")
        self._cap_merged = self.cand_capacity * len(tiles)

    def merged_dev(self):
        ptr, nbytes = C.c_void_p(), C.c_size_t()
        _check(lib().ffgpu_exec_merged_dev(self.h, C.byref(ptr), C.byref(nbytes)), "ffgpu_exec_merged_dev")
        return ptr.value, nbytes.value

    def read_merged(self, nimages):
        out = np.zeros(max(1, nimages), DETS_DTYPE)
        n = _check(lib().ffgpu_exec_read_merged(self.h, out.ctypes.data, nimages), "ffgpu_exec_read_merged")
        return out[:n]

    def read_merged_boxes(self, image=0):
        """every box of picture `image` that survived the merge (the merged record keeps the first FFGPU.MAX_DET)"""
        out = np.zeros(max(1, getattr(self, "_cap_merged", 0)), BOX_DTYPE)
        n = _check(lib().ffgpu_exec_read_merged_boxes(self.h, image, out.ctypes.data, out.size), "ffgpu_exec_read_merged_boxes")
        return out[:n].copy()

    def draw_bgr(self, frames, which=0, color=(0, 255, 0), palette=None, thickness=1, stream=None):
        """enqueue the outlines of the last forward's boxes (which = DRAW_ENTRIES: entry n into frames[n]) or of the last merge's (DRAW_MERGED:
        picture g into frames[g]) behind it (ffgpu_exec_draw_bgr): frames as forward_bgr_frames_dev takes them (None, or a NULL address: skipped),
        colours as B G R bytes (draw_style)"""
        arr = bgr_frame_table(frames)
        _check(lib().ffgpu_exec_draw_bgr(self.h, which, arr, len(frames), draw_style(color, palette, thickness), stream), "ffgpu_exec_draw_bgr")

    def draw_nv12(self, frames, which=0, color=(0, 255, 0), palette=None, thickness=1, stream=None):
        """the same into NV12 frames (ffgpu_exec_draw_nv12): frames as forward_nv12_frames_dev takes them, colours as Y U V bytes"""
        arr = nv12_frame_table(frames)
        _check(lib().ffgpu_exec_draw_nv12(self.h, which, arr, len(frames), draw_style(color, palette, thickness), stream), "ffgpu_exec_draw_nv12")

    def redact_bgr(self, frames, spec, which=0, stream=None):
        """enqueue the redaction of the last forward's boxes (which = REDACT_ENTRIES: entry n in frames[n]) or of the last merge's (REDACT_MERGED:
        picture g in frames[g]) behind it (ffgpu_exec_redact_bgr): frames as draw_bgr takes them, spec from redact_spec.  Redact before draw."""
        _check(lib().ffgpu_exec_redact_bgr(self.h, which, bgr_frame_table(frames), len(frames), spec, stream), "ffgpu_exec_redact_bgr")

    def blur_bgr(self, frames, scratch, spec, which=0, stream=None):
        """enqueue the blur of the last forward's boxes (which = BLUR_ENTRIES) or of the last merge's (BLUR_MERGED) behind it (ffgpu_exec_blur_bgr):
        frames as redact_bgr takes them, scratch one surface of the same w x h per frame (None where the frame is), spec from blur_spec.  Blur
        before draw."""
        if len(scratch) != len(frames):
            raise ValueError("blur_bgr: %d scratch surfaces for %d frames" % (len(scratch), len(frames)))
        _check(lib().ffgpu_exec_blur_bgr(self.h, which, bgr_frame_table(frames), bgr_frame_table(scratch), len(frames), spec, stream), "ffgpu_exec_blur_bgr")

    def blur_nv12(self, frames, scratch, spec, which=0, stream=None):
        """the same in NV12 frames (ffgpu_exec_blur_nv12): chroma is blurred with radius (radius + 1) / 2"""
        if len(scratch) != len(frames):
            raise ValueError("blur_nv12: %d scratch surfaces for %d frames" % (len(scratch), len(frames)))
        _check(lib().ffgpu_exec_blur_nv12(self.h, which, nv12_frame_table(frames), nv12_frame_table(scratch), len(frames), spec, stream), "ffgpu_exec_blur_nv12")

    def redact_nv12(self, frames, spec, which=0, stream=None):
        """the same in NV12 frames (ffgpu_exec_redact_nv12): the spec's colour is Y U V bytes, its cell even"""
        _check(lib().ffgpu_exec_redact_nv12(self.h, which, nv12_frame_table(frames), len(frames), spec, stream), "ffgpu_exec_redact_nv12")

    def crop_bgr(self, frames, spec, d_out, d_table, capacity, which=0, stream=None):
        """enqueue the cut of the last forward's boxes (which = CROP_ENTRIES: entry n out of frames[n]) or of the last merge's (CROP_MERGED: picture
        g out of frames[g]) behind it (ffgpu_exec_crop_bgr): frames as forward_bgr_frames_dev takes them (None, or a NULL address: skipped), spec
        from crop_spec, d_out / d_table the caller's device buffers of capacity slots (crop_slot_bytes) and crop_table_bytes(capacity) bytes"""
        _check(lib().ffgpu_exec_crop_bgr(self.h, which, bgr_frame_table(frames), len(frames), spec, d_out, d_table, capacity, stream), "ffgpu_exec_crop_bgr")

    def crop_nv12(self, frames, spec, d_out, d_table, capacity, which=0, stream=None, matrix=0):
        """the same out of NV12 frames (ffgpu_exec_crop_nv12): frames as forward_nv12_frames_dev takes them"""
        _check(lib().ffgpu_exec_crop_nv12(self.h, which, nv12_frame_table(frames, matrix), len(frames), spec, d_out, d_table, capacity, stream), "ffgpu_exec_crop_nv12")

    def track(self, streams, spec, d_state, nstreams, d_ids, d_out_records=None, d_out_lists=None, which=0, stream=None):
        """enqueue the tracker on the last forward's boxes (which = TRACK_ENTRIES: entry n is record n of video stream streams[n], -1: ignored) or on
        the last merge's (TRACK_MERGED: picture g) behind it (ffgpu_exec_track): spec from track_spec, d_state / d_ids / d_out_* the caller's device
        buffers (track_state_bytes; rows of 8 + S ints; records; lists of S boxes, S as include/ffcnn_hip.h states it)"""
        arr = (C.c_int * max(1, len(streams)))(*[int(v) for v in streams])
        _check(lib().ffgpu_exec_track(self.h, which, arr, len(streams), spec, d_state, nstreams, d_ids, d_out_records, d_out_lists, stream), "ffgpu_exec_track")

    def zones(self, streams, spec, d_scenes, d_state, nstreams, d_events, d_ids=None, d_out_records=None, d_out_lists=None, which=0, stream=None):
        """enqueue the zones pass on the last forward's boxes (which = ZONES_ENTRIES: entry n is record n of video stream streams[n], -1: ignored) or on
        the last merge's (ZONES_MERGED: picture g) behind it (ffgpu_exec_zones): spec from zones_spec, d_scenes nstreams uploaded Scenes, d_state /
        d_events / d_out_* the caller's device buffers (zones_state_bytes; rows of ZONES_ROW + 2 S ints; records; lists of S boxes), d_ids the rows
        Executor.track wrote for the same `which` (with identity ZONES_IDS)"""
        arr = (C.c_int * max(1, len(streams)))(*[int(v) for v in streams])
        _check(lib().ffgpu_exec_zones(self.h, which, arr, len(streams), spec, d_scenes, d_state, nstreams, d_ids, d_events, d_out_records, d_out_lists, stream),
               "ffgpu_exec_zones")

    def heat(self, streams, spec, d_state, nstreams, d_rows, which=0, stream=None):
        """enqueue the heat accumulate pass on the last forward's boxes (which = HEAT_ENTRIES: entry n is record n of video stream streams[n], -1:
        ignored) or on the last merge's (HEAT_MERGED: picture g) behind it (ffgpu_exec_heat): spec from heat_spec, d_state / d_rows the caller's device
        buffers (heat_state_bytes; rows of HEAT_ROW ints).  heat_blend_bgr_dev / _nv12_dev show the state in the frames."""
        arr = (C.c_int * max(1, len(streams)))(*[int(v) for v in streams])
        _check(lib().ffgpu_exec_heat(self.h, which, arr, len(streams), spec, d_state, nstreams, d_rows, stream), "ffgpu_exec_heat")

    def motion_gate(self, streams, spec, d_state, nstreams, d_words, d_out_records=None, d_out_lists=None, which=0, stream=None):
        """enqueue the motion gate on the last forward's boxes (which = MOTION_ENTRIES: entry n is record n of video stream streams[n], -1: ignored) or
        on the last merge's (MOTION_MERGED: picture g) behind it (ffgpu_exec_motion_gate): spec from motion_spec, d_state what motion_update_*_dev
        keeps (only read), d_words rows of MOTION_WORDS + 2 S ints, the gated records and lists optional and the caller's."""
        arr = (C.c_int * max(1, len(streams)))(*[int(v) for v in streams])
        _check(lib().ffgpu_exec_motion_gate(self.h, which, arr, len(streams), spec, d_state, nstreams, d_words, d_out_records, d_out_lists, stream), "ffgpu_exec_motion_gate")

    def trails(self, streams, spec, d_state, nstreams, d_rows, d_ids=None, d_items=None, items_stride=0, first_item=0, nitems=0, which=0, stream=None):
        """enqueue the trails pass on the last forward's boxes (which = TRAILS_ENTRIES: entry n is record n of video stream streams[n], -1: ignored) or
        on the last merge's (TRAILS_MERGED: picture g) behind it (ffgpu_exec_trails): spec from trails_spec, d_state / d_rows / d_items the caller's
        device buffers (trails_state_bytes; rows of TRAILS_ROW + 4 S ints; rows of items_stride segment items), d_ids the rows Executor.track wrote for
        the same `which` (with identity ZONES_IDS)"""
        arr = (C.c_int * max(1, len(streams)))(*[int(v) for v in streams])
        _check(lib().ffgpu_exec_trails(self.h, which, arr, len(streams), spec, d_state, nstreams, d_ids, d_rows, d_items, items_stride, first_item, nitems, stream),
               "ffgpu_exec_trails")

    def caption_bgr(self, frames, spec, d_items, items_stride, d_ids=None, d_font=None, which=0, stream=None):
        """enqueue the captions of the last forward's boxes (which = CAPTION_ENTRIES: entry n into frames[n]) or of the last merge's (CAPTION_MERGED:
        picture g into frames[g]) behind it (ffgpu_exec_caption_bgr): frames as draw_bgr takes them, spec from caption_spec, d_items the caller's
        device buffer of len(frames) x items_stride x 64 bytes (it holds the composed items afterwards), d_ids the rows Executor.track wrote for the
        same `which` (with identity ZONES_IDS), d_font 2 048 device bytes or None: the built-in font.  Redact, then draw, then caption."""
        _check(lib().ffgpu_exec_caption_bgr(self.h, which, bgr_frame_table(frames), len(frames), spec, d_ids, d_items, items_stride, d_font, stream),
               "ffgpu_exec_caption_bgr")

    def caption_nv12(self, frames, spec, d_items, items_stride, d_ids=None, d_font=None, which=0, stream=None):
        """the same into NV12 frames (ffgpu_exec_caption_nv12): the spec's colours are Y U V bytes"""
        _check(lib().ffgpu_exec_caption_nv12(self.h, which, nv12_frame_table(frames), len(frames), spec, d_ids, d_items, items_stride, d_font, stream),
               "ffgpu_exec_caption_nv12")

    def feature_dim(self, spec):
        """D of the rows Executor.features writes for `spec` (a FeatureSpec from feature_spec); pure host code (ffgpu_exec_feature_dim)"""
        return _check(lib().ffgpu_exec_feature_dim(self.h, spec), "ffgpu_exec_feature_dim")

    def features(self, spec, d_out, out_stride=None, stream=None):
        """enqueue the rows of the last forward's tensor behind it (ffgpu_exec_features): spec from feature_spec (layer -1: the tensor the last layer
        leaves), d_out the caller's device buffer of batch rows, out_stride floats apart (default: D); returns D"""
        d = self.feature_dim(spec)
        _check(lib().ffgpu_exec_features(self.h, spec, d_out, d if out_stride is None else out_stride, stream), "ffgpu_exec_features")
        return d

    def relabel(self, d_table, capacity, d_labels, k, spec, d_out_records, d_out_lists=None, which=0, ntargets=None, stream=None):
        """enqueue the relabelling of the last forward's records and lists (which = RELABEL_ENTRIES; ntargets = the batch) or of the last merge's
        (RELABEL_MERGED; ntargets = its pictures) behind it (ffgpu_exec_relabel): d_table the crop table these records' crops were cut with, d_labels
        its slots' top-k rows of k Label each, spec from relabel_spec, d_out_* the caller's device buffers (records; lists of S boxes, S as
        include/ffcnn_hip.h states it)"""
        n = self.batch if ntargets is None else ntargets
        _check(lib().ffgpu_exec_relabel(self.h, which, d_table, capacity, d_labels, k, n, spec, d_out_records, d_out_lists, stream), "ffgpu_exec_relabel")

    def read_candidates(self, frame=0):
        out = np.zeros(max(1, self.cand_capacity), BOX_DTYPE)
        n = _check(lib().ffgpu_exec_read_layer(self.h, -2, frame, out.ctypes.data_as(f32p), out.size * 6), "read candidates")
        return out[:n].copy()

    def profile_steps(self, dev_ptr):
        cap = 512
        lay, us = (C.c_int * cap)(), (C.c_float * cap)()
        n = _check(lib().ffgpu_exec_profile_steps(self.h, dev_ptr, lay, us, cap), "ffgpu_exec_profile_steps")
        return [(lay[k], us[k]) for k in range(n)]

    def step_model(self):
        """[(layer, model HBM bytes)] per step of the plan (ffgpu_exec_step_model)"""
        cap = 512
        lay, by = (C.c_int * cap)(), (C.c_double * cap)()
        n = _check(lib().ffgpu_exec_step_model(self.h, lay, by, cap), "ffgpu_exec_step_model")
        return [(lay[k], by[k]) for k in range(n)]

    def profile(self, dev_ptr):
        us = (C.c_float * 8)()
        _check(lib().ffgpu_exec_profile(self.h, dev_ptr, us), "ffgpu_exec_profile")
        return list(us)


def bgr_frame_desc(f):
    """(ptr, w, h, pitch, 0) of one frame for ffgpu_exec_forward_bgr_frames_dev: a (ptr, w, h[, pitch]) tuple, or a torch.uint8 device
    tensor of shape (h, w, 3) (rows may be strided) or (h, pitch) (w = pitch // 3)"""
    if isinstance(f, (tuple, list)):
        ptr, w, h = f[0], f[1], f[2]
        return (ptr, w, h, f[3] if len(f) > 3 else 0, 0)
    import torch
    if f.dtype != torch.uint8:
        raise TypeError("frames must be torch.uint8 tensors, not %s" % f.dtype)
    if not f.is_cuda:
        raise ValueError("frames must be device tensors (the kernels read them on the GPU), not %s ones" % f.device)
    if f.dim() == 3:
        h, w, c = f.shape
        if c != 3 or f.stride(2) != 1 or f.stride(1) != 3:
            raise ValueError("an (h, w, 3) frame needs contiguous pixels (strides (pitch, 3, 1))")
        return (f.data_ptr(), w, h, f.stride(0) if h > 1 else 3 * w, 0)
    if f.dim() == 2:
        h, pitch = f.shape
        if f.stride(1) != 1:
            raise ValueError("an (h, pitch) frame needs contiguous rows")
        return (f.data_ptr(), pitch // 3, h, f.stride(0) if h > 1 else pitch, 0)
    raise ValueError("a frame is (h, w, 3) or (h, pitch)")


def nv12_frame_desc(f, matrix=0):
    """(y, uv, w, h, pitch_y, pitch_uv, matrix, 0) of one frame for ffgpu_exec_forward_nv12_frames_dev: a (y_ptr, uv_ptr or 0, w, h[, pitch_y,
    pitch_uv, matrix]) tuple (uv 0 = y + pitch_y h; pitches 0 = w and 2 ceil(w / 2)), or a (Y, UV) pair of torch.uint8 device tensors: Y of
    shape (h, pitch_y) (w = pitch_y columns), UV of shape (ceil(h / 2), pitch_uv); rows may be strided"""
    if not isinstance(f, (tuple, list)) or not (len(f) == 2 or 4 <= len(f) <= 7):
        raise ValueError("a frame is (y_ptr, uv_ptr or 0, w, h[, pitch_y, pitch_uv, matrix]) or a (Y, UV) pair of torch.uint8 device tensors")
    if len(f) == 2:
        import torch
        Y, UV = f
        if not (isinstance(Y, torch.Tensor) and isinstance(UV, torch.Tensor)):
            raise ValueError("a frame is (y_ptr, uv_ptr or 0, w, h[, pitch_y, pitch_uv, matrix]) or a (Y, UV) pair of torch.uint8 device tensors")
        for t in (Y, UV):
            if t.dtype != torch.uint8:
                raise TypeError("frames must be torch.uint8 tensors, not %s" % t.dtype)
            if not t.is_cuda:
                raise ValueError("frames must be device tensors (the kernels read them on the GPU), not %s ones" % t.device)
            if t.dim() != 2 or t.stride(1) != 1:
                raise ValueError("a plane is (rows, pitch) with contiguous rows")
        h, w = Y.shape
        if UV.shape[0] != (h + 1) // 2 or UV.shape[1] < 2 * ((w + 1) // 2):
            raise ValueError("the UV plane of a %d x %d frame has %d rows of at least %d bytes, not %s" % (w, h, (h + 1) // 2, 2 * ((w + 1) // 2), tuple(UV.shape)))
        return (Y.data_ptr(), UV.data_ptr(), w, h, Y.stride(0) if h > 1 else w, UV.stride(0) if UV.shape[0] > 1 else UV.shape[1] & ~1, matrix, 0)
    y, uv, w, h = f[0], f[1], f[2], f[3]
    return (y, uv or 0, w, h, f[4] if len(f) > 4 else 0, f[5] if len(f) > 5 else 0, f[6] if len(f) > 6 else matrix, 0)


def bgr_frame_table(frames):
    """a BgrFrame array from what bgr_frame_desc accepts; None is a NULL address (a skipped draw target)"""
    arr = (BgrFrame * max(1, len(frames)))()
    for k, f in enumerate(frames):
        arr[k] = BgrFrame(None, 1, 1, 0, 0) if f is None else BgrFrame(*bgr_frame_desc(f))
    return arr


def nv12_frame_table(frames, matrix=0):
    """an Nv12Frame array from what nv12_frame_desc accepts; None is a NULL address (a skipped draw target)"""
    arr = (Nv12Frame * max(1, len(frames)))()
    for k, f in enumerate(frames):
        arr[k] = Nv12Frame(None, None, 1, 1, 0, 0, 0, 0) if f is None else Nv12Frame(*nv12_frame_desc(f, matrix))
    return arr


def draw_style(color=(0, 255, 0), palette=None, thickness=1):
    """a DrawStyle: one colour of three bytes (B G R for BGR targets, Y U V for NV12 ones), or a palette of 1..256 such colours (a sequence of
    triples or an (n, 3 | 4) uint8 array) indexed by the box's class mod its length.  The structure keeps its palette bytes alive."""
    st = DrawStyle()
    st.color[:] = (int(color[0]), int(color[1]), int(color[2]), 0)
    st.thickness = thickness
    if palette is not None:
        pal = np.zeros((len(palette), 4), np.uint8)
        if len(palette):
            pal[:, :3] = np.asarray(palette, np.uint8).reshape(len(palette), -1)[:, :3]
        st._pal = pal                                           # (owned by the structure: the C side reads it during the call)
        st.palette = pal.ctypes.data
        st.npalette = len(palette)
    return st


def _draw_boxes_dev(fn, name, table, d_records, d_lists, list_stride, list_first, frames, style, stream):
    first = None if list_first is None else (C.c_int * max(1, len(list_first)))(*[int(v) for v in list_first])
    _check(fn(d_records, d_lists, list_stride, first, table(frames), len(frames), style if style is not None else draw_style(), stream), name)


def draw_boxes_bgr_dev(d_records, d_lists, list_stride, frames, style=None, list_first=None, stream=None):
    """ffgpu_draw_boxes_bgr_dev on device records / lists: record t outlined in frames[t] (what bgr_frame_desc accepts, or None: skipped);
    d_lists None: the records' own boxes; list_first: the first box of each target's list (default t * list_stride)"""
    _draw_boxes_dev(lib().ffgpu_draw_boxes_bgr_dev, "ffgpu_draw_boxes_bgr_dev", bgr_frame_table, d_records, d_lists, list_stride, list_first, frames, style, stream)


def draw_boxes_nv12_dev(d_records, d_lists, list_stride, frames, style=None, list_first=None, stream=None):
    """ffgpu_draw_boxes_nv12_dev: the same into NV12 frames (what nv12_frame_desc accepts, or None: skipped); colours are Y U V bytes"""
    _draw_boxes_dev(lib().ffgpu_draw_boxes_nv12_dev, "ffgpu_draw_boxes_nv12_dev", nv12_frame_table, d_records, d_lists, list_stride, list_first, frames, style, stream)


def redact_spec(mode, cell=0, outside=False, min_score=0.0, classes=None, margin=(0, 1), color=(0, 0, 0)):
    """a RedactSpec: mode REDACT_FILL (cell 0, color = B G R or Y U V bytes) or REDACT_MOSAIC (cell 2..64, even for NV12 targets); outside: everything
    BUT the regions; classes, min_score and margin as crop_spec.  The structure keeps its class bytes alive."""
    sp = RedactSpec()
    sp.mode, sp.cell, sp.flags, sp.min_score = mode, cell, REDACT_OUTSIDE if outside else 0, min_score
    sp.margin_num, sp.margin_den = margin
    sp.color[:] = (int(color[0]), int(color[1]), int(color[2]), 0)
    if classes is not None:
        cls = np.ascontiguousarray(np.asarray(classes) != 0, np.uint8) if len(classes) else np.zeros(1, np.uint8)
        sp._cls = cls                                           # (owned by the structure: the C side reads it during the call)
        sp.classes = cls.ctypes.data
        sp.nclasses = len(classes)
    return sp


def _redact_boxes_dev(fn, name, table, d_records, d_lists, list_stride, list_first, frames, spec, stream):
    first = None if list_first is None else (C.c_int * max(1, len(list_first)))(*[int(v) for v in list_first])
    _check(fn(d_records, d_lists, list_stride, first, table(frames), len(frames), spec, stream), name)


def redact_boxes_bgr_dev(d_records, d_lists, list_stride, frames, spec, list_first=None, stream=None):
    """ffgpu_redact_boxes_bgr_dev on device records / lists: the regions of record t's qualifying boxes (or everything but them) redacted in
    frames[t] (what bgr_frame_desc accepts, or None: skipped); d_lists None: the records' own boxes; list_first as draw_boxes_bgr_dev"""
    _redact_boxes_dev(lib().ffgpu_redact_boxes_bgr_dev, "ffgpu_redact_boxes_bgr_dev", bgr_frame_table, d_records, d_lists, list_stride, list_first, frames, spec, stream)


def redact_boxes_nv12_dev(d_records, d_lists, list_stride, frames, spec, list_first=None, stream=None):
    """ffgpu_redact_boxes_nv12_dev: the same in NV12 frames (what nv12_frame_desc accepts, or None: skipped)"""
    _redact_boxes_dev(lib().ffgpu_redact_boxes_nv12_dev, "ffgpu_redact_boxes_nv12_dev", nv12_frame_table, d_records, d_lists, list_stride, list_first, frames, spec, stream)


def blur_spec(radius, passes=1, outside=False, min_score=0.0, classes=None, margin=(0, 1)):
    """a BlurSpec: radius 1..31 (the box window is 2 radius + 1 pixels square, clipped to the frame), passes 1..3; outside: everything BUT the
    regions; classes, min_score and margin as redact_spec.  The structure keeps its class bytes alive."""
    sp = BlurSpec()
    sp.radius, sp.passes, sp.flags, sp.min_score = radius, passes, BLUR_OUTSIDE if outside else 0, min_score
    sp.margin_num, sp.margin_den = margin
    if classes is not None:
        cls = np.ascontiguousarray(np.asarray(classes) != 0, np.uint8) if len(classes) else np.zeros(1, np.uint8)
        sp._cls = cls                                           # (owned by the structure: the C side reads it during the call)
        sp.classes = cls.ctypes.data
        sp.nclasses = len(classes)
    return sp


def _blur_boxes_dev(fn, name, table, d_records, d_lists, list_stride, list_first, frames, scratch, spec, stream):
    if len(scratch) != len(frames):
        raise ValueError("%s: %d scratch surfaces for %d frames" % (name, len(scratch), len(frames)))
    first = None if list_first is None else (C.c_int * max(1, len(list_first)))(*[int(v) for v in list_first])
    _check(fn(d_records, d_lists, list_stride, first, table(frames), table(scratch), len(frames), spec, stream), name)


def blur_boxes_bgr_dev(d_records, d_lists, list_stride, frames, scratch, spec, list_first=None, stream=None):
    """ffgpu_blur_boxes_bgr_dev on device records / lists: the regions of record t's qualifying boxes (or everything but them) box-blurred in
    frames[t] through scratch[t] (both what bgr_frame_desc accepts, or None: skipped); d_lists None: the records' own boxes; list_first as
    draw_boxes_bgr_dev"""
    _blur_boxes_dev(lib().ffgpu_blur_boxes_bgr_dev, "ffgpu_blur_boxes_bgr_dev", bgr_frame_table, d_records, d_lists, list_stride, list_first, frames, scratch, spec, stream)


def blur_boxes_nv12_dev(d_records, d_lists, list_stride, frames, scratch, spec, list_first=None, stream=None):
    """ffgpu_blur_boxes_nv12_dev: the same in NV12 frames (what nv12_frame_desc accepts, or None: skipped)"""
    _blur_boxes_dev(lib().ffgpu_blur_boxes_nv12_dev, "ffgpu_blur_boxes_nv12_dev", nv12_frame_table, d_records, d_lists, list_stride, list_first, frames, scratch, spec, stream)


def crop_spec(out_w, out_h, form=CROP_F32, per_target=1, min_score=0.0, classes=None, margin=(0, 1), mean=(0.0, 0.0, 0.0), norm=(1 / 255.0,) * 3):
    """a CropSpec: classes is None (every class) or a sequence of 1..256 flags indexed by the box's class; margin is (num, den).  The structure
    keeps its class bytes alive."""
    sp = CropSpec()
    sp.out_w, sp.out_h, sp.form, sp.per_target, sp.min_score = out_w, out_h, form, per_target, min_score
    sp.margin_num, sp.margin_den = margin
    sp.mean[:], sp.norm[:] = [float(v) for v in mean], [float(v) for v in norm]
    if classes is not None:
        cls = np.ascontiguousarray(np.asarray(classes) != 0, np.uint8) if len(classes) else np.zeros(1, np.uint8)
        sp._cls = cls                                           # (owned by the structure: the C side reads it during the call)
        sp.classes = cls.ctypes.data
        sp.nclasses = len(classes)
    return sp


def crop_table_bytes(capacity):
    return lib().ffgpu_crop_table_bytes(capacity)


def crop_slot_bytes(out_w, out_h, form=CROP_F32):
    return lib().ffgpu_crop_slot_bytes(out_w, out_h, form)


def crop_table(raw):
    """(header dict, entries as a CROP_DTYPE array) of a crop table's bytes (a uint8 array of crop_table_bytes(capacity) bytes)"""
    raw = np.ascontiguousarray(raw, np.uint8).reshape(-1)
    hdr = raw[:16].view("<i4")
    return dict(total=int(hdr[0]), taken=int(hdr[1]), empty=int(hdr[2]), capacity=int(hdr[3])), raw[16:].view(CROP_DTYPE)


def _crop_boxes_dev(fn, name, table, d_records, d_lists, list_stride, list_first, frames, spec, d_out, d_table, capacity, stream):
    first = None if list_first is None else (C.c_int * max(1, len(list_first)))(*[int(v) for v in list_first])
    _check(fn(d_records, d_lists, list_stride, first, table(frames), len(frames), spec, d_out, d_table, capacity, stream), name)


def crop_boxes_bgr_dev(d_records, d_lists, list_stride, frames, spec, d_out, d_table, capacity, list_first=None, stream=None):
    """ffgpu_crop_boxes_bgr_dev on device records / lists: the selected boxes of record t cut out of frames[t] (what bgr_frame_desc accepts, or
    None: skipped) into the slots at d_out, the table at d_table; d_lists None: the records' own boxes; list_first as draw_boxes_bgr_dev"""
    _crop_boxes_dev(lib().ffgpu_crop_boxes_bgr_dev, "ffgpu_crop_boxes_bgr_dev", bgr_frame_table, d_records, d_lists, list_stride, list_first, frames, spec,
                    d_out, d_table, capacity, stream)


def crop_boxes_nv12_dev(d_records, d_lists, list_stride, frames, spec, d_out, d_table, capacity, list_first=None, stream=None):
    """ffgpu_crop_boxes_nv12_dev: the same out of NV12 frames (what nv12_frame_desc accepts, or None: skipped)"""
    _crop_boxes_dev(lib().ffgpu_crop_boxes_nv12_dev, "ffgpu_crop_boxes_nv12_dev", nv12_frame_table, d_records, d_lists, list_stride, list_first, frames, spec,
                    d_out, d_table, capacity, stream)


def crops_to_source_dev(d_table, capacity, d_records, d_lists, list_stride, d_out_records, d_out_lists=None, stream=None):
    """ffgpu_crops_to_source_dev: the records (and full lists) of a forward over the slots back into the sources' coordinates; in place is legal"""
    _check(lib().ffgpu_crops_to_source_dev(d_table, capacity, d_records, d_lists, list_stride, d_out_records, d_out_lists, stream), "ffgpu_crops_to_source_dev")


def track_spec(capacity, max_missed=0, min_hits=1, iou_thresh=0.3, min_score=0.0, birth_score=0.0, class_aware=1):
    """a TrackSpec (ffgpu_track_spec)"""
    sp = TrackSpec()
    sp.capacity, sp.max_missed, sp.min_hits, sp.class_aware = capacity, max_missed, min_hits, int(class_aware)
    sp.iou_thresh, sp.min_score, sp.birth_score = iou_thresh, min_score, birth_score
    return sp


def track_state_bytes(nstreams, capacity):
    return lib().ffgpu_track_state_bytes(nstreams, capacity)


def track_state(raw, nstreams, capacity):
    """([header dict per stream], slots as a TRACK_DTYPE array of nstreams x capacity) of a state's bytes (a uint8 array of track_state_bytes bytes)"""
    raw = np.ascontiguousarray(raw, np.uint8).reshape(nstreams, 16 + 48 * capacity)
    hdr = [dict(zip(("issued", "frames", "live", "reserved"), (int(v) for v in r[:16].view("<i4")))) for r in raw]
    return hdr, np.ascontiguousarray(raw[:, 16:]).view(TRACK_DTYPE).reshape(nstreams, capacity)


def track_reset_dev(d_state, nstreams, capacity, which_stream=-1, stream=None):
    """ffgpu_track_reset_dev: zero the state of one video stream, or of all (-1), in stream order"""
    _check(lib().ffgpu_track_reset_dev(d_state, nstreams, capacity, which_stream, stream), "ffgpu_track_reset_dev")


def track_boxes_dev(d_records, d_lists, list_stride, streams, spec, d_state, nstreams, d_ids, d_out_records=None, d_out_lists=None, list_first=None,
                    stream=None):
    """ffgpu_track_boxes_dev on device records / lists: record t is the next frame of video stream streams[t] (-1: ignored); d_lists None: the
    records' own boxes; list_first as draw_boxes_bgr_dev"""
    first = None if list_first is None else (C.c_int * max(1, len(list_first)))(*[int(v) for v in list_first])
    arr = (C.c_int * max(1, len(streams)))(*[int(v) for v in streams])
    _check(lib().ffgpu_track_boxes_dev(d_records, d_lists, list_stride, first, arr, len(streams), spec, d_state, nstreams, d_ids, d_out_records,
                                       d_out_lists, stream), "ffgpu_track_boxes_dev")


def class_mask(classes=None):
    """the four words of a zone's or a line's class mask: None (or nothing): every class, else a bit per class 0..127"""
    m = [0, 0, 0, 0]
    for c in classes or ():
        if not 0 <= int(c) < 128:
            raise ValueError("class %r is outside 0..127" % (c,))
        m[int(c) >> 5] |= 1 << (int(c) & 31)
    return m


def scene(zones=(), lines=(), anchor=0):
    """a Scene (ffgpu_scene): zones = [(vertices [(x, y), ...][, dwell_frames[, classes]]), ...], lines = [((ax, ay), (bx, by)[, classes]), ...],
    anchor 0: the box's centre, 1: its bottom centre"""
    if len(zones) > SCENE_ZONES or len(lines) > SCENE_LINES:
        raise ValueError("a scene holds %d zones and %d lines at most" % (SCENE_ZONES, SCENE_LINES))
    sc = Scene()
    sc.nzones, sc.nlines, sc.anchor = len(zones), len(lines), anchor
    for z, zn in enumerate(zones):
        verts = zn[0]
        if len(verts) > ZONE_VERTS:
            raise ValueError("zone %d: %d vertices (%d at most)" % (z, len(verts), ZONE_VERTS))
        sc.zone[z].nverts, sc.zone[z].dwell_frames = len(verts), zn[1] if len(zn) > 1 else 0
        for k, (x, y) in enumerate(verts):
            sc.zone[z].x[k], sc.zone[z].y[k] = x, y
        sc.zone[z].classes[:] = class_mask(zn[2] if len(zn) > 2 else None)
    for l, ln in enumerate(lines):
        (sc.line[l].ax, sc.line[l].ay), (sc.line[l].bx, sc.line[l].by) = ln[0], ln[1]
        sc.line[l].classes[:] = class_mask(ln[2] if len(ln) > 2 else None)
    return sc


def scene_check(scenes):
    """ffgpu_scene_check on a list of Scenes (pure host code): raises with what is wrong with the first bad one"""
    arr = (Scene * max(1, len(scenes)))(*scenes)
    _check(lib().ffgpu_scene_check(arr, len(scenes)), "ffgpu_scene_check")


def scenes_bytes(scenes):
    """the bytes to upload as d_scenes: the Scenes one after the other"""
    return b"".join(bytes(s) for s in scenes)


def zones_spec(capacity, max_missed=0, identity=ZONES_IDS, min_score=0.0, gate_zone=0, gate_line=0, invert=False):
    """a ZonesSpec (ffgpu_zones_spec)"""
    sp = ZonesSpec()
    sp.capacity, sp.max_missed, sp.identity, sp.flags = capacity, max_missed, identity, ZONES_GATE_INVERT if invert else 0
    sp.min_score, sp.gate_zone, sp.gate_line = min_score, gate_zone, gate_line
    return sp


def zones_state_bytes(nstreams, capacity):
    return lib().ffgpu_zones_state_bytes(nstreams, capacity)


def zones_state(raw, nstreams, capacity):
    """([header dict per stream], slots as a ZONE_SLOT_DTYPE array of nstreams x capacity) of a state's bytes (a uint8 array of zones_state_bytes bytes)"""
    raw = np.ascontiguousarray(raw, np.uint8).reshape(nstreams, ZONES_STATE_HEADER + 64 * capacity)
    hdr = []
    for r in raw:
        w = np.ascontiguousarray(r[:ZONES_STATE_HEADER]).view("<u4")
        hdr.append(dict(frames=int(w[0]), live=int(w[1]), total_entered=[int(v) for v in w[4:12]], total_left=[int(v) for v in w[12:20]],
                        total_fwd=[int(v) for v in w[20:28]], total_back=[int(v) for v in w[28:36]]))
    return hdr, np.ascontiguousarray(raw[:, ZONES_STATE_HEADER:]).view(ZONE_SLOT_DTYPE).reshape(nstreams, capacity)


def zones_reset_dev(d_state, nstreams, capacity, which_stream=-1, stream=None):
    """ffgpu_zones_reset_dev: zero the state of one video stream, or of all (-1), in stream order"""
    _check(lib().ffgpu_zones_reset_dev(d_state, nstreams, capacity, which_stream, stream), "ffgpu_zones_reset_dev")


def zones_boxes_dev(d_records, d_lists, list_stride, streams, spec, d_scenes, d_state, nstreams, d_events, d_ids=None, d_out_records=None, d_out_lists=None,
                    list_first=None, stream=None):
    """ffgpu_zones_boxes_dev on device records / lists: record t is the next frame of video stream streams[t] (-1: ignored); d_lists None: the
    records' own boxes; list_first as draw_boxes_bgr_dev; d_ids: the rows track_boxes_dev wrote (with identity ZONES_IDS)"""
    first = None if list_first is None else (C.c_int * max(1, len(list_first)))(*[int(v) for v in list_first])
    arr = (C.c_int * max(1, len(streams)))(*[int(v) for v in streams])
    _check(lib().ffgpu_zones_boxes_dev(d_records, d_lists, list_stride, first, arr, len(streams), spec, d_scenes, d_state, nstreams, d_ids, d_events,
                                       d_out_records, d_out_lists, stream), "ffgpu_zones_boxes_dev")


def font_builtin():
    """the built-in font's 2 048 bytes as a (256, 8) uint8 array: row r of glyph g, bit 7 - c = column c (ffgpu_font_builtin; pure host code)"""
    out = np.zeros((256, 8), np.uint8)
    lib().ffgpu_font_builtin(out.ctypes.data)
    return out


def text_items(items, stride=None):
    """TEXT_ITEM_DTYPE rows for one target from (x, y, text[, fg, bg, scale, opaque]) tuples, text a str (its characters' codes) or bytes; padded with
    unused slots (len 0) to `stride` rows"""
    out = np.zeros(len(items) if stride is None else stride, TEXT_ITEM_DTYPE)
    if len(items) > len(out):
        raise ValueError("%d items for a stride of %d" % (len(items), len(out)))
    for k, it in enumerate(items):
        x, y, text = it[0], it[1], it[2]
        fg, bg, scale, opaque = (tuple(it[3:]) + ((255, 255, 255), (0, 0, 0), 1, False)[len(it) - 3:])[:4]
        raw = text.encode("latin-1") if isinstance(text, str) else bytes(text)
        if len(raw) > TEXT_MAX:
            raise ValueError("a text item holds %d characters, not %d" % (TEXT_MAX, len(raw)))
        out[k]["x"], out[k]["y"], out[k]["scale"], out[k]["flags"], out[k]["len"] = x, y, scale, TEXT_OPAQUE if opaque else 0, len(raw)
        out[k]["fg"][:3], out[k]["bg"][:3] = fg[:3], bg[:3]
        out[k]["text"][:len(raw)] = np.frombuffer(raw, np.uint8)
    return out


def caption_spec(name=True, score=True, ident=False, opaque=True, min_score=0.0, identity=ZONES_NONE, scale=1, fg=(255, 255, 255), color=(0, 0, 0), palette=None,
                 d_names=None, nnames=0):
    """a CaptionSpec: which parts a caption has, from which score on, where the id comes from (ZONES_NONE | _TYPE | _IDS), the ink `fg` and the paper:
    one colour or a palette as draw_style takes it (B G R bytes for BGR targets, Y U V for NV12 ones); d_names: nnames rows of 16 device bytes.  The
    structure keeps its palette bytes alive."""
    sp = CaptionSpec()
    sp.min_score, sp.identity, sp.scale = min_score, identity, scale
    sp.flags = (CAPTION_NAME if name else 0) | (CAPTION_SCORE if score else 0) | (CAPTION_ID if ident else 0) | (CAPTION_OPAQUE if opaque else 0)
    sp.fg[:] = (int(fg[0]), int(fg[1]), int(fg[2]), 0)
    sp.color[:] = (int(color[0]), int(color[1]), int(color[2]), 0)
    if palette is not None:
        pal = np.zeros((len(palette), 4), np.uint8)
        if len(palette):
            pal[:, :3] = np.asarray(palette, np.uint8).reshape(len(palette), -1)[:, :3]
        sp._pal = pal                                           # (owned by the structure: the C side reads it during the call)
        sp.palette = pal.ctypes.data
        sp.npalette = len(palette)
    sp.d_names, sp.nnames = d_names, nnames
    return sp


def names_bytes(names):
    """the rows of 16 bytes ffgpu_caption_spec.d_names points to, for the caller to upload: a NUL ends a name shorter than 16 bytes"""
    out = np.zeros((len(names), 16), np.uint8)
    for k, nm in enumerate(names):
        raw = (nm.encode("latin-1") if isinstance(nm, str) else bytes(nm))[:16]
        out[k, :len(raw)] = np.frombuffer(raw, np.uint8)
    return out


def draw_text_bgr_dev(d_items, items_stride, frames, d_font=None, stream=None):
    """ffgpu_draw_text_bgr_dev: items t * items_stride ... of d_items rasterised into frames[t] (what bgr_frame_desc accepts, or None: skipped);
    d_font 2 048 device bytes, or None: the built-in font"""
    _check(lib().ffgpu_draw_text_bgr_dev(d_items, items_stride, d_font, bgr_frame_table(frames), len(frames), stream), "ffgpu_draw_text_bgr_dev")


def draw_text_nv12_dev(d_items, items_stride, frames, d_font=None, stream=None):
    """ffgpu_draw_text_nv12_dev: the same into NV12 frames (what nv12_frame_desc accepts, or None: skipped); colours are Y U V bytes"""
    _check(lib().ffgpu_draw_text_nv12_dev(d_items, items_stride, d_font, nv12_frame_table(frames), len(frames), stream), "ffgpu_draw_text_nv12_dev")


def caption_boxes_dev(d_records, d_lists, list_stride, ntargets, spec, d_items, items_stride, d_ids=None, list_first=None, stream=None):
    """ffgpu_caption_boxes_dev on device records / lists: the captions of record t composed into items t * items_stride ... of d_items; spec from
    caption_spec, d_ids the rows track_boxes_dev wrote (with identity ZONES_IDS); the other arguments as draw_boxes_bgr_dev takes them"""
    first = None if list_first is None else (C.c_int * max(1, len(list_first)))(*[int(v) for v in list_first])
    _check(lib().ffgpu_caption_boxes_dev(d_records, d_lists, list_stride, first, ntargets, spec, d_ids, d_items, items_stride, stream), "ffgpu_caption_boxes_dev")


def caption_scene_dev(d_scenes, d_state, nstreams, capacity, d_events, events_stride, streams, spec, d_items, items_stride, stream=None):
    """ffgpu_caption_scene_dev: the zones' occupancies (event row t) and the lines' totals (the state of stream streams[t]) as items t * items_stride ...
    of d_items (items_stride 16..256); spec from caption_spec (its colours and scale); draw them with draw_text_*_dev"""
    arr = (C.c_int * max(1, len(streams)))(*[int(v) for v in streams])
    _check(lib().ffgpu_caption_scene_dev(d_scenes, d_state, nstreams, capacity, d_events, events_stride, arr, len(streams), spec, d_items, items_stride, stream),
           "ffgpu_caption_scene_dev")


def seg_items(items, stride=None):
    """SEG_ITEM_DTYPE rows for one target from (x0, y0, x1, y1[, color, thickness, dash]) tuples; padded with unused slots (thickness 0) to `stride`
    rows"""
    out = np.zeros(len(items) if stride is None else stride, SEG_ITEM_DTYPE)
    if len(items) > len(out):
        raise ValueError("%d items for a stride of %d" % (len(items), len(out)))
    for k, it in enumerate(items):
        color, thickness, dash = (tuple(it[4:]) + ((255, 255, 255), 1, 0)[len(it) - 4:])[:3]
        out[k]["x0"], out[k]["y0"], out[k]["x1"], out[k]["y1"], out[k]["thickness"], out[k]["dash"] = it[0], it[1], it[2], it[3], thickness, dash
        out[k]["color"][:3] = color[:3]
    return out


def outline_spec(zones=True, lines=True, ticks=False, markers=False, alarm_on=False, thickness=1, line_dash=0, marker=0, color=(0, 0, 0), alarm=(0, 0, 255),
                 palette=None):
    """an OutlineSpec: which parts of a scene become segments (the zones' edges, the lines' shafts, their forward ticks, the anchors' crosses; alarm_on:
    a loitered zone takes the colour `alarm`), how thick, the shafts' dash, the crosses' arm length, and the colours: one colour or a palette as
    draw_style takes it (B G R bytes for BGR targets, Y U V for NV12 ones).  The structure keeps its palette bytes alive."""
    sp = OutlineSpec()
    sp.flags = ((OUTLINE_ZONES if zones else 0) | (OUTLINE_LINES if lines else 0) | (OUTLINE_TICKS if ticks else 0) | (OUTLINE_MARKERS if markers else 0) |
                (OUTLINE_ALARM if alarm_on else 0))
    sp.thickness, sp.line_dash, sp.marker = thickness, line_dash, marker
    sp.color[:] = (int(color[0]), int(color[1]), int(color[2]), 0)
    sp.alarm[:] = (int(alarm[0]), int(alarm[1]), int(alarm[2]), 0)
    if palette is not None:
        pal = np.zeros((len(palette), 4), np.uint8)
        if len(palette):
            pal[:, :3] = np.asarray(palette, np.uint8).reshape(len(palette), -1)[:, :3]
        sp._pal = pal                                           # (owned by the structure: the C side reads it during the call)
        sp.palette = pal.ctypes.data
        sp.npalette = len(palette)
    return sp


def outline_spec_check(spec):
    """ffgpu_outline_spec_check (pure host code): raises with what is wrong with the spec"""
    _check(lib().ffgpu_outline_spec_check(spec), "ffgpu_outline_spec_check")


def draw_segments_bgr_dev(d_items, items_stride, frames, stream=None):
    """ffgpu_draw_segments_bgr_dev: items t * items_stride ... of d_items (SEG_ITEM_DTYPE rows) rasterised into frames[t] (what bgr_frame_desc accepts, or
    None: skipped)"""
    _check(lib().ffgpu_draw_segments_bgr_dev(d_items, items_stride, bgr_frame_table(frames), len(frames), stream), "ffgpu_draw_segments_bgr_dev")


def draw_segments_nv12_dev(d_items, items_stride, frames, stream=None):
    """ffgpu_draw_segments_nv12_dev: the same into NV12 frames (what nv12_frame_desc accepts, or None: skipped); colours are Y U V bytes"""
    _check(lib().ffgpu_draw_segments_nv12_dev(d_items, items_stride, nv12_frame_table(frames), len(frames), stream), "ffgpu_draw_segments_nv12_dev")


def outline_scene_dev(d_scenes, d_state, nstreams, capacity, d_events, events_stride, streams, spec, d_items, items_stride, stream=None):
    """ffgpu_outline_scene_dev: the zones' edges, the lines' shafts and ticks and the anchors' crosses of stream streams[t] (scene, event row t, state)
    as items t * items_stride ... of d_items (items_stride 80..512); spec from outline_spec; draw them with draw_segments_*_dev"""
    arr = (C.c_int * max(1, len(streams)))(*[int(v) for v in streams])
    _check(lib().ffgpu_outline_scene_dev(d_scenes, d_state, nstreams, capacity, d_events, events_stride, arr, len(streams), spec, d_items, items_stride, stream),
           "ffgpu_outline_scene_dev")


def trails_spec(capacity, max_missed=0, identity=ZONES_IDS, min_score=0.0, anchor=0, points=TRAIL_POINTS, min_move=0, thickness=1, coast=False, taper=False,
                coast_dash=0, color=(0, 0, 0), palette=None):
    """a TrailsSpec (ffgpu_trails_spec): slots per stream, how long an unseen object is kept, where the identity comes from (ZONES_TYPE | _IDS), the
    anchor (0: centre, 1: bottom centre), the history kept per object, the distance from which a point is appended, and how the trail is drawn: one
    colour or a palette as draw_style takes it.  The structure keeps its palette bytes alive."""
    sp = TrailsSpec()
    sp.capacity, sp.max_missed, sp.identity, sp.flags = capacity, max_missed, identity, (TRAILS_COAST if coast else 0) | (TRAILS_TAPER if taper else 0)
    sp.min_score, sp.anchor, sp.points, sp.min_move, sp.thickness, sp.coast_dash = min_score, anchor, points, min_move, thickness, coast_dash
    sp.color[:] = (int(color[0]), int(color[1]), int(color[2]), 0)
    if palette is not None:
        pal = np.zeros((len(palette), 4), np.uint8)
        if len(palette):
            pal[:, :3] = np.asarray(palette, np.uint8).reshape(len(palette), -1)[:, :3]
        sp._pal = pal                                           # (owned by the structure: the C side reads it during the call)
        sp.palette = pal.ctypes.data
        sp.npalette = len(palette)
    return sp


def trails_spec_check(spec):
    """ffgpu_trails_spec_check (pure host code): raises with what is wrong with the spec"""
    _check(lib().ffgpu_trails_spec_check(spec), "ffgpu_trails_spec_check")


def trails_state_bytes(nstreams, capacity):
    return lib().ffgpu_trails_state_bytes(nstreams, capacity)


def trails_state(raw, nstreams, capacity):
    """(headers as an int array of nstreams x 4: frames, live, reserved x 2; slots as a TRAIL_SLOT_DTYPE array of nstreams x capacity) of a state's bytes"""
    raw = np.ascontiguousarray(raw, np.uint8).reshape(nstreams, TRAILS_STATE_HEADER + 416 * capacity)
    return (np.ascontiguousarray(raw[:, :TRAILS_STATE_HEADER]).view("<i4"),
            np.ascontiguousarray(raw[:, TRAILS_STATE_HEADER:]).view(TRAIL_SLOT_DTYPE).reshape(nstreams, capacity))


def trails_reset_dev(d_state, nstreams, capacity, which_stream=-1, stream=None):
    """ffgpu_trails_reset_dev: zero the trails state of one video stream, or of all (-1), in stream order"""
    _check(lib().ffgpu_trails_reset_dev(d_state, nstreams, capacity, which_stream, stream), "ffgpu_trails_reset_dev")


def trails_boxes_dev(d_records, d_lists, list_stride, streams, spec, d_state, nstreams, d_rows, d_ids=None, d_items=None, items_stride=0, first_item=0, nitems=0,
                     list_first=None, stream=None):
    """ffgpu_trails_boxes_dev on device records / lists: record t is the next frame of video stream streams[t] (-1: ignored); d_lists None: the
    records' own boxes; list_first as draw_boxes_bgr_dev; d_ids: the rows track_boxes_dev wrote (with identity ZONES_IDS); d_rows: rows of
    TRAILS_ROW + 4 S ints; d_items: rows of items_stride SEG_ITEM_DTYPE items of which first_item .. first_item + nitems - 1 are written, or None"""
    arr = (C.c_int * max(1, len(streams)))(*[int(v) for v in streams])
    first = None if list_first is None else (C.c_int * max(1, len(list_first)))(*[int(v) for v in list_first])
    _check(lib().ffgpu_trails_boxes_dev(d_records, d_lists, list_stride, first, arr, len(streams), spec, d_state, nstreams, d_ids, d_rows, d_items, items_stride,
                                        first_item, nitems, stream), "ffgpu_trails_boxes_dev")


def heat_spec(gw, gh, cell_log2, mode=HEAT_ANCHOR, anchor=0, spread=0, gain=1, decay_shift=0, min_score=0.0, classes=None):
    """a HeatSpec (ffgpu_heat_spec): the grid (gw x gh cells of 1 << cell_log2 pixels), the footprint of a box (HEAT_ANCHOR: the cells within `spread`
    of the anchor's, 0: centre, 1: bottom centre; HEAT_BOX: every cell the box touches), what a box adds, the decay per frame (a shift, 0: none) and
    which boxes qualify (min_score, classes as redact_spec).  The structure keeps its class bytes alive."""
    sp = HeatSpec()
    sp.gw, sp.gh, sp.cell_log2, sp.mode, sp.anchor, sp.spread, sp.gain, sp.decay_shift, sp.min_score = gw, gh, cell_log2, mode, anchor, spread, gain, decay_shift, min_score
    if classes is not None:
        cls = np.ascontiguousarray(np.asarray(classes) != 0, np.uint8) if len(classes) else np.zeros(1, np.uint8)
        sp._cls = cls                                           # (owned by the structure: the C side reads it during the call)
        sp.classes = cls.ctypes.data
        sp.nclasses = len(classes)
    return sp


def heat_blend_spec(gw, gh, cell_log2, full_scale=0, floor=0, opacity=128, smooth=False, ramp_alpha=False, palette=None):
    """a HeatBlendSpec (ffgpu_heat_blend_spec): the grid's geometry, the cell value shown as level 255 (0: the stream's peak), the level below which
    a pixel stays, the opacity, the sampling and a palette of 256 colours (B G R for BGR targets, Y U V for NV12 ones; a (256, 3 | 4) uint8 array) or
    None: the built-in one.  The structure keeps its palette bytes alive."""
    sp = HeatBlendSpec()
    sp.gw, sp.gh, sp.cell_log2, sp.full_scale, sp.floor, sp.opacity = gw, gh, cell_log2, full_scale, floor, opacity
    sp.sampling, sp.flags = HEAT_SMOOTH if smooth else HEAT_NEAREST, HEAT_RAMP_ALPHA if ramp_alpha else 0
    if palette is not None:
        pal = np.zeros((256, 4), np.uint8)
        pal[:, :3] = np.asarray(palette, np.uint8).reshape(256, -1)[:, :3]
        sp._pal = pal
        sp.palette = pal.ctypes.data
    return sp


def heat_spec_check(spec):
    """ffgpu_heat_spec_check (pure host code): raises with what is wrong with the spec"""
    _check(lib().ffgpu_heat_spec_check(spec), "ffgpu_heat_spec_check")


def heat_blend_spec_check(spec):
    """ffgpu_heat_blend_spec_check (pure host code): raises with what is wrong with the spec"""
    _check(lib().ffgpu_heat_blend_spec_check(spec), "ffgpu_heat_blend_spec_check")


def heat_palette(nv12=False):
    """ffgpu_heat_palette (pure host code): the built-in palette as a (256, 4) uint8 array, B G R 0 or Y U V 0"""
    out = np.zeros((256, 4), np.uint8)
    _check(lib().ffgpu_heat_palette(1 if nv12 else 0, out.ctypes.data), "ffgpu_heat_palette")
    return out


def heat_state_bytes(nstreams, gw, gh):
    return lib().ffgpu_heat_state_bytes(nstreams, gw, gh)


def heat_state(raw, nstreams, gw, gh):
    """(headers as a uint32 array of nstreams x 4: frames, peak, reserved x 2; cells as a uint32 array of nstreams x gh x gw) of a state's bytes"""
    one = (HEAT_STATE_HEADER + 4 * gw * gh + 15) & ~15
    raw = np.ascontiguousarray(raw, np.uint8).reshape(nstreams, one)
    return (np.ascontiguousarray(raw[:, :HEAT_STATE_HEADER]).view("<u4"),
            np.ascontiguousarray(raw[:, HEAT_STATE_HEADER:HEAT_STATE_HEADER + 4 * gw * gh]).view("<u4").reshape(nstreams, gh, gw))


def heat_reset_dev(d_state, nstreams, gw, gh, which_stream=-1, stream=None):
    """ffgpu_heat_reset_dev: zero the heat state of one video stream, or of all (-1), in stream order"""
    _check(lib().ffgpu_heat_reset_dev(d_state, nstreams, gw, gh, which_stream, stream), "ffgpu_heat_reset_dev")


def heat_boxes_dev(d_records, d_lists, list_stride, streams, spec, d_state, nstreams, d_rows, list_first=None, stream=None):
    """ffgpu_heat_boxes_dev on device records / lists: record t is the next frame of video stream streams[t] (-1: ignored); d_lists None: the
    records' own boxes; list_first as draw_boxes_bgr_dev; d_rows: rows of HEAT_ROW ints"""
    arr = (C.c_int * max(1, len(streams)))(*[int(v) for v in streams])
    first = None if list_first is None else (C.c_int * max(1, len(list_first)))(*[int(v) for v in list_first])
    _check(lib().ffgpu_heat_boxes_dev(d_records, d_lists, list_stride, first, arr, len(streams), spec, d_state, nstreams, d_rows, stream), "ffgpu_heat_boxes_dev")


def heat_blend_bgr_dev(d_state, nstreams, streams, frames, spec, stream=None):
    """ffgpu_heat_blend_bgr_dev: the grid of video stream streams[t] (-1: untouched) blended into frames[t] (what bgr_frame_desc accepts, or None:
    skipped) as it is when the launch runs"""
    arr = (C.c_int * max(1, len(streams)))(*[int(v) for v in streams])
    _check(lib().ffgpu_heat_blend_bgr_dev(d_state, nstreams, arr, bgr_frame_table(frames), len(frames), spec, stream), "ffgpu_heat_blend_bgr_dev")


def heat_blend_nv12_dev(d_state, nstreams, streams, frames, spec, stream=None):
    """ffgpu_heat_blend_nv12_dev: the same in NV12 frames (what nv12_frame_desc accepts, or None: skipped)"""
    arr = (C.c_int * max(1, len(streams)))(*[int(v) for v in streams])
    _check(lib().ffgpu_heat_blend_nv12_dev(d_state, nstreams, arr, nv12_frame_table(frames), len(frames), spec, stream), "ffgpu_heat_blend_nv12_dev")


def motion_spec(w, h, cell_log2, threshold=16, learn_shift=4, learn_shift_changed=8, min_pixels=1, cover=64, warmup=0, invert=False, min_score=0.0, classes=None):
    """a MotionSpec (ffgpu_motion_spec): the model's size and its cells (1 << cell_log2 pixels), when a pixel counts as changed, how fast the model
    follows an unchanged and a changed pixel (shifts; 0: take the frame, 16: keep the model), when a cell is active, the share of a box's cells
    (of 256) that must be active for the box to move, the frames the gate fails open for, and which boxes qualify (min_score, classes as
    redact_spec).  The structure keeps its class bytes alive."""
    sp = MotionSpec()
    sp.w, sp.h, sp.cell_log2, sp.threshold, sp.learn_shift, sp.learn_shift_changed, sp.min_pixels = w, h, cell_log2, threshold, learn_shift, learn_shift_changed, min_pixels
    sp.cover, sp.warmup, sp.flags, sp.min_score = cover, warmup, MOTION_GATE_INVERT if invert else 0, min_score
    if classes is not None:
        cls = np.ascontiguousarray(np.asarray(classes) != 0, np.uint8) if len(classes) else np.zeros(1, np.uint8)
        sp._cls = cls                                           # (owned by the structure: the C side reads it during the call)
        sp.classes = cls.ctypes.data
        sp.nclasses = len(classes)
    return sp


def motion_spec_check(spec):
    """ffgpu_motion_spec_check (pure host code): raises with what is wrong with the spec"""
    _check(lib().ffgpu_motion_spec_check(spec), "ffgpu_motion_spec_check")


def motion_state_bytes(nstreams, w, h, cell_log2):
    return lib().ffgpu_motion_state_bytes(nstreams, w, h, cell_log2)


def motion_state(raw, nstreams, w, h, cell_log2):
    """(headers as a uint32 array of nstreams x 4: frames, reserved x 3; the planes as a uint16 array of nstreams x h x w, luma in 8.8 fixed point;
    the cells as a uint32 array of nstreams x gh x gw) of a state's bytes"""
    c = 1 << cell_log2
    gw, gh, pitch = (w + c - 1) // c, (h + c - 1) // c, (w + 7) & ~7
    cells_off = MOTION_STATE_HEADER + 2 * pitch * h
    one = cells_off + ((4 * gw * gh + 15) & ~15)
    raw = np.ascontiguousarray(raw, np.uint8).reshape(nstreams, one)
    return (np.ascontiguousarray(raw[:, :MOTION_STATE_HEADER]).view("<u4"),
            np.ascontiguousarray(np.ascontiguousarray(raw[:, MOTION_STATE_HEADER:cells_off]).view("<u2").reshape(nstreams, h, pitch)[:, :, :w]),
            np.ascontiguousarray(raw[:, cells_off:cells_off + 4 * gw * gh]).view("<u4").reshape(nstreams, gh, gw))


def motion_reset_dev(d_state, nstreams, w, h, cell_log2, which_stream=-1, stream=None):
    """ffgpu_motion_reset_dev: zero the motion state of one video stream, or of all (-1), in stream order"""
    _check(lib().ffgpu_motion_reset_dev(d_state, nstreams, w, h, cell_log2, which_stream, stream), "ffgpu_motion_reset_dev")


def motion_update_bgr_dev(frames, streams, spec, d_state, nstreams, d_rows, stream=None):
    """ffgpu_motion_update_bgr_dev: frames[t] (what bgr_frame_desc accepts, or None: skipped) is the next frame of video stream streams[t] (-1:
    ignored); a stream's frames are taken in the order given; d_rows: rows of MOTION_ROW ints"""
    arr = (C.c_int * max(1, len(streams)))(*[int(v) for v in streams])
    _check(lib().ffgpu_motion_update_bgr_dev(bgr_frame_table(frames), len(frames), arr, spec, d_state, nstreams, d_rows, stream), "ffgpu_motion_update_bgr_dev")


def motion_update_nv12_dev(frames, streams, spec, d_state, nstreams, d_rows, stream=None):
    """ffgpu_motion_update_nv12_dev: the same on NV12 frames (what nv12_frame_desc accepts, or None: skipped); only the Y plane is read"""
    arr = (C.c_int * max(1, len(streams)))(*[int(v) for v in streams])
    _check(lib().ffgpu_motion_update_nv12_dev(nv12_frame_table(frames), len(frames), arr, spec, d_state, nstreams, d_rows, stream), "ffgpu_motion_update_nv12_dev")


def motion_gate_dev(d_records, d_lists, list_stride, streams, spec, d_state, nstreams, d_words, d_out_records=None, d_out_lists=None, list_first=None, stream=None):
    """ffgpu_motion_gate_dev on device records / lists: record t belongs to video stream streams[t] (-1: ignored); d_lists None: the records' own
    boxes; list_first as draw_boxes_bgr_dev; d_words: rows of MOTION_WORDS + 2 S ints; the gated records and lists are optional"""
    arr = (C.c_int * max(1, len(streams)))(*[int(v) for v in streams])
    first = None if list_first is None else (C.c_int * max(1, len(list_first)))(*[int(v) for v in list_first])
    _check(lib().ffgpu_motion_gate_dev(d_records, d_lists, list_stride, first, arr, len(streams), spec, d_state, nstreams, d_words, d_out_records, d_out_lists, stream),
           "ffgpu_motion_gate_dev")


def feature_spec(layer=-1, pool=FFGPU.FEAT_MEAN, post=FFGPU.POST_NONE):
    """a FeatureSpec (ffgpu_feature_spec)"""
    return FeatureSpec(layer, pool, post, 0)


def feature_dim(c, h, w, pool):
    """ffgpu_feature_dim: D of a c x h x w tensor under `pool`; 0 outside the ranges (no GPU needed)"""
    return lib().ffgpu_feature_dim(c, h, w, pool)


def features_dev(d_in, n, c, h, w, pool, post, d_out, out_stride=None, stream=None):
    """ffgpu_features_dev on a device tensor in CNHW layout: n rows of D floats at d_out, out_stride floats apart (default: D); returns D"""
    d = feature_dim(c, h, w, pool)
    _check(lib().ffgpu_features_dev(d_in, n, c, h, w, pool, post, d_out, (d if out_stride is None else out_stride), stream), "ffgpu_features_dev")
    return d


def topk_dev(d_in, n, d, k, d_out, in_stride=None, stream=None):
    """ffgpu_topk_dev: the k best (index, value) of each of n rows of d floats (in_stride floats apart, default d) as n x k Label at d_out"""
    _check(lib().ffgpu_topk_dev(d_in, n, d, d if in_stride is None else in_stride, k, d_out, stream), "ffgpu_topk_dev")


def relabel_spec(min_value=0.0, type_base=0, score_mode=FFGPU.RELABEL_KEEP_SCORE):
    """a RelabelSpec (ffgpu_relabel_spec)"""
    return RelabelSpec(min_value, type_base, score_mode, 0)


def crops_relabel_dev(d_table, capacity, d_labels, k, d_records, d_lists, list_stride, ntargets, spec, d_out_records, d_out_lists=None, list_first=None,
                      stream=None):
    """ffgpu_crops_relabel_dev on device records / lists: the best label of every crop slot written into the box the crop was cut from; d_lists None:
    the records' own boxes; list_first as draw_boxes_bgr_dev"""
    first = None if list_first is None else (C.c_int * max(1, len(list_first)))(*[int(v) for v in list_first])
    _check(lib().ffgpu_crops_relabel_dev(d_table, capacity, d_labels, k, d_records, d_lists, list_stride, first, ntargets, spec, d_out_records, d_out_lists,
                                         stream), "ffgpu_crops_relabel_dev")


def gallery(d_rows, capacity, d, d_ids=None, d_head=None, row_stride=None):
    """a Gallery (ffgpu_gallery): capacity rows of d floats at d_rows, row_stride floats apart (default d); d_ids / d_head as the header says"""
    return Gallery(d_rows, d_ids, d_head, d if row_stride is None else row_stride, capacity, d)


def match_workspace_bytes(nq, capacity, k):
    """ffgpu_match_workspace_bytes: the scratch ffgpu_match_dev needs; 0 outside the ranges (no GPU needed)"""
    return int(lib().ffgpu_match_workspace_bytes(nq, capacity, k))


def match_dev(d_q, nq, g, k, d_out_labels, d_work, work_bytes, d_sim=None, sim_stride=None, q_stride=None, stream=None):
    """ffgpu_match_dev: the k best gallery rows of each of nq query rows (q_stride floats apart, default g.d) as nq x k Label at d_out_labels; d_sim:
    the nq x capacity matrix as well, sim_stride floats apart (default capacity)"""
    _check(lib().ffgpu_match_dev(d_q, nq, g.d if q_stride is None else q_stride, g, k, d_out_labels, d_sim, g.capacity if sim_stride is None else sim_stride,
                                 d_work, work_bytes, stream), "ffgpu_match_dev")


def gallery_enroll_dev(g, d_q, nq, d_labels, k, min_value, d_out_labels, q_stride=None, stream=None):
    """ffgpu_gallery_enroll_dev: the queries whose best label (entry 0 of each row of k) does not reach min_value appended to the gallery; nq Label at
    d_out_labels"""
    _check(lib().ffgpu_gallery_enroll_dev(g, d_q, nq, g.d if q_stride is None else q_stride, d_labels, k, min_value, d_out_labels, stream),
           "ffgpu_gallery_enroll_dev")


# the operators as attributes of FFGPU as well (FFGPU.features_dev(...)), next to the constants they take
for _f in (feature_spec, feature_dim, features_dev, topk_dev, relabel_spec, crops_relabel_dev, gallery, match_workspace_bytes, match_dev, gallery_enroll_dev):
    setattr(FFGPU, _f.__name__, staticmethod(_f))
del _f


def tile_table(tiles):
    """a Tile array from a sequence of (image, x0, y0) tuples (or Tile structures; a Tile array passes through)"""
    if isinstance(tiles, C.Array):
        return tiles
    arr = (Tile * max(1, len(tiles)))()
    for k, t in enumerate(tiles):
        arr[k] = t if isinstance(t, Tile) else Tile(t[0], t[1], t[2], 0)
    return arr


def tile_plan(img_w, img_h, tile_w, tile_h, overlap_x=0, overlap_y=0, align=1):
    """ffgpu_tile_plan: [(x0, y0, w, h)] of the tiles that cover an img_w x img_h picture, rows of tiles left to right, top to bottom"""
    n = _check(lib().ffgpu_tile_plan(img_w, img_h, tile_w, tile_h, overlap_x, overlap_y, align, None, 0), "ffgpu_tile_plan")
    out = (TileRect * n)()
    _check(lib().ffgpu_tile_plan(img_w, img_h, tile_w, tile_h, overlap_x, overlap_y, align, out, n), "ffgpu_tile_plan")
    return [(r.x0, r.y0, r.w, r.h) for r in out]


def tiles_of(img, plan, image=0):
    """(frames, tiles) for Executor.forward_bgr_frames_dev and Executor.merge_tiles: the plan's crops of an (h, w, 3) uint8 device tensor (views, no copy)"""
    return [img[y0:y0 + h, x0:x0 + w] for x0, y0, w, h in plan], [(image, x0, y0) for x0, y0, w, h in plan]


def merge_tiles_dev(d_records, d_lists, list_stride, tiles, nimages, d_out_records, d_out_lists=None, thresh=0.5, use_min=1,
                    d_scratch=None, scratch_bytes=0, stream=None):
    """ffgpu_merge_tiles_dev on device buffers: tiles as Executor.merge_tiles takes them"""
    _check(lib().ffgpu_merge_tiles_dev(d_records, d_lists, list_stride, tile_table(tiles), len(tiles), nimages, thresh, use_min,
                                       d_out_records, d_out_lists, d_scratch, scratch_bytes, stream), "ffgpu_merge_tiles_dev")


def merge_tiles_scratch_bytes(ntiles, list_stride):
    return int(lib().ffgpu_merge_tiles_scratch_bytes(ntiles, list_stride))


def shard_range(total, rank, world):
    lo, hi = C.c_int(), C.c_int()
    lib().ffgpu_shard_range(total, rank, world, C.byref(lo), C.byref(hi))
    return lo.value, hi.value


class Node:
    """ffgpu_node_*: one process, ndev GPUs (RCCL broadcast of the weights, gather of the records)"""
    LOOPBACK = 1

    @staticmethod
    def DEPTH(n):
        return (n & 0xf) << 8

    def submit(self, frames=None):
        if frames is not None:
            frames = np.ascontiguousarray(frames, np.float32)
            assert frames.shape == (self.total,) + self.net.input_shape, frames.shape
        t = lib().ffgpu_node_submit(self.h, frames.ctypes.data_as(f32p) if frames is not None else None)
        if t < 0:
            raise RuntimeError("ffgpu_node_submit failed: %s" % last_error())
        return t                                                # (numpy memory is staged inside submit: `frames` is free again)

    def wait(self, ticket):
        out = np.zeros(self.total, DETS_DTYPE)
        _check(lib().ffgpu_node_wait(self.h, ticket, out.ctypes.data), "ffgpu_node_wait")
        return out

    def wait_into(self, ticket, out):
        """as wait(), into a caller-owned DETS_DTYPE array of `total` records"""
        assert out.dtype == DETS_DTYPE and len(out) == self.total and out.flags["C_CONTIGUOUS"]
        _check(lib().ffgpu_node_wait(self.h, ticket, out.ctypes.data), "ffgpu_node_wait")
        return out

    def rccl_ranks(self):
        return lib().ffgpu_node_rccl_ranks(self.h)

    def run(self, steps, out=None):
        """ffgpu_node_run: `steps` pipelined steps from the slots' input buffers (the loop runs in C); records of the last step"""
        if out is None:
            out = np.zeros(self.total, DETS_DTYPE)
        assert out.dtype == DETS_DTYPE and len(out) == self.total and out.flags["C_CONTIGUOUS"]
        _check(lib().ffgpu_node_run(self.h, steps, out.ctypes.data), "ffgpu_node_run")
        return out

    def input_slot_dev(self, rank, slot):
        return lib().ffgpu_node_input_slot_dev(self.h, rank, slot)

    def __init__(self, net, ndev, global_batch, devices=None, exec_flags=0, node_flags=0):
        self.net, self.ndev, self.total = net, ndev, global_batch
        dv = (C.c_int * ndev)(*devices) if devices is not None else None
        self.h = lib().ffgpu_node_create(net.p, ndev, dv, global_batch, exec_flags, node_flags)
        if not self.h:
            raise RuntimeError("ffgpu_node_create failed: %s" % last_error())

    def close(self):
        if self.h:
            lib().ffgpu_node_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def shard(self, rank):
        lo, hi, dev = C.c_int(), C.c_int(), C.c_int()
        _check(lib().ffgpu_node_shard(self.h, rank, C.byref(lo), C.byref(hi), C.byref(dev)), "ffgpu_node_shard")
        return lo.value, hi.value, dev.value

    def set_scale(self, s1, s2):
        _check(lib().ffgpu_node_set_scale(self.h, s1, s2), "ffgpu_node_set_scale")

    def input_dev(self, rank):
        return lib().ffgpu_node_input_dev(self.h, rank)

    def forward(self):
        out = np.zeros(self.total, DETS_DTYPE)
        _check(lib().ffgpu_node_forward(self.h, out.ctypes.data), "ffgpu_node_forward")
        return out

    def forward_host(self, frames):
        frames = np.ascontiguousarray(frames, np.float32)
        assert frames.shape == (self.total,) + self.net.input_shape, frames.shape
        out = np.zeros(self.total, DETS_DTYPE)
        _check(lib().ffgpu_node_forward_host(self.h, frames.ctypes.data_as(f32p), out.ctypes.data), "ffgpu_node_forward_host")
        return out


def groupconv_dev(d_in, d_filt, d_out, batch, iw, ih, ic, groups, pad, stride, fs, fn, act=0, flags=0, variant=0, stream=None):
    ow, oh = (iw + 2 * pad - fs) // stride + 1, (ih + 2 * pad - fs) // stride + 1
    _check(lib().ffgpu_groupconv_dev(d_in, d_filt, d_out, batch, iw, ih, ic, groups, pad, stride, fs, fn, ow, oh, fn,
                                     act, flags, variant, stream), "ffgpu_groupconv_dev")


def groupconv_time_dev(d_in, d_filt, d_out, batch, iw, ih, ic, groups, pad, stride, fs, fn, act=0, flags=0, variant=0,
                       warmup=5, iters=20, stream=None):
    ow, oh = (iw + 2 * pad - fs) // stride + 1, (ih + 2 * pad - fs) // stride + 1
    us = lib().ffgpu_groupconv_time_dev(d_in, d_filt, d_out, batch, iw, ih, ic, groups, pad, stride, fs, fn, ow, oh, fn,
                                        act, flags, variant, warmup, iters, stream)
    if us < 0:
        raise RuntimeError("ffgpu_groupconv_time_dev failed: %s" % last_error())
    return us


def packed_records_bytes(batch, cap):
    return int(lib().ffgpu_packed_records_bytes(batch, cap))


def pack_records_dev(d_records, nslots, slot_stride_records, batch, cap, d_out, stream=None):
    """pack nslots steps of `batch` fixed-size records (device) into compact blocks (device): what the multi-GPU gather moves"""
    _check(lib().ffgpu_pack_records(d_records, nslots, slot_stride_records, batch, cap, d_out, stream), "ffgpu_pack_records")


def kernel_name(batch, iw, ih, ic, groups, pad, stride, fs, fn, variant=0):
    return lib().ffgpu_groupconv_kernel_name(batch, iw, ih, ic, groups, pad, stride, fs, fn, variant).decode()


def irb_plan_text(shape, flags=0):
    """what the planner decides for the fused block shape = (batch, iw, ih, ic, ec, oc, stride, act1, actd, act2, res_act), as one line of text (no GPU needed)"""
    buf = C.create_string_buffer(1024)
    if lib().ffgpu_irb_plan_text(*shape, flags, buf, len(buf)) < 0:
        raise RuntimeError("ffgpu_irb_plan_text failed: %s" % last_error())
    return buf.value.decode()


def irb_stage_plan_text(batch, iw, ih, blocks, act1=2, actd=2, flags=0):
    """what an executor of `batch` frames made with `flags` does with a run of `blocks` blocks 48 -> 224 -> 48 on an iw x ih plane: "stage ..." (one
    launch), "blocks ..." (one per block) or "unsupported" (no GPU needed)"""
    buf = C.create_string_buffer(1024)
    if lib().ffgpu_irb_stage_plan_text(batch, iw, ih, blocks, act1, actd, flags, buf, len(buf)) < 0:
        raise RuntimeError("ffgpu_irb_stage_plan_text failed: %s" % last_error())
    return buf.value.decode()


FRONT_FORMS = {"f32": 0, "u8": 1, "bgr_frames": 2, "nv12_frames": 3}


def front_plan_text(batch, pw, ph, form="f32"):
    """which instantiation of k_front a batch on a pw x ph plane (net input 2 pw x 2 ph) takes when it arrives in `form` (a key of FRONT_FORMS), and its launch
    shape: "front<OC,U8,NC,RS,NV> W= H= N= band= nbands= ntasks= grid= block=", "staged" or "unsupported" (no GPU needed)"""
    buf = C.create_string_buffer(256)
    if lib().ffgpu_front_plan_text(batch, pw, ph, FRONT_FORMS[form], buf, len(buf)) < 0:
        raise RuntimeError("ffgpu_front_plan_text failed: %s" % last_error())
    return buf.value.decode()


def irb_instantiations():
    """the key of every fused-block instantiation (the first word of irb_plan_text's line), in table order (no GPU needed)"""
    buf = C.create_string_buffer(4096)
    n = lib().ffgpu_irb_instantiations(buf, len(buf))
    if n < 0 or n >= len(buf):
        raise RuntimeError("ffgpu_irb_instantiations failed: %s" % (last_error() if n < 0 else "%d bytes" % n))
    return buf.value.decode().split()


def knobs():
    """every environment variable the library reads, in table order (no GPU needed): dicts of name, kind (INT / ON / SET / TEXT), default
    (an int, "computed" or None), cls (product / tuning / test / lab), value (what a read returns now under os.environ, as text) and text"""
    buf = C.create_string_buffer(1 << 16)
    n = lib().ffgpu_knobs_text(buf, len(buf))
    if n < 0 or n >= len(buf):
        raise RuntimeError("ffgpu_knobs_text failed: %s" % (last_error() if n < 0 else "%d bytes" % n))
    rows = []
    for line in buf.value.decode().splitlines():
        name, kind, dflt, cls, value, text = line.split(" ", 5)
        rows.append({"name": name, "kind": kind, "default": None if dflt == "-" else dflt if dflt == "computed" else int(dflt), "cls": cls, "value": value, "text": text})
    return rows


def dwpw_dev(d_in, d_wd, d_wp, d_out, batch, iw, ih, c, oc, fs, actd=2, actp=0, warmup=0, iters=0, stream=None):
    """fused depthwise KxK (s1, same padding) -> pointwise 1x1; returns us per launch when iters > 0"""
    us = lib().ffgpu_dwpw_dev(d_in, d_wd, d_wp, d_out, batch, iw, ih, c, oc, fs, actd, actp, warmup, iters, stream)
    if us < 0:
        raise RuntimeError("ffgpu_dwpw_dev failed: %s" % last_error())
    return us


def irb_thin_launch_text(shape, flags=0):
    """what the launch of the thin block shape = (batch, iw, ih, ic, ec, oc, stride, act1, actd, act2, res_act) does in an executor made with `flags`:
    "thin<IC,8,OC> ..." (one frame per wave), "thin_pair<IC,8,OC,NC> ..." (two) or "unsupported" (no GPU needed)"""
    buf = C.create_string_buffer(256)
    if lib().ffgpu_irb_thin_launch_text(*shape, flags, buf, len(buf)) < 0:
        raise RuntimeError("ffgpu_irb_thin_launch_text failed: %s" % last_error())
    return buf.value.decode()


def irb_s2_launch_text(shape, flags=0):
    """what the launch of the block shape = (batch, iw, ih, ic, ec, oc, stride, act1, actd, act2, res_act) does in an executor made with `flags`:
    "thin_s2<4,24,8,3> frames= band= tasks= grid= ..." (the streaming stride-2 form), "<planned key> frames= band= tasks= grid= block=" or
    "unsupported" (no GPU needed)"""
    buf = C.create_string_buffer(256)
    if lib().ffgpu_irb_s2_launch_text(*shape, flags, buf, len(buf)) < 0:
        raise RuntimeError("ffgpu_irb_s2_launch_text failed: %s" % last_error())
    return buf.value.decode()


def sparse_head_dev(d_in, d_filt, d_out, batch, iw, ih, ic, classes, thresh, d_list, d_count, act=0, stream=None):
    """the pointwise layer ic -> 3 (5 + classes) in front of a yolo head as the sparse pair of k_conv_x3 launches (box pass, class pass) on caller-owned
    device tensors; d_list (batch ih iw / 4 int32) and d_count (one int32, the caller zeroes it) receive the listed quads and their number"""
    _check(lib().ffgpu_sparse_head_dev(d_in, d_filt, d_out, batch, iw, ih, ic, classes, act, thresh, d_list, d_count, stream), "ffgpu_sparse_head_dev")


def sparse_head_launch_text(batch, iw, ih, ic, classes, flags=0):
    """what an executor made with `flags` launches for that layer: "sparse box<1,NW> rows=15 grid= class<MT,NW> rows= grid= quads= image=" or
    "dense <kernel>" (no GPU needed)"""
    buf = C.create_string_buffer(256)
    if lib().ffgpu_sparse_head_launch_text(batch, iw, ih, ic, classes, flags, buf, len(buf)) < 0:
        raise RuntimeError("ffgpu_sparse_head_launch_text failed: %s" % last_error())
    return buf.value.decode()


def irb_dev(d_in, d_w1, d_wd, d_w2, d_res, d_out, batch, iw, ih, ic, ec, oc, stride, act1=2, actd=2, act2=0, res_act=0,
            warmup=0, iters=0, stream=None, flags=0):
    """fused expand -> dw3x3 -> project [+ residual], planned and launched as in an executor made with `flags`; returns us per launch when iters > 0"""
    us = lib().ffgpu_irb_flags_dev(d_in, d_w1, d_wd, d_w2, d_res, d_out, batch, iw, ih, ic, ec, oc, stride, act1, actd, act2, res_act, flags,
                                   warmup, iters, stream)
    if us < 0:
        raise RuntimeError("ffgpu_irb_dev failed: %s" % last_error())
    return us


# ---------------------------------------------------------------------------------------------------------------- preview surfaces
def preview_pane(src=None, dst=None):
    """a PreviewPane (ffgpu_preview_pane): src = (sx, sy, sw, sh), the source region, or None for the whole frame; dst = (dx, dy, dw, dh), the pane
    in the destination surface, or None for the whole surface"""
    p = PreviewPane()
    if src is not None:
        p.sx, p.sy, p.sw, p.sh = (int(v) for v in src)
    if dst is not None:
        p.dx, p.dy, p.dw, p.dh = (int(v) for v in dst)
    return p


def preview_spec(fit=PREVIEW_STRETCH, fill=(0, 0, 0), keep_bars=False):
    """a PreviewSpec (ffgpu_preview_spec): PREVIEW_STRETCH or PREVIEW_FIT; the bars' colour, B G R for BGR surfaces and Y U V for NV12 ones; keep_bars:
    the bars are not written"""
    sp = PreviewSpec()
    sp.fit, sp.flags = fit, PREVIEW_KEEP_BARS if keep_bars else 0
    sp.fill[:] = (int(fill[0]), int(fill[1]), int(fill[2]), 0)
    return sp


def preview_spec_check(spec):
    """ffgpu_preview_spec_check (pure host code): raises with what is wrong with the spec"""
    _check(lib().ffgpu_preview_spec_check(spec), "ffgpu_preview_spec_check")


def preview_rect(src_w, src_h, dst_w, dst_h, pane, spec, nv12=False):
    """ffgpu_preview_rect (pure host code): (sx, sy, sw, sh, X0, Y0, ow, oh) -- the pane's source region and its image in the destination surface"""
    out = (C.c_int * 8)()
    _check(lib().ffgpu_preview_rect(src_w, src_h, dst_w, dst_h, pane, spec, int(bool(nv12)), out), "ffgpu_preview_rect")
    return tuple(out)


def preview_grid(npanes, cols, dst_w, dst_h, gap=0, nv12=False):
    """ffgpu_preview_grid (pure host code): the panes of a wall of `cols` columns in a dst_w x dst_h surface, as a list of PreviewPane whose source
    fields are zero (the whole frame)"""
    arr = (PreviewPane * max(1, npanes))()
    _check(lib().ffgpu_preview_grid(npanes, cols, dst_w, dst_h, gap, int(bool(nv12)), arr), "ffgpu_preview_grid")
    return [PreviewPane.from_buffer_copy(arr[k]) for k in range(npanes)]


def preview_tile():
    """ffgpu_preview_tile (pure host code): (the columns, the rows of a workgroup's tile of destination samples, the planes one launch takes)"""
    out = (C.c_int * 3)()
    _check(lib().ffgpu_preview_tile(out), "ffgpu_preview_tile")
    return tuple(out)


def _preview_panes(panes):
    arr = (PreviewPane * max(1, len(panes)))()
    for k, p in enumerate(panes):
        arr[k] = p
    return arr


def preview_bgr_dev(srcs, dsts, panes, spec, stream=None):
    """ffgpu_preview_bgr_dev: pane p scales srcs[p] into dsts[p] (what bgr_frame_desc accepts, or None: the pane is skipped); panes from preview_pane
    or preview_grid, spec from preview_spec.  Enqueued on `stream` without synchronising."""
    if not len(srcs) == len(dsts) == len(panes):
        raise ValueError("%d sources, %d destinations and %d panes" % (len(srcs), len(dsts), len(panes)))
    _check(lib().ffgpu_preview_bgr_dev(bgr_frame_table(srcs), bgr_frame_table(dsts), _preview_panes(panes), len(panes), spec, stream), "ffgpu_preview_bgr_dev")


def preview_nv12_dev(srcs, dsts, panes, spec, stream=None):
    """ffgpu_preview_nv12_dev: the same on NV12 frames (what nv12_frame_desc accepts, or None: skipped)"""
    if not len(srcs) == len(dsts) == len(panes):
        raise ValueError("%d sources, %d destinations and %d panes" % (len(srcs), len(dsts), len(panes)))
    _check(lib().ffgpu_preview_nv12_dev(nv12_frame_table(srcs), nv12_frame_table(dsts), _preview_panes(panes), len(panes), spec, stream), "ffgpu_preview_nv12_dev")


# ---------------------------------------------------------------------------------------------------------------- warp surfaces
def warp_spec(filter=WARP_BILINEAR, border=WARP_FILL, fill=(0, 0, 0)):
    """a WarpSpec (ffgpu_warp_spec): WARP_BILINEAR or WARP_NEAREST; WARP_FILL or WARP_CLAMP; the colour of a tap outside the source frame, B G R for
    BGR frames and Y U V for NV12 ones"""
    sp = WarpSpec()
    sp.filter, sp.border = filter, border
    sp.fill[:] = (int(fill[0]), int(fill[1]), int(fill[2]), 0)
    return sp


def warp_spec_check(spec):
    """ffgpu_warp_spec_check (pure host code): raises with what is wrong with the spec"""
    _check(lib().ffgpu_warp_spec_check(spec), "ffgpu_warp_spec_check")


def warp_mesh_size(dst_w, dst_h, cell):
    """ffgpu_warp_mesh_size (pure host code): (mw, mh)"""
    out = (C.c_int * 2)()
    _check(lib().ffgpu_warp_mesh_size(dst_w, dst_h, cell, out), "ffgpu_warp_mesh_size")
    return tuple(out)


def warp_mesh_orient(src_w, src_h, orient, cell):
    """ffgpu_warp_mesh_orient (pure host code): ((dw, dh), the mesh as an int32 array of shape (mh, mw, 2)) for orientation 0..7 of a src_w x src_h frame"""
    wh = (C.c_int * 2)()
    _check(lib().ffgpu_warp_mesh_orient(src_w, src_h, orient, cell, wh, None), "ffgpu_warp_mesh_orient")
    mw, mh = warp_mesh_size(wh[0], wh[1], cell)
    xy = np.empty((mh, mw, 2), np.int32)
    _check(lib().ffgpu_warp_mesh_orient(src_w, src_h, orient, cell, wh, xy.ctypes.data), "ffgpu_warp_mesh_orient")
    return (wh[0], wh[1]), xy


def warp_mesh_homography(dst_w, dst_h, cell, h):
    """ffgpu_warp_mesh_homography (pure host code): the mesh (mh, mw, 2) of the homography h (9 numbers, row-major, destination pixel to source position)"""
    mw, mh = warp_mesh_size(dst_w, dst_h, cell)
    xy = np.empty((mh, mw, 2), np.int32)
    _check(lib().ffgpu_warp_mesh_homography(dst_w, dst_h, cell, (C.c_double * 9)(*[float(v) for v in h]), xy.ctypes.data), "ffgpu_warp_mesh_homography")
    return xy


def warp_lens(model, dst, src, k=(0, 0, 0, 0), p=(0, 0)):
    """a WarpLens (ffgpu_warp_lens): WARP_LENS_BROWN or WARP_LENS_EQUIDISTANT; dst and src are (fx, fy, cx, cy) of the ideal pinhole image and of the camera"""
    ln = WarpLens()
    ln.model = model
    ln.dst[:], ln.src[:] = [float(v) for v in dst], [float(v) for v in src]
    ln.k[:], ln.p[:] = [float(v) for v in k], [float(v) for v in p]
    return ln


def warp_mesh_lens(dst_w, dst_h, cell, lens):
    """ffgpu_warp_mesh_lens (pure host code): the mesh (mh, mw, 2) that undistorts the lens (from warp_lens) into a dst_w x dst_h pinhole image"""
    mw, mh = warp_mesh_size(dst_w, dst_h, cell)
    xy = np.empty((mh, mw, 2), np.int32)
    _check(lib().ffgpu_warp_mesh_lens(dst_w, dst_h, cell, lens, xy.ctypes.data), "ffgpu_warp_mesh_lens")
    return xy


def warp_mesh(xy_ptr, dst_w, dst_h, cell):
    """a WarpMesh (ffgpu_warp_mesh) for a destination of dst_w x dst_h: xy_ptr is the address of its (mh, mw, 2) int32 points -- device memory for the
    operators, host memory for warp_point"""
    m = WarpMesh()
    m.xy, m.cell = xy_ptr, cell
    m.mw, m.mh = (dst_w - 1) // cell + 2, (dst_h - 1) // cell + 2
    return m


def warp_point(xy, cell, dst_w, dst_h, i, j):
    """ffgpu_warp_point (pure host code): (X8, Y8) of destination pixel (i, j) under the host mesh xy (an int32 array of shape (mh, mw, 2))"""
    xy = np.ascontiguousarray(xy, np.int32)
    m = WarpMesh(xy.ctypes.data, xy.shape[1], xy.shape[0], cell, 0)
    out = (C.c_int * 2)()
    _check(lib().ffgpu_warp_point(m, dst_w, dst_h, i, j, out), "ffgpu_warp_point")
    return tuple(out)


def warp_tile():
    """ffgpu_warp_tile (pure host code): (the columns, the rows of a workgroup's tile of destination pixels, the bytes of LDS the staged form may fill,
    the jobs one launch takes)"""
    out = (C.c_int * 4)()
    _check(lib().ffgpu_warp_tile(out), "ffgpu_warp_tile")
    return tuple(out)


def _warp_meshes(meshes):
    arr = (WarpMesh * max(1, len(meshes)))()
    for k, m in enumerate(meshes):
        if m is not None:
            arr[k] = m
    return arr


def warp_bgr_dev(srcs, dsts, meshes, spec, stream=None):
    """ffgpu_warp_bgr_dev: job n maps srcs[n] through meshes[n] into the whole of dsts[n] (what bgr_frame_desc accepts, or None: the job is skipped);
    meshes from warp_mesh, spec from warp_spec.  Enqueued on `stream` without synchronising."""
    if not len(srcs) == len(dsts) == len(meshes):
        raise ValueError("%d sources, %d destinations and %d meshes" % (len(srcs), len(dsts), len(meshes)))
    _check(lib().ffgpu_warp_bgr_dev(bgr_frame_table(srcs), bgr_frame_table(dsts), _warp_meshes(meshes), len(meshes), spec, stream), "ffgpu_warp_bgr_dev")


def warp_nv12_dev(srcs, dsts, meshes, spec, stream=None):
    """ffgpu_warp_nv12_dev: the same on NV12 frames (what nv12_frame_desc accepts, or None: skipped)"""
    if not len(srcs) == len(dsts) == len(meshes):
        raise ValueError("%d sources, %d destinations and %d meshes" % (len(srcs), len(dsts), len(meshes)))
    _check(lib().ffgpu_warp_nv12_dev(nv12_frame_table(srcs), nv12_frame_table(dsts), _warp_meshes(meshes), len(meshes), spec, stream), "ffgpu_warp_nv12_dev")
