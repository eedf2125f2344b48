"""Small nets for the merged 10x10 stage (ffgpu_irb_stage.inc): a depthwise 1x1 layer with weight 1 -- the net input has no tensor of its own, and a
fused block needs one to read; it hands every value on as it is, NaN and +-Inf included -- then B blocks 48 -> 224 -> 48 (1x1 expand, depthwise 3x3,
linear 1x1 project, dropout, linear shortcut from the block's input, the layer order of yolo-fastest) and nothing behind them: a headless net, whose last tensor every plan hands out
bit for bit (ffgpu_exec_features, FFGPU_FEAT_FLAT on layer -1; read_layer is for FFGPU_KEEP_ALL executors, which never merge).
Weights are the conv.h rows of tests/irb_blocks/blockref.py, written straight into the net's weight buffer."""
import ctypes as C

import numpy as np

from irb_blocks import blockref

IC, EC = 48, 224
ACT = {0: "linear", 1: "relu", 2: "leaky"}


class _DevBuf:
    """the library's device weight buffer as a CUDA array interface (fp32)"""
    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes // 4,), "typestr": "<f4", "data": (ptr, False), "version": 2}


def conv(filters, size, act, groups=1, stride=1):
    return "[convolutional]\n%sfilters=%d\nsize=%d\nstride=%d\npad=%d\nactivation=%s\n\n" % ("groups=%d\n" % groups if groups > 1 else "", filters, size, stride, 1 if size > 1 else 0, act)


def block(act1, actd, ic=IC, ec=EC, oc=IC, frm=-5, dropout=True):
    return conv(ec, 1, ACT[act1]) + conv(ec, 3, ACT[actd], groups=ec) + conv(oc, 1, "linear") + ("[dropout]\nprobability=.5\n\n" if dropout else "") + \
        "[shortcut]\nfrom=%d\nactivation=linear\n\n" % frm


def cfg_text(W, H, B, act1=2, actd=2):
    return "[net]\nwidth=%d\nheight=%d\nchannels=%d\n\n" % (W, H, IC) + conv(IC, 1, "linear", groups=IC) + "".join(block(act1, actd) for _ in range(B))


def first_layer(b):
    """index of block b's expand layer; its shortcut is 4 layers on"""
    return 1 + 5 * b


def rows(net, layer, fn, K):
    """the layer's filter rows inside the net's weight buffer, (fn, k4 + 4), writable"""
    k4 = (K + 3) & ~3
    off = (C.cast(net.layer(layer).filter, C.c_void_p).value - C.cast(net.n.weight_buf, C.c_void_p).value) // 4
    return net.weights_host()[off:off + fn * (k4 + 4)].reshape(fn, k4 + 4)


def commit(net):
    """the rows written through rows() are the host copy: write them over the device copy (the way a broadcast does), then refresh the packed images"""
    import torch
    ptr, nbytes = net.weights_dev()
    host = net.weights_host()
    assert nbytes == host.nbytes
    torch.as_tensor(_DevBuf(ptr, nbytes), device="cuda").copy_(torch.from_numpy(host.copy()))
    torch.cuda.synchronize()
    net.weights_commit()


def put(net, layers):
    """layers: [(layer index, K, filter rows (fn, k4 + 4))] of any cfg made of convolutions (tests/front uses it too); then commit"""
    for layer, K, f in layers:
        rows(net, layer, f.shape[0], K)[...] = f
    commit(net)


def fill(net, filters):
    """filters: [(f1, fd, f2)] per block"""
    ident = np.zeros((IC, 8), np.float32)
    ident[:, 0] = 1.0
    ident[:, 4] = 1.0
    layers = [(0, 1, ident)]
    for b, (f1, fd, f2) in enumerate(filters):
        p0 = first_layer(b)
        layers += [(p0, IC, f1), (p0 + 1, 9, fd), (p0 + 2, EC, f2)]
    put(net, layers)


def draw(seed, N, W, H, B):
    """x (CNHW: (48 N, H, W)) and B filter triples, seeded as tests/irb_blocks/cases.py seeds a case"""
    x, filters = None, []
    for b in range(B):
        xb, f1, fd, f2, _ = blockref.make_inputs(seed + b, N, W, H, IC, EC, IC, 1)
        x = xb if x is None else x
        filters.append((f1, fd, f2))
    return x, filters
