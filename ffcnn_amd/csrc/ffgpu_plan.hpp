// ffgpu_plan.hpp -- the executor planner's layout pass: which layer's output lives in which tensor (aliases, fused blocks, concat in place), how long
// every tensor lives, the optional side lane, and every tensor's offset in the one arena.  Integer work on the LAYER table alone: plain C++17 with no
// HIP in it, every refusal reported through ffgpu_set_error, so san/plan_driver.cc runs the same lines on the CPU under ASan + UBSan and checks the
// layout's invariants I1 - I5 (tests/test_plan_host.py).  The two questions only the kernels can answer -- does a fused kernel take the
// block of layers p0 .. p0 + 2, does one take the depthwise + pointwise pair p0, p0 + 1 -- reach the layout as callables of the layer index.
#pragma once
#include <algorithm>
#include <vector>
#include "ffcnn.h"

extern "C" void ffgpu_set_error(const char *fmt, ...);

struct Tensor {
    long size = 0;           // floats
    int  first = 1 << 30, last = -1;
    long off = -1;           // arena offset (roots only)
    int  parent = -1;        // concat-in-place parent tensor
    long parent_off = 0;
    bool used = false;
};

inline int root_of(const std::vector<Tensor> &ts, int t) { while (ts[t].parent >= 0) t = ts[t].parent; return t; }

// What the layout depends on beside the LAYER table; the executor fills one from its flags and the environment (plan_options, ffgpu_exec.hip).
struct PlanOptions {
    int  batch = 1;
    bool keep_all = false;   // FFGPU_KEEP_ALL: no two tensors share arena space
    bool fuse = true;        // !FFGPU_NO_FUSE: every rewrite below
    bool branch = false;     // FFGPU_BRANCH=1: the first detection head as a side lane
    bool no_irb = false;     // FFGPU_NO_IRB=1
    int  irb_min_ec = 0;     // FFGPU_IRB_MIN_EC, filled in by the executor for its block callable (the layout itself does not read it)
    bool dwpw = false;       // FFGPU_DWPW=1
    bool stage = false;      // runs of small-plane fused blocks as one launch: an FFGPU_CONCURRENT executor of at least 32 frames, FFGPU_IRB_STAGE not 0
};

struct NetLayout {
    std::vector<Tensor> tensors;        // index = layer id
    std::vector<int>    canon;          // layer id -> tensor id holding its output (-1: the batch input, -2: none, -3: fused away)
    std::vector<char>   readable;       // layer's own output value exists in memory after a forward
    std::vector<char>   route_inplace;  // multi-source route whose sources were allocated inside its tensor
    std::vector<int>    nuses;          // consumers per LAYER output (before aliasing)
    std::vector<int>    fused_into;     // conv p -> shortcut s whose add it absorbs
    std::vector<int>    irb_tail;       // layer p + 2 -> p: 1x1 expand -> depthwise 3x3 -> 1x1 project as one fused block
    std::vector<int>    dwpw_tail;      // layer p + 1 -> p: depthwise + pointwise as one launch
    std::vector<int>    stage_first;    // last layer of the LAST block of a merged run -> first layer of its first block: the run is one launch at that layer
    std::vector<char>   stage_inner;    // last layer of every other block of a merged run: no launch, no tensor
    int    side_lo = -1, side_hi = -1;  // layers [side_lo, side_hi] form the side lane
    size_t arena_floats = 0;

    int src(int i) const { return i < 0 ? -1 : canon[i]; }      // tensor holding the output of layer i
    long offset_of(int t) const                                 // arena offset of tensor t, its concat parents folded in
    {
        long off = 0;
        while (tensors[t].parent >= 0) { off += tensors[t].parent_off; t = tensors[t].parent; }
        return tensors[t].off + off;
    }
};

// The tensors layer i reads, each handed to f (ids below 0 -- the batch input, no tensor -- included): its chain input, its depend_list entries, the
// input of a fused block that ends at i, and the residual of a shortcut that block absorbed.
template <class F>
void ffgpu_layer_reads(const LAYER *ll, const NetLayout &nl, int i, F f)
{
    if (ll[i].type != LAYER_TYPE_ROUTE) f(nl.src(i - 1));
    for (int k = 0; k < ll[i].depend_num; k++) f(nl.src(ll[i].depend_list[k]));
    if (nl.irb_tail[i] >= 0) f(nl.src(nl.irb_tail[i] - 1));
    if (nl.dwpw_tail[i] >= 0) f(nl.src(nl.dwpw_tail[i] - 1));
    if (nl.stage_first[i] >= 0) f(nl.src(nl.stage_first[i] - 1));
    if (nl.irb_tail[i] >= 0 && nl.fused_into[i] >= 0) f(nl.src(ll[nl.fused_into[i]].depend_list[0]));
}

// a concat root lives as long as any tensor inside it
inline void ffgpu_fold_onto_roots(std::vector<Tensor> &T)
{
    for (size_t t = 0; t < T.size(); t++) {
        if (!T[t].used || T[t].parent < 0) continue;
        Tensor &r = T[root_of(T, (int)t)];
        r.first = std::min(r.first, T[t].first);
        r.last = std::max(r.last, T[t].last);
    }
}

// pass 1: the dependency graph checked, consumers counted, dropouts and one-source routes aliased, conv -> [dropout] -> shortcut chains marked
// (every pass reads a shortcut's depend_list[0] unasked: the parser gives a shortcut exactly one source, a route at most four -- shape_layers, ffcnn_host.c)
inline int ffgpu_layout_aliases(const LAYER *ll, int L, const PlanOptions &opt, NetLayout &nl)
{
    for (int i = 0; i < L; i++) {
        if (i > 0 && ll[i].type != LAYER_TYPE_ROUTE) nl.nuses[i - 1]++;
        for (int k = 0; k < ll[i].depend_num; k++) {
            const int d = ll[i].depend_list[k];
            if (d < 0 || d >= i) { ffgpu_set_error("layer %d depends on layer %d (not earlier)", i, d); return -1; }
            nl.nuses[d]++;
        }
    }
    for (int i = 0; i < L; i++) {
        switch (ll[i].type) {
        case LAYER_TYPE_DROPOUT: nl.canon[i] = nl.src(i - 1); break;
        case LAYER_TYPE_YOLO: nl.canon[i] = -2; break;
        case LAYER_TYPE_ROUTE:
            nl.canon[i] = (ll[i].depend_num == 1 && nl.src(ll[i].depend_list[0]) >= -1) ? nl.src(ll[i].depend_list[0]) : i;     // (-1: an alias of the net input)
            break;
        default: nl.canon[i] = i;
        }
        if (opt.fuse && ll[i].type == LAYER_TYPE_SHORTCUT && i > 0) {
            // walk back over dropouts to the producer of our input
            int p = i - 1;
            while (p > 0 && ll[p].type == LAYER_TYPE_DROPOUT && nl.nuses[p] == 1) p--;
            bool chain_private = ll[p].type == LAYER_TYPE_CONV && nl.nuses[p] == 1 && nl.src(ll[i].depend_list[0]) >= 0;
            for (int q = p + 1; q < i && chain_private; q++) chain_private = ll[q].type == LAYER_TYPE_DROPOUT && nl.nuses[q] == 1;
            if (chain_private) { nl.fused_into[p] = i; for (int q = p; q < i; q++) nl.canon[q] = i; }
        }
    }
    return 0;
}

// pass 1b: 1x1 expand -> depthwise 3x3 -> 1x1 project triples that block_ok(p0) takes become ONE fused kernel; the two expanded tensors are
// never materialised
template <class BlockOk>
void ffgpu_layout_irb(const LAYER *ll, int L, NetLayout &nl, BlockOk &&block_ok)
{
    for (int p0 = 0; p0 + 2 < L; p0++) {
        const LAYER &a = ll[p0], &b = ll[p0 + 1], &c = ll[p0 + 2];
        if (a.type != LAYER_TYPE_CONV || b.type != LAYER_TYPE_CONV || c.type != LAYER_TYPE_CONV) continue;
        const bool pw_a = a.fs == 1 && a.stride == 1 && a.pad == 0 && a.groups == 1;
        const bool dw_b = b.fs == 3 && b.pad == 1 && (b.stride == 1 || b.stride == 2) && b.groups == b.c && b.fn == b.c;
        const bool pw_c = c.fs == 1 && c.stride == 1 && c.pad == 0 && c.groups == 1;
        if (!pw_a || !dw_b || !pw_c || nl.nuses[p0] != 1 || nl.nuses[p0 + 1] != 1 || nl.src(p0 - 1) < 0) continue;
        if (nl.canon[p0] != p0 || nl.canon[p0 + 1] != p0 + 1) continue;
        if (!block_ok(p0)) continue;
        nl.irb_tail[p0 + 2] = p0;
        nl.canon[p0] = nl.canon[p0 + 1] = -3;
        p0 += 2;
    }
}

// pass 1b': a maximal run of at least two consecutive fused blocks on one small plane -- 48 -> 224 -> 48 channels, stride 1, at most 128 pixels in at
// most 32 quads of a row, linear projection, a linear shortcut from the block's own input -- becomes ONE launch that keeps the frame on chip
// (ffgpu_irb_stage.inc) where run_ok(the blocks' last layers) takes it.  A block's output may feed the next block alone: any other reader ends the
// run behind that block.  The tensors between the blocks are never materialised: they get no tensor, so no arena range, and cannot be read back.
constexpr int FFGPU_STAGE_MAX_BLOCKS = 8;
template <class RunOk>
void ffgpu_layout_stage(const LAYER *ll, int L, NetLayout &nl, RunOk &&run_ok)
{
    auto linear = [](int act) { return act != 1 && act != 2 && act != 3; };
    // the block that ends at layer t has the stage's shape; its output tensor is the shortcut's
    auto shaped = [&](int t) {
        const int p0 = nl.irb_tail[t], s = nl.fused_into[t];
        if (p0 < 0 || s < 0 || nl.canon[t] != s) return false;
        const LAYER &a = ll[p0], &b = ll[p0 + 1], &c = ll[p0 + 2];
        return a.c == 48 && a.fn == 224 && c.fn == 48 && b.stride == 1 && a.w * a.h <= 128 && (a.w + 3) / 4 * a.h <= 32 &&
               linear(c.activation) && linear(ll[s].activation) && nl.src(ll[s].depend_list[0]) >= 0 && nl.src(ll[s].depend_list[0]) == nl.src(p0 - 1);
    };
    // block tn follows block t: it reads t's output, and nothing outside block tn does
    auto follows = [&](int t, int tn) {
        const int out = nl.canon[t], p0n = nl.irb_tail[tn], sn = nl.fused_into[tn];
        if (nl.src(p0n - 1) != out || ll[p0n].w != ll[nl.irb_tail[t]].w || ll[p0n].h != ll[nl.irb_tail[t]].h ||
            ll[p0n].activation != ll[nl.irb_tail[t]].activation || ll[p0n + 1].activation != ll[nl.irb_tail[t] + 1].activation) return false;
        for (int i = 0; i < L; i++) {
            if (ll[i].type == LAYER_TYPE_DROPOUT || (i >= nl.irb_tail[t] && i <= out) || (i >= p0n && i <= sn)) continue;     // (the two blocks' own layers)
            bool reads = false;
            ffgpu_layer_reads(ll, nl, i, [&](int x) { reads = reads || x == out; });
            if (reads) return false;
        }
        return true;
    };
    for (int t = 0; t < L; t++) {
        if (nl.irb_tail[t] < 0 || !shaped(t)) continue;
        std::vector<int> run(1, t);
        for (int tn = run.back() + 1; tn < L && (int)run.size() < FFGPU_STAGE_MAX_BLOCKS; tn++) {
            if (nl.irb_tail[tn] < 0) continue;
            if (!shaped(tn) || !follows(run.back(), tn)) break;
            run.push_back(tn);
        }
        if (run.size() >= 2 && run_ok(run)) {
            nl.stage_first[run.back()] = nl.irb_tail[run.front()];
            for (size_t k = 0; k + 1 < run.size(); k++) {
                const int out = nl.canon[run[k]];
                nl.stage_inner[run[k]] = 1;
                for (int i = 0; i < L; i++) if (nl.canon[i] == out) nl.canon[i] = -3;
            }
        }
        t = run.back();
    }
}

// pass 1c (opt-in, FFGPU_DWPW=1): depthwise K x K (stride 1) -> 1x1 pairs that no fused block claimed (the heads' 5x5 + 1x1 of yolo-fastest) and
// that pair_ok(p0) takes become one launch (ffgpu_dwpw.inc); the depthwise tensor is never materialised.  MEASURED (r02, tools/dwpw_bench.py):
// correct but SLOWER than the two launches it replaces -- 61 vs 8 + 15 us on 20x20x120 at batch 64 (one workgroup per CU, a barrier chain of 15
// short depthwise / MFMA phases with one wave per SIMD; 147.5 k frames/s end to end against 182.7 k) -- so the planner leaves the pairs alone
// unless asked.
template <class PairOk>
void ffgpu_layout_dwpw(const LAYER *ll, int L, NetLayout &nl, PairOk &&pair_ok)
{
    for (int p0 = 0; p0 + 1 < L; p0++) {
        if (ll[p0].type != LAYER_TYPE_CONV || ll[p0 + 1].type != LAYER_TYPE_CONV) continue;
        if (nl.canon[p0] != p0 || nl.canon[p0 + 1] != p0 + 1 || nl.nuses[p0] != 1 || nl.fused_into[p0] >= 0 || nl.fused_into[p0 + 1] >= 0 || nl.src(p0 - 1) < 0) continue;
        if (!pair_ok(p0)) continue;
        nl.dwpw_tail[p0 + 1] = p0;
        nl.canon[p0] = -3;
        p0++;
    }
}

// the tensors that exist, their sizes, and which layers' own values can be read back.  A route that joins planes of several sizes is refused: the
// parser gives it the last source's plane and the sum of the channels, so its sources, copied or placed behind each other, would not end where it does.
inline int ffgpu_layout_tensors(const LAYER *ll, int L, const PlanOptions &opt, NetLayout &nl)
{
    for (int i = 0; i < L; i++)
        if (nl.canon[i] == i) { nl.tensors[i].used = true; nl.tensors[i].size = (long)ll[i + 1].w * ll[i + 1].h * ll[i + 1].c * opt.batch; }
    for (int i = 0; i < L; i++) {
        if (nl.canon[i] == i) nl.readable[i] = 1;
        else if (ll[i].type == LAYER_TYPE_DROPOUT && i > 0 && nl.canon[i] >= 0 && nl.canon[i] == nl.canon[i - 1]) nl.readable[i] = nl.readable[i - 1];
        else if (ll[i].type == LAYER_TYPE_ROUTE && ll[i].depend_num == 1 && nl.canon[i] >= 0) nl.readable[i] = nl.readable[ll[i].depend_list[0]];
        for (int k = 0; ll[i].type == LAYER_TYPE_ROUTE && nl.canon[i] == i && k < ll[i].depend_num; k++) {
            const LAYER &o = ll[ll[i].depend_list[k] + 1];
            if (nl.src(ll[i].depend_list[k]) < 0 || (o.w == ll[i + 1].w && o.h == ll[i + 1].h)) continue;      // (a source without a tensor: the step builder's refusal)
            ffgpu_set_error("route %d: source layer %d is %d x %d, the route %d x %d", i, ll[i].depend_list[k], o.w, o.h, ll[i + 1].w, ll[i + 1].h);
            return -1;
        }
    }
    return 0;
}

// pass 2: concat in place -- the sources of a multi-source route are allocated inside the route's tensor (each tensor once, none already inside another)
inline void ffgpu_layout_concat(const LAYER *ll, int L, NetLayout &nl)
{
    std::vector<Tensor> &T = nl.tensors;
    for (int i = 0; i < L; i++) {
        if (ll[i].type != LAYER_TYPE_ROUTE || nl.canon[i] != i || ll[i].depend_num < 2) continue;
        bool ok = true;
        std::vector<int> kids;
        for (int k = 0; k < ll[i].depend_num && ok; k++) {
            const int t = nl.src(ll[i].depend_list[k]);
            ok = t >= 0 && T[t].parent < 0 && std::find(kids.begin(), kids.end(), t) == kids.end();
            kids.push_back(t);
        }
        if (!ok) continue;
        long off = 0;
        for (int t : kids) { T[t].parent = i; T[t].parent_off = off; off += T[t].size; }
        nl.route_inplace[i] = 1;
    }
}

// pass 3: lifetimes (in layer-index time), folded onto concat roots
inline void ffgpu_layout_lifetimes(const LAYER *ll, int L, NetLayout &nl)
{
    std::vector<Tensor> &T = nl.tensors;
    auto touch = [&](int t, int when) { if (t >= 0) { T[t].first = std::min(T[t].first, when); T[t].last = std::max(T[t].last, when); } };
    for (int i = 0; i < L; i++) {
        if (ll[i].type == LAYER_TYPE_DROPOUT) continue;
        if (nl.canon[i] >= 0 && !(ll[i].type == LAYER_TYPE_ROUTE && nl.canon[i] != i)) touch(nl.canon[i], i);     // written at i
        ffgpu_layer_reads(ll, nl, i, [&](int t) { touch(t, i); });
    }
    ffgpu_fold_onto_roots(T);
}

// pass 3b: the first detection head runs BESIDE the rest of the net.  In a yolo cfg the layer after a [yolo] is a [route] back to a tensor produced
// at layer r: layers r+1 .. yolo only feed that head, everything after the yolo only depends on layers <= r, so the two chains become parallel
// branches of the HIP graph (the head's 10x10 kernels are latency-bound and hide under the other branch).  Their tensors must then not share arena
// space: every tensor born after the fork, and whatever the side lane READS (its kernels may run late), stays live to the end.
inline void ffgpu_layout_side_lane(const LAYER *ll, int L, NetLayout &nl)
{
    std::vector<Tensor> &T = nl.tensors;
    for (int y = 0; y + 1 < L; y++) {
        if (ll[y].type != LAYER_TYPE_YOLO || ll[y + 1].type != LAYER_TYPE_ROUTE || ll[y + 1].depend_num != 1) continue;
        const int r = ll[y + 1].depend_list[0];
        bool ok = r >= 0 && r < y;
        // nothing after the yolo may read a tensor produced inside (r, y]
        for (int i = y + 1; i < L && ok; i++)
            for (int k = 0; k < ll[i].depend_num; k++) if (ll[i].depend_list[k] > r && ll[i].depend_list[k] <= y) ok = false;
        // nothing inside (r, y] may be a fused block straddling the fork (its first layer must be > r)
        for (int i = r + 1; i <= y && ok; i++) if ((nl.irb_tail[i] >= 0 && nl.irb_tail[i] <= r) || (nl.dwpw_tail[i] >= 0 && nl.dwpw_tail[i] <= r)) ok = false;
        if (ok && nl.fused_into[r] > r) ok = false;       // the fork tensor's producer was absorbed by a later shortcut
        if (!ok) continue;
        nl.side_lo = r + 1; nl.side_hi = y;
        for (int t = 0; t < L; t++) if (T[t].used && T[t].first > r) T[t].last = L + 1;
        for (int i = r + 1; i <= y; i++) ffgpu_layer_reads(ll, nl, i, [&](int t) { if (t >= 0) T[t].last = L + 1; });
        ffgpu_fold_onto_roots(T);
        break;
    }
}

// pass 4: first-fit arena allocation of the roots in order of birth, 256-byte granules; a range is handed on only to a tensor born behind its last use
inline void ffgpu_layout_arena(int L, const PlanOptions &opt, NetLayout &nl)
{
    std::vector<Tensor> &T = nl.tensors;
    struct Live { long off, size; int last; };
    std::vector<Live> live;
    long high = 0;
    std::vector<int> order;
    for (int t = 0; t < L; t++) if (T[t].used && T[t].parent < 0) order.push_back(t);
    std::sort(order.begin(), order.end(), [&](int a, int b) { return T[a].first != T[b].first ? T[a].first < T[b].first : a < b; });
    for (int t : order) {
        const long need = (T[t].size + 63) & ~63L;
        if (opt.keep_all) { T[t].off = high; high += need; continue; }
        live.erase(std::remove_if(live.begin(), live.end(), [&](const Live &l) { return l.last < T[t].first; }), live.end());
        std::sort(live.begin(), live.end(), [](const Live &a, const Live &b) { return a.off < b.off; });
        long at = 0;
        for (const Live &l : live) { if (at + need <= l.off) break; at = std::max(at, l.off + l.size); }
        T[t].off = at;
        live.push_back({ at, need, T[t].last });
        high = std::max(high, at + need);
    }
    nl.arena_floats = (size_t)std::max(high, 64L);
}

// The whole layout of the L layers at ll (L + 1 entries); -1 with a message when the dependency graph or a route is refused.
template <class BlockOk, class PairOk, class RunOk>
int ffgpu_net_layout(const LAYER *ll, int L, const PlanOptions &opt, BlockOk &&block_ok, PairOk &&pair_ok, RunOk &&run_ok, NetLayout &nl)
{
    nl = NetLayout();
    nl.tensors.assign(L, Tensor());
    nl.canon.assign(L, -2);
    nl.readable.assign(L, 0); nl.route_inplace.assign(L, 0);
    nl.nuses.assign(L, 0);
    nl.fused_into.assign(L, -1); nl.irb_tail.assign(L, -1); nl.dwpw_tail.assign(L, -1);
    nl.stage_first.assign(L, -1); nl.stage_inner.assign(L, 0);
    if (ffgpu_layout_aliases(ll, L, opt, nl)) return -1;
    if (opt.fuse && !opt.no_irb) ffgpu_layout_irb(ll, L, nl, block_ok);
    if (opt.fuse && !opt.no_irb && !opt.keep_all && opt.stage) ffgpu_layout_stage(ll, L, nl, run_ok);
    if (opt.fuse && opt.dwpw) ffgpu_layout_dwpw(ll, L, nl, pair_ok);
    if (ffgpu_layout_tensors(ll, L, opt, nl)) return -1;
    if (opt.fuse) ffgpu_layout_concat(ll, L, nl);
    ffgpu_layout_lifetimes(ll, L, nl);
    if (opt.fuse && opt.branch) ffgpu_layout_side_lane(ll, L, nl);
    ffgpu_layout_arena(L, opt, nl);
    return 0;
}

// (without merged runs)
template <class BlockOk, class PairOk>
int ffgpu_net_layout(const LAYER *ll, int L, const PlanOptions &opt, BlockOk &&block_ok, PairOk &&pair_ok, NetLayout &nl)
{
    return ffgpu_net_layout(ll, L, opt, block_ok, pair_ok, [](const std::vector<int> &) { return false; }, nl);
}
