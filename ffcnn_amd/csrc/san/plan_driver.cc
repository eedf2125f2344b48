// plan_driver.cc -- the planner's layout pass (ffgpu_plan.hpp) on the CPU under AddressSanitizer + UBSan (`make plan`; tests/test_plan_host.py):
//     ffgpu_plan_san <cfg> <batch> <flags> <irb: none|all> <dwpw 0|1> <branch 0|1> [stage 0|1]
// net_load through the host parser and the stub device side (no GPU), then ffgpu_net_layout with callables that take every candidate block / pair
// that passed the layout's own structural test (all) or none of them.  Prints one line per layer -- layer canon readable first last root offset size
// ("-" where the layer has no tensor) --, then "side_lo side_hi arena_floats", then the counts of the rewrites, and checks the invariants I1 - I5
//  itself.  Exit code 0 = the walk ended, whether net_load or the layout accepted or refused the net; 1 = an invariant is violated (named,
// with the layers); a sanitizer report aborts with its own exit code.
// With stage = 1 the layout may merge runs of small-plane blocks (PlanOptions::stage; the callable takes every run or none, like the others): one more
// line per merged run behind the counts, "stage <first layer> <last layer> <blocks>", and invariant I6 on them.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ffcnn.h"
#include "ffcnn_hip.h"
#include "../ffgpu_plan.hpp"

static int g_bad = 0;
#define VIOLATION(...) do { printf("VIOLATION " __VA_ARGS__); printf("\n"); g_bad = 1; } while (0)

static bool disjoint(const NetLayout &nl, int a, int b)
{
    const long a0 = nl.offset_of(a), a1 = a0 + nl.tensors[a].size, b0 = nl.offset_of(b), b1 = b0 + nl.tensors[b].size;
    return a1 <= b0 || b1 <= a0;
}

static void check(const LAYER *ll, int L, const PlanOptions &opt, const NetLayout &nl)
{
    const std::vector<Tensor> &T = nl.tensors;
    std::vector<int> roots;
    for (int t = 0; t < L; t++) if (T[t].used && T[t].parent < 0) roots.push_back(t);
    // I1: EVERY pair of roots
    for (size_t x = 0; x < roots.size(); x++)
        for (size_t y = x + 1; y < roots.size(); y++) {
            const int a = roots[x], b = roots[y];
            const bool meet = T[a].first <= T[b].last && T[b].first <= T[a].last;
            if ((meet || opt.keep_all) && !disjoint(nl, a, b)) VIOLATION("I1: tensors %d and %d are live together and share arena space", a, b);
        }
    // I2: the children of a concat parent
    for (int t = 0; t < L; t++) {
        if (T[t].parent >= 0 && !(T[t].used && nl.route_inplace[T[t].parent] && T[T[t].parent].used)) VIOLATION("I2: tensor %d lies in %d, which is no concat in place", t, T[t].parent);
        if (!nl.route_inplace[t]) continue;
        long off = 0;
        for (int k = 0; k < ll[t].depend_num; k++) {
            const int c = nl.src(ll[t].depend_list[k]);
            if (c < 0 || T[c].parent != t || T[c].parent_off != off) { VIOLATION("I2: source %d of route %d is not at its place inside it", k, t); break; }
            off += T[c].size;
        }
        if (off != T[t].size) VIOLATION("I2: the sources of route %d have %ld floats, the route %ld", t, off, T[t].size);
        for (int c = 0; c < L; c++) {
            bool named = false;
            for (int k = 0; k < ll[t].depend_num; k++) named = named || nl.src(ll[t].depend_list[k]) == c;
            if (T[c].parent == t && !named) VIOLATION("I2: tensor %d lies in route %d, which does not name it", c, t);
        }
    }
    // I3: what a layer reads and writes is live at that layer, and so is the root around it (a dropout launches nothing)
    for (int i = 0; i < L; i++) {
        if (ll[i].type == LAYER_TYPE_DROPOUT) continue;
        auto live = [&](int t, const char *verb) {
            if (t < 0) return;
            const Tensor &r = T[root_of(T, t)];
            if (!T[t].used || T[t].first > i || T[t].last < i || r.first > i || r.last < i) VIOLATION("I3: layer %d %s tensor %d outside its lifetime %d .. %d", i, verb, t, T[t].first, T[t].last);
        };
        ffgpu_layer_reads(ll, nl, i, [&](int t) { live(t, "reads"); });
        if (nl.canon[i] >= 0 && !(ll[i].type == LAYER_TYPE_ROUTE && nl.canon[i] != i)) live(nl.canon[i], "writes");
    }
    // I4
    for (int t = 0; t < L; t++) {
        if (!T[t].used) continue;
        if (T[t].size < 0 || nl.offset_of(t) < 0 || (size_t)(nl.offset_of(t) + T[t].size) > nl.arena_floats) VIOLATION("I4: tensor %d ends outside the arena", t);
        if (T[t].parent < 0 && T[t].off % 64) VIOLATION("I4: tensor %d starts at %ld, no multiple of 64 floats", t, T[t].off);
    }
    for (int i = 0; i < L; i++) if (nl.readable[i] && nl.canon[i] < 0) VIOLATION("I4: layer %d is readable without a tensor", i);
    // I6: a merged run is one launch at its last block: the blocks before it leave no tensor, and the run's input lives until that launch
    for (int i = 0; i < L; i++) {
        if (nl.stage_inner[i] && (nl.canon[i] != -3 || nl.irb_tail[i] < 0 || nl.fused_into[i] < 0 || T[nl.fused_into[i]].used)) VIOLATION("I6: layer %d ends a block inside a merged run and still has a tensor", i);
        if (nl.stage_first[i] < 0) continue;
        const int in = nl.src(nl.stage_first[i] - 1);
        if (in < 0 || nl.canon[i] < 0 || T[in].last < i || !disjoint(nl, root_of(T, in), root_of(T, nl.canon[i]))) VIOLATION("I6: the run that ends at layer %d has no input of its own at its launch", i);
    }
    // I5: the side lane's tensors are nobody's to reuse
    if (nl.side_lo >= 0) {
        std::vector<char> kept(L, 0);
        for (int t = 0; t < L; t++) if (T[t].used && T[t].first >= nl.side_lo) kept[root_of(T, t)] = 1;
        for (int i = nl.side_lo; i <= nl.side_hi; i++) ffgpu_layer_reads(ll, nl, i, [&](int t) { if (t >= 0) kept[root_of(T, t)] = 1; });
        for (int a : roots)
            for (int b : roots)
                if (kept[a] && a != b && T[b].first >= T[a].first && !disjoint(nl, a, b)) VIOLATION("I5: tensor %d of the side lane shares arena space with the later tensor %d", a, b);
    }
}

int main(int argc, char **argv)
{
    if (argc != 7 && argc != 8) { fprintf(stderr, "usage: %s cfg batch flags none|all dwpw branch [stage]\n", argv[0]); return 2; }
    const int flags = atoi(argv[3]);
    const bool take = !strcmp(argv[4], "all");
    PlanOptions opt;
    opt.batch = atoi(argv[2]);
    opt.keep_all = flags & FFGPU_KEEP_ALL; opt.fuse = !(flags & FFGPU_NO_FUSE);
    opt.dwpw = atoi(argv[5]) != 0; opt.branch = atoi(argv[6]) != 0;
    opt.stage = argc == 8 && atoi(argv[7]) != 0;
    if (opt.batch < 1) { fprintf(stderr, "batch must be >= 1\n"); return 2; }
    NET *net = net_load(argv[1], NULL, 0, 0);
    if (!net) { printf("net_load: NULL (%s)\n", ffgpu_last_error()); return 0; }
    const LAYER *ll = net->layer_list;
    const int L = net->layer_num;
    NetLayout nl;
    if (ffgpu_net_layout(ll, L, opt, [&](int) { return take; }, [&](int) { return take; }, [&](const std::vector<int> &) { return take; }, nl)) {
        printf("layout: refused (%s)\n", ffgpu_last_error());
        net_free(net);
        return 0;
    }
    int nfused = 0, nirb = 0, ndwpw = 0, ninplace = 0;
    for (int i = 0; i < L; i++) {
        const int c = nl.canon[i];
        if (c < 0) printf("%d %d %d - - - - -\n", i, c, (int)nl.readable[i]);
        else printf("%d %d %d %d %d %d %ld %ld\n", i, c, (int)nl.readable[i], nl.tensors[c].first, nl.tensors[c].last, root_of(nl.tensors, c), nl.offset_of(c), nl.tensors[c].size);
        nfused += nl.fused_into[i] >= 0; nirb += nl.irb_tail[i] >= 0; ndwpw += nl.dwpw_tail[i] >= 0; ninplace += nl.route_inplace[i] != 0;
    }
    printf("%d %d %zu\n", nl.side_lo, nl.side_hi, nl.arena_floats);
    printf("fused_into %d irb %d dwpw %d inplace %d\n", nfused, nirb, ndwpw, ninplace);
    for (int i = 0; i < L; i++) {
        if (nl.stage_first[i] < 0) continue;
        int blocks = 0;
        for (int t = nl.stage_first[i] + 2; t <= i; t++) blocks += nl.irb_tail[t] >= 0;
        printf("stage %d %d %d\n", nl.stage_first[i], i, blocks);
    }
    check(ll, L, opt, nl);
    net_free(net);
    return g_bad;
}
