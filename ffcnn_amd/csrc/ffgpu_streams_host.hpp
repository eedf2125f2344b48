// ffgpu_streams_host.hpp -- what the per-stream passes (track, zones, trails, heat, motion) share on the host.  A record is "the next frame of video
// stream streams[t]" (-1: ignored); each family keeps a block of state per stream in device memory and sends its records to the kernel in chunks, as
// a by-value table grouped by stream.  Here: that table and the grouping behind it, the checks of ntargets / nstreams / the state / the streams, and
// the bytes a reset clears.  Plain C++17 with no HIP in it: every function reports through ffgpu_set_error and touches no device, so
// san/streams_driver.cc runs the same lines on the CPU under ASan + UBSan (tests/test_streams_host.py).
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>

extern "C" void ffgpu_set_error(const char *fmt, ...);

// The records t0 .. t0 + nt - 1 of a call grouped by video stream: order[i] = the i-th record in "stream ascending, record order kept inside a
// stream"; group g (= workgroup g) serves stream gstream[g] (-1: the ignored entries) with order[goff[g] .. goff[g + 1] - 1].
// Returns the number of groups.
inline int ffgpu_group_by_stream(const int *streams, int t0, int nt, int *order, int *gstream, int *goff)
{
    for (int i = 0; i < nt; i++) order[i] = t0 + i;
    std::stable_sort(order, order + nt, [&](int x, int y) { return streams[x] < streams[y]; });
    int ng = 0;
    for (int i = 0; i < nt; i++)
        if (i == 0 || streams[order[i]] != streams[order[i - 1]]) { gstream[ng] = streams[order[i]]; goff[ng] = i; ng++; }
    goff[ng] = nt;
    return ng;
}

// The entries of one launch as the stream kernels read them: N records at most, the first member of the family's by-value kernel argument.  The
// table is 5 N + 1 words, an odd number: with 8-byte aligned list starts a word of padding would follow it and move whatever the family puts next.
// So the starts are 4-byte aligned here, and the kernel-argument bytes lie where they lay when the four arrays were each family's own.
typedef long long stream_first_t __attribute__((aligned(4)));
template <int N> struct StreamEntries {
    stream_first_t first[N];                          // entry e: its list's first box in `lists`
    int   rec[N];                                     //          its record
    int   gstream[N];                                 // group g (= workgroup g): its video stream, or -1: the ignored entries
    int   goff[N + 1];                                //          its entries goff[g] .. goff[g + 1] - 1
};
static_assert(sizeof(StreamEntries<64>) == 4 * (5 * 64 + 1) && sizeof(StreamEntries<128>) == 4 * (5 * 128 + 1) && alignof(StreamEntries<64>) == 4, "no padding");

// the table of the records t0 .. t0 + nt - 1 (nt <= N; first: DetSource::first, one per record of the call); returns the number of groups
template <int N> int ffgpu_stream_entries(const std::vector<long long> &first, const int *streams, int t0, int nt, StreamEntries<N> &en)
{
    const int ng = ffgpu_group_by_stream(streams, t0, nt, en.rec, en.gstream, en.goff);
    for (int i = 0; i < nt; i++) en.first[i] = first[(size_t)en.rec[i]];
    return ng;
}

// ntargets, nstreams and the state's alignment, in this order (the state is not NULL: the caller's check)
inline int ffgpu_streams_check(const char *what, int ntargets, int nstreams, const void *d_state)
{
    if (ntargets < 1 || ntargets > (1 << 24)) { ffgpu_set_error("%s: %d targets (ntargets >= 1)", what, ntargets); return -1; }
    if (nstreams < 1 || nstreams > 65536) { ffgpu_set_error("%s: nstreams %d is outside 1..65536", what, nstreams); return -1; }
    if (reinterpret_cast<uintptr_t>(d_state) & 15) { ffgpu_set_error("%s: the state must be 16-byte aligned", what); return -1; }
    return 0;
}

// every target's stream is -1 or one of the nstreams
inline int ffgpu_stream_range_check(const char *what, const int *streams, int ntargets, int nstreams)
{
    for (int t = 0; t < ntargets; t++)
        if (streams[t] < -1 || streams[t] >= nstreams) { ffgpu_set_error("%s: target %d: stream %d is outside -1 .. %d", what, t, streams[t], nstreams - 1); return -1; }
    return 0;
}

// What a reset clears: stream which_stream's block of a state of `all` bytes over nstreams streams, or all of it (-1).  all == 0: the family's
// arguments give no state; the family has set its message for that before the call, and it stands unless the state is NULL.
inline int ffgpu_state_span(const char *what, const void *d_state, size_t all, int nstreams, int which_stream, size_t &off, size_t &len)
{
    if (!d_state) { ffgpu_set_error("%s: NULL state", what); return -1; }
    if (!all) return -1;
    if (reinterpret_cast<uintptr_t>(d_state) & 15) { ffgpu_set_error("%s: the state must be 16-byte aligned", what); return -1; }
    if (which_stream < -1 || which_stream >= nstreams) { ffgpu_set_error("%s: stream %d is outside -1 .. %d", what, which_stream, nstreams - 1); return -1; }
    const size_t one = all / (size_t)nstreams;
    off = which_stream < 0 ? 0 : one * (size_t)which_stream;
    len = which_stream < 0 ? all : one;
    return 0;
}
