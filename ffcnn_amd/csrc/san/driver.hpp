// driver.hpp -- what the stand-alone host-check drivers of this directory share (args, zones, track, streams, text, lines, trails, heat, motion, preview,
// warp, convert; each is one program with its own main, built by `make <name>` under AddressSanitizer + UBSan).  A driver includes the host header it
// checks, then this one, and holds only its fixtures and its table of cases.  Here: the error sink the host headers report into, the counters, the
// printers of a case's line -- id, return value, message, and "   <-- WRONG" where the case did not end as the table says --, made-up addresses, and
// the closing line "<name>_driver: N cases, W wrong" with the exit status.  Included once per program: the sink is a definition.
#pragma once
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>

static char g_err[512];                               // the last message; a case clears it (g_err[0] = 0) before its call
extern "C" void ffgpu_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

static int g_cases, g_wrong;                          // a driver that judges a case itself counts it here too

// One case's line.  rc_ok: the return value is what the table wants.  failed: rc is a failure, so the message is printed and must contain want_msg.
static inline void case_line(const char *id, int rc, bool rc_ok, bool failed, const char *want_msg, bool also = true)
{
    const bool ok = rc_ok && (!failed || strstr(g_err, want_msg)) && also;
    g_cases++;
    g_wrong += !ok;
    printf("%s %d %s%s\n", id, rc, failed ? g_err : "", ok ? "" : "   <-- WRONG");
}
// The two acceptance rules.  Exact: rc == want_rc.  Non-negative: where the table wants success (want_rc >= 0) any rc >= 0 passes -- for checks that
// return a count --, a wanted failure is still exact.  The exact rule comes in two forms, by which return values carry a message: every rc but 0,
// or the negative ones alone (a check that returns a count on success).
static inline void line_exact(const char *id, int rc, int want_rc, const char *want_msg, bool also = true) { case_line(id, rc, rc == want_rc, rc != 0, want_msg, also); }
static inline void line_exact_neg(const char *id, int rc, int want_rc, const char *want_msg) { case_line(id, rc, rc == want_rc, rc < 0, want_msg); }
static inline void line_nonneg(const char *id, int rc, int want_rc, const char *want_msg) { case_line(id, rc, want_rc < 0 ? rc == want_rc : rc >= 0, rc < 0, want_msg); }

static inline void fact(const char *id, bool ok)
{
    g_cases++;
    g_wrong += !ok;
    printf("%s %s\n", id, ok ? "holds" : "fails   <-- WRONG");
}

// made-up addresses, never followed: as an untyped pointer, and as the bytes of a frame's plane
static inline const void *at(uintptr_t a) { return reinterpret_cast<const void *>(a); }
static inline unsigned char *bytes_at(uintptr_t a) { return reinterpret_cast<unsigned char *>(a); }

static inline int finish(const char *name)
{
    printf("%s: %d cases, %d wrong\n", name, g_cases, g_wrong);
    return g_wrong ? 1 : 0;
}
