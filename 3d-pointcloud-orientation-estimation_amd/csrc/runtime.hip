// runtime.hip -- the library's runtime, shared by every API file: the last-error string, the opt-in launch timing behind ProfScope,
// the SyncBN statistics exchange, and the entry points that report on the library itself.  No kernel lives here.
#include <stdarg.h>

#include <map>
#include <string>
#include <vector>

#include "kernels.h"

namespace pnpp {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ---- opt-in launch timing ----------------------------------------------------------------------
struct ProfRec {
    std::string tag;
    hipEvent_t a, b;
};
static bool g_prof = false;
static std::vector<ProfRec> g_recs;
static std::string g_open_tag;   // tag of the open ProfScope; every launch inside it gets its own record
static bool g_scope_open = false;

bool prof_on() { return g_prof; }
void prof_begin(hipStream_t, const char *fmt, ...) {
    char buf[160];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_open_tag = buf;
    g_scope_open = true;
}
void prof_end(hipStream_t) { g_scope_open = false; }
bool prof_take_events(hipEvent_t *a, hipEvent_t *b) {
    if (!g_prof || !g_scope_open) return false;   // a launch outside any scope is not timed
    ProfRec r;
    r.tag = g_open_tag;
    if (hipEventCreate(&r.a) != hipSuccess) return false;
    if (hipEventCreate(&r.b) != hipSuccess) {
        (void)hipEventDestroy(r.a);
        return false;
    }
    g_recs.push_back(r);
    *a = r.a, *b = r.b;
    return true;
}

// ---- SyncBN: optional cross-rank exchange of the BatchNorm sums (off by default) ----------------------------
// The callback sums a device buffer of doubles over the ranks, stream-ordered (RCCL: an all-reduce enqueued behind `stream`).
// The buffer is the caller's (this library never allocates): [0, half) is exchanged, [half, 2 half) keeps this rank's sums.
struct StatsExchange {
    pnpp_stats_exchange_fn fn = nullptr;
    void *user = nullptr;
    double *buf = nullptr;
    size_t half = 0;   // doubles per half
};
static StatsExchange g_sx;

bool stats_sync_on() { return g_sx.fn != nullptr; }
double *stats_buffer_global() { return g_sx.buf; }
double *stats_buffer_local() { return g_sx.buf + g_sx.half; }

int stats_exchange_inplace(int C, hipStream_t st, StatsView *out) {
    PNPP_REQUIRE((size_t)(2 * C + 1) <= g_sx.half, PNPP_ERR_ARG, "stats exchange: buffer of %zu doubles per half is too small for C=%d",
                 g_sx.half, C);
    const int rc = g_sx.fn(g_sx.buf, (size_t)(2 * C + 1), (void *)st, g_sx.user);
    PNPP_REQUIRE(rc == 0, PNPP_ERR_LAUNCH, "stats exchange: the registered callback returned %d", rc);
    out->slab = g_sx.buf, out->nslab = 1, out->count_dev = g_sx.buf + 2 * C, out->local = g_sx.buf + g_sx.half;
    return PNPP_OK;
}

int stats_exchange(const double *slab, int nslab, int C, double count, hipStream_t st, StatsView *out) {
    if (!g_sx.fn) {
        out->slab = slab, out->nslab = nslab, out->count_dev = nullptr, out->local = nullptr;
        return PNPP_OK;
    }
    PNPP_REQUIRE((size_t)(2 * C + 1) <= g_sx.half, PNPP_ERR_ARG, "stats exchange: buffer of %zu doubles per half is too small for C=%d",
                 g_sx.half, C);
    int rc = launch_slab_sum(slab, nslab, C, count, g_sx.buf, g_sx.buf + g_sx.half, st);
    if (rc != PNPP_OK) return rc;
    return stats_exchange_inplace(C, st, out);
}

}  // namespace pnpp

using namespace pnpp;

extern "C" const char *pnpp_last_error(void) { return g_err; }
extern "C" int pnpp_abi_version(void) { return 5; }

extern "C" int pnpp_set_stats_exchange(pnpp_stats_exchange_fn fn, void *user, double *buf, size_t buf_doubles) {
    if (!fn) {
        g_sx = StatsExchange();
        return PNPP_OK;
    }
    PNPP_REQUIRE(buf && buf_doubles >= 2 * (2 * 32 + 1), PNPP_ERR_ARG, "set_stats_exchange: a device buffer of doubles is required");
    g_sx.fn = fn, g_sx.user = user, g_sx.buf = buf, g_sx.half = buf_doubles / 2;
    return PNPP_OK;
}
extern "C" int pnpp_stats_exchange_enabled(void) { return g_sx.fn ? 1 : 0; }

extern "C" int pnpp_profile_enable(int on) {
    for (auto &r : g_recs) {
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    g_recs.clear();
    g_prof = on != 0;
    return PNPP_OK;
}

extern "C" int pnpp_profile_report(char *buf, size_t buflen) {
    PNPP_REQUIRE(buf && buflen > 0, PNPP_ERR_ARG, "profile_report: null buffer");
    std::map<std::string, std::pair<long, double>> agg;
    std::vector<std::string> order;
    for (auto &r : g_recs) {
        float ms = 0.f;
        if (hipEventSynchronize(r.b) != hipSuccess || hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) {
            set_error("profile_report: event query failed");
            return PNPP_ERR_LAUNCH;
        }
        if (!agg.count(r.tag)) order.push_back(r.tag);
        agg[r.tag].first += 1;
        agg[r.tag].second += (double)ms;
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    g_recs.clear();
    size_t off = 0;
    buf[0] = 0;
    for (auto &t : order) {
        int n = snprintf(buf + off, buflen - off, "%s\t%ld\t%.6f\n", t.c_str(), agg[t].first, agg[t].second);
        if (n < 0 || (size_t)n >= buflen - off) break;
        off += (size_t)n;
    }
    return (int)order.size();
}
extern "C" unsigned pnpp_build_flags(void) {
    return gemm_build_flags() | wsp_build_flags() | wsx_build_flags() | wsq_build_flags() | fc_build_flags() | wsf_build_flags() | wsd3_build_flags() |
           mid3_build_flags();
}
