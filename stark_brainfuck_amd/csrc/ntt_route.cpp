// ntt_route.cpp -- which buffer pass 0 of a large out-of-place bfs_gl_ntt() writes to: the remembered routes, their measurement
// (bfs_ntt_tune) and the ownership of the candidate buffers.  Host code only; the passes run through ntt.hip's ntt_run_steps.
#include <algorithm>
#include <cstdio>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "runtime.hpp"

namespace bfs {

// Where pass 0 of a LARGE out-of-place transform writes.  Pass 0 is the one pass that streams one buffer in and another out with
// long strides, and how fast that goes depends on the PAIR of buffers -- some property of their physical placement that user space
// cannot see: 405-510 us for the same launch between different pairs of 1 GiB buffers of one process, while the in-place passes do
// not move (profiles/r03/buffer_placement.txt, profiles/r04/ab_ws_probe.txt; address-translation counters are flat, so it is not the
// TLB).  The library cannot move the caller's buffers, but it can put one of its own in between at no cost in traffic: pass 0 ->
// intermediate, pass 1 intermediate -> output (pass 1 is indifferent to being out of place).
//
// Since round 5 this is OPT-IN (round-4 advice: a measurement hidden inside the third call of a stream-ordered entry point allocated
// three buffers of the transform's size, synchronised the stream and broke under stream capture): a caller that keeps coming back with
// the same (input, output) pair -- the bench step, a prover's pooled buffers -- calls bfs_ntt_tune() ONCE, outside anything it times or
// captures; bfs_gl_ntt itself only looks the pair up and never measures, allocates candidates or synchronises.  ntt_tune times passes
// 0 + 1 on the direct route and through each of NTT_ROUTE_CANDIDATES library buffers in the state the transform will run in, the
// power-limited clock: NTT_ROUTE_WARM untimed rounds over all routes first, then NTT_ROUTE_REPS timed ones, every other one
// backwards, median per route (18 rounds x 8 launches = ~63 ms at 8 x 2^24, one stream synchronisation).  A short probe straight after
// idle (one warm-up round, minimum of four) read 0.89-0.94 ms for routes that run at 0.85 and did not tell fast from slow: 5 of 12
// processes ended on a slow pair against 0 of 12 with the long one (profiles/r04/ab_ws_probe.txt).  Only transforms of >=
// NTT_ROUTE_MIN_BYTES.  A remembered route dies with either buffer: bfs_free / bfs_free_async of a block drops every pair that
// touches it (ntt_route_forget_range, called by the pool), and bfs_ntt_route_forget() is there for memory the library does not own.
// BFS_NTT_WS_PROBE: "0" never route (tune becomes a no-op), "direct" / "buffer0..2" that route for every large transform without
// measuring (the GPU tests run a large transform over every route), "auto" the round-4 behaviour (bfs_gl_ntt tunes a pair by itself
// the third time it sees it).  BFS_NTT_WS_PROBE_LOG=1: the measurements go to stderr.
constexpr int NTT_ROUTE_SIGHTINGS = 3;
#ifndef NTT_ROUTE_WARM
#define NTT_ROUTE_WARM 10
#define NTT_ROUTE_REPS 8
#endif
constexpr u64 NTT_ROUTE_MIN_BYTES = 256ull << 20;
constexpr int ROUTE_UNSEEN = -100;
namespace {
std::mutex g_route_mu;
struct RouteKey {
    int dev; hipStream_t stream; const void* in; const void* out; u64 in_stride, out_stride, shape; u64 in_bytes, out_bytes;
    bool operator<(const RouteKey& o) const {
        return std::tie(dev, stream, in, out, in_stride, out_stride, shape) < std::tie(o.dev, o.stream, o.in, o.out, o.in_stride, o.out_stride, o.shape);
    }
};
std::map<RouteKey, int> g_routes;                       // a route (>= NTT_ROUTE_DIRECT), or ROUTE_UNSEEN - sightings so far ("auto" mode)
std::set<std::pair<int, hipStream_t>> g_candidate_owners;   // (device, stream) pairs that may hold candidate buffers
struct { float us[NTT_ROUTE_CANDIDATES + 1] = {0}; int route = NTT_ROUTE_DIRECT; unsigned long long probes = 0; } g_last_probe;      // (under g_route_mu)
// the candidate buffers no remembered pair of (dev, stream) is routed through go back to the driver; the stream must be idle
void release_unused_candidates_locked(int dev, hipStream_t stream) {
    bool used[NTT_ROUTE_CANDIDATES] = {false};
    for (const auto& kv : g_routes)
        if (kv.first.dev == dev && kv.first.stream == stream && kv.second >= 0) used[kv.second] = true;
    for (int k = 0; k < NTT_ROUTE_CANDIDATES; ++k)
        if (!used[k]) (void)workspace_release(NTT_ROUTE_SLOT0 + k, stream);
}
// hipEvents of one measurement: destroyed on every way out of ntt_tune (the round-4 version leaked all of them when a launch failed)
struct EventGrid {
    std::vector<hipEvent_t> ev;
    int make(size_t count) {
        ev.reserve(count);
        for (size_t i = 0; i < count; ++i) {
            hipEvent_t e = nullptr;
            BFS_HIP(hipEventCreate(&e));
            ev.push_back(e);
        }
        return BFS_OK;
    }
    ~EventGrid() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
};
}
// what the last route measurement of this process read (bfs_ntt_route_probe_info; bench.py prints it next to the step it explains)
int ntt_route_probe_info(float* us, int* route, unsigned long long* probes) {
    std::lock_guard<std::mutex> lock(g_route_mu);
    if (us) for (int k = 0; k <= NTT_ROUTE_CANDIDATES; ++k) us[k] = g_last_probe.us[k];
    if (route) *route = g_last_probe.route;
    if (probes) *probes = g_last_probe.probes;
    return BFS_OK;
}

// forget every remembered pair with a buffer inside [lo, lo + bytes) (bytes == 0: the pair whose buffer STARTS at lo; lo == nullptr:
// everything); candidate buffers that no pair needs any more are freed when `may_free` (the device must then be idle on those streams:
// the callers below synchronise first).  Returns the number of pairs forgotten.
size_t ntt_route_forget_range(const void* lo, size_t bytes, bool may_free) {
    std::lock_guard<std::mutex> lock(g_route_mu);
    size_t gone = 0;
    std::vector<std::pair<int, hipStream_t>> touched;
    for (auto it = g_routes.begin(); it != g_routes.end();) {
        const RouteKey& k = it->first;
        auto hits = [&](const void* p, u64 span) {
            if (lo == nullptr) return true;
            const char *a = (const char*)p, *b = (const char*)lo;
            if (bytes == 0) return a == b;
            return a < b + bytes && b < a + span;
        };
        if (hits(k.in, k.in_bytes) || hits(k.out, k.out_bytes)) {
            touched.emplace_back(k.dev, k.stream);
            it = g_routes.erase(it);
            ++gone;
        } else {
            ++it;
        }
    }
    if (may_free) {
        int cur = 0;
        (void)hipGetDevice(&cur);
        for (const auto& ds : touched) {
            if (ds.first != cur && hipSetDevice(ds.first) != hipSuccess) continue;
            if (hipStreamSynchronize(ds.second) == hipSuccess) release_unused_candidates_locked(ds.first, ds.second);
            else (void)hipGetLastError();
        }
        (void)hipSetDevice(cur);
    }
    return gone;
}

// bfs_pool_trim (the device is idle): candidate buffers that no remembered pair is routed through any more go back to the driver
void ntt_route_trim() {
    std::lock_guard<std::mutex> lock(g_route_mu);
    int cur = 0;
    (void)hipGetDevice(&cur);
    for (const auto& ds : g_candidate_owners)
        if (ds.first == cur) release_unused_candidates_locked(ds.first, ds.second);
}

static RouteKey route_key(int dev, const NttCall& c, u32 log_n) {
    const u64 n = 1ull << log_n;
    return RouteKey{dev, c.stream, c.in, c.out, c.in_stride, c.out_stride, ((u64)log_n << 32) | c.batch,
                    ((u64)(c.batch - 1) * c.in_stride + c.n_in) * sizeof(u64), ((u64)(c.batch - 1) * c.out_stride + n) * sizeof(u64)};
}

// the measurement itself (bfs_ntt_tune, or bfs_gl_ntt in "auto" mode).  Overwrites the output with passes 0 + 1 of the transform,
// synchronises the stream.  *route: NTT_ROUTE_DIRECT, or k >= 0 through candidate buffer k.  Not being able to measure (no memory for
// the candidates) is not an error: the pair stays direct.
static int ntt_measure_route(const NttCall& c, const NttPlan& p, const RouteKey& key, int* route) {
    *route = NTT_ROUTE_DIRECT;
    const bool log = ntt_env().probe_log;
    const hipStream_t stream = c.stream;
    const u64 n = 1ull << p.log_n;
    const size_t bytes = (size_t)n * c.batch * sizeof(u64);
    constexpr int R = NTT_ROUTE_CANDIDATES + 1, REPS = NTT_ROUTE_REPS, WARM = NTT_ROUTE_WARM;
    auto stay_direct = [&](const char* why) {
        if (log) fprintf(stderr, "bfs ntt route: in %p out %p 2^%u x %u: not measured (%s) -> direct\n", (const void*)c.in, (void*)c.out, p.log_n, c.batch, why);
        std::lock_guard<std::mutex> lock(g_route_mu);
        g_routes[key] = NTT_ROUTE_DIRECT;
        return BFS_OK;
    };
    // room for the candidates AND for whatever the caller allocates next: four transform sizes free, or the pair stays direct
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return stay_direct("hipMemGetInfo failed"); }
    size_t held = 0;                                     // candidates of this stream that are already allocated count as free
    {
        void* w = nullptr;
        for (int k = 0; k < NTT_ROUTE_CANDIDATES; ++k)
            if (workspace_peek(NTT_ROUTE_SLOT0 + k, stream, &w, nullptr) && w) held += bytes;
    }
    if (free_b + held < 4 * bytes) return stay_direct("less than four transform sizes of free memory");
    u64* cand[R] = {nullptr};                            // [0]: direct
    { std::lock_guard<std::mutex> lock(g_route_mu); g_candidate_owners.emplace(key.dev, stream); }
    for (int k = 0; k < NTT_ROUTE_CANDIDATES; ++k) {
        void* w = nullptr;
        if (workspace(NTT_ROUTE_SLOT0 + k, bytes, stream, &w) != BFS_OK) {
            (void)hipGetLastError();
            (void)hipStreamSynchronize(stream);
            { std::lock_guard<std::mutex> lock(g_route_mu); g_routes[key] = NTT_ROUTE_DIRECT; release_unused_candidates_locked(key.dev, stream); }
            return stay_direct("no memory for the candidate buffers");
        }
        cand[k + 1] = (u64*)w;
    }
    int rc = BFS_OK;
    float ms[R] = {0};
    {
        EventGrid grid;                                  // REPS x R x {start, stop}; gone when this block ends, however it ends
        rc = grid.make((size_t)REPS * R * 2);
        auto ev = [&](int rep, int r, int which) { return grid.ev[((size_t)rep * R + r) * 2 + which]; };
        // untimed rounds first (a freshly allocated buffer is slow the first time it is written, 1.2 ms against 0.85, and the clock takes
        // tens of ms of load to settle at the power limit), then REPS timed rounds over all routes; the median per route counts
        for (int rep = -WARM; rc == BFS_OK && rep < REPS; ++rep)
            for (int k = 0; rc == BFS_OK && k < R; ++k) {
                // (every other round backwards: while the clock is still ramping after idle, whatever is measured later in a round looks
                //  faster -- the first version always found direct > buffer 0 > buffer 1 > buffer 2, the order it measured them in)
                const int r = (rep & 1) ? R - 1 - k : k;
                if (rep >= 0 && hipEventRecord(ev(rep, r, 0), stream) != hipSuccess) { set_error("hipEventRecord failed in the route measurement"); rc = BFS_ERR_HIP; break; }
                rc = ntt_run_steps(c, p, cand[r], 0, 1);
                if (rc == BFS_OK && rep >= 0 && hipEventRecord(ev(rep, r, 1), stream) != hipSuccess) { set_error("hipEventRecord failed in the route measurement"); rc = BFS_ERR_HIP; }
            }
        if (hipStreamSynchronize(stream) != hipSuccess && rc == BFS_OK) { set_error("hipStreamSynchronize failed in the route measurement"); rc = BFS_ERR_HIP; }
        for (int r = 0; rc == BFS_OK && r < R; ++r) {
            float t[REPS];
            for (int rep = 0; rep < REPS; ++rep)
                if (hipEventElapsedTime(&t[rep], ev(rep, r, 0), ev(rep, r, 1)) != hipSuccess) { set_error("hipEventElapsedTime failed in the route measurement"); rc = BFS_ERR_HIP; break; }
            std::sort(t, t + REPS);
            ms[r] = 0.5f * (t[(REPS - 1) / 2] + t[REPS / 2]);
        }
    }
    if (rc != BFS_OK) {                                   // a failed measurement leaves nothing behind: no events (above), no candidates, no route
        (void)hipGetLastError();
        (void)hipStreamSynchronize(stream);
        std::lock_guard<std::mutex> lock(g_route_mu);
        g_routes.erase(key);
        release_unused_candidates_locked(key.dev, stream);
        return rc;
    }
    int best = 0;
    for (int r = 1; r < R; ++r) if (ms[r] < ms[best]) best = r;
    if (ms[0] <= ms[best] * 1.01f) best = 0;             // the direct route unless an intermediate buffer is clearly faster
    if (log) {
        fprintf(stderr, "bfs ntt route: in %p out %p 2^%u x %u: passes 0+1 direct %.1f us", (const void*)c.in, (void*)c.out, p.log_n, c.batch, ms[0] * 1e3);
        for (int k = 1; k <= NTT_ROUTE_CANDIDATES; ++k) fprintf(stderr, ", via buffer %d (%p) %.1f us", k - 1, (void*)cand[k], ms[k] * 1e3);
        fprintf(stderr, " -> %s\n", best == 0 ? "direct" : (std::string("buffer ") + std::to_string(best - 1)).c_str());
    }
    *route = best - 1;
    // the candidates that lost go back to the driver (the stream is idle: synchronised above).  Slot NTT_ROUTE_SLOT0 + k is buffer k for
    // every pair of this stream, so a buffer another pair was routed through must stay
    {
        std::lock_guard<std::mutex> lock(g_route_mu);
        if (g_routes.size() >= 256 && !g_routes.count(key)) g_routes.clear();
        g_routes[key] = *route;
        for (int r = 0; r < R; ++r) g_last_probe.us[r] = ms[r] * 1e3f;
        g_last_probe.route = *route;
        ++g_last_probe.probes;
        release_unused_candidates_locked(key.dev, stream);
    }
    return BFS_OK;
}

// bfs_gl_ntt's side: the remembered route of the pair, nothing else (unless BFS_NTT_WS_PROBE forces a route or asks for "auto")
int ntt_route(const NttCall& c, const NttPlan& p, int* route) {
    *route = NTT_ROUTE_DIRECT;
    const u64 n = 1ull << p.log_n;
    const NttEnv& env = ntt_env();
    if (c.n_in != n || (u64)n * c.batch * sizeof(u64) < NTT_ROUTE_MIN_BYTES) return BFS_OK;
    if (env.route_mode == NttRouteMode::Forced) { *route = env.forced_route; return BFS_OK; }
    int dev = 0;
    BFS_HIP(hipGetDevice(&dev));
    const RouteKey key = route_key(dev, c, p.log_n);
    {
        std::lock_guard<std::mutex> lock(g_route_mu);
        auto it = g_routes.find(key);
        if (it != g_routes.end() && it->second >= NTT_ROUTE_DIRECT) { *route = it->second; return BFS_OK; }
        if (env.route_mode != NttRouteMode::Auto) return BFS_OK;                 // default: pairs nobody tuned run direct
        if (g_routes.size() >= 256 && it == g_routes.end()) { g_routes.clear(); it = g_routes.end(); }
        int& state = it != g_routes.end() ? it->second : g_routes.emplace(key, ROUTE_UNSEEN).first->second;
        if (ROUTE_UNSEEN - --state < NTT_ROUTE_SIGHTINGS) return BFS_OK;         // "auto": direct until the pair has come back often enough
    }
    return ntt_measure_route(c, p, key, route);
}

// bfs_ntt_tune (include/bfstark.h)
int ntt_tune(const u64* d_in, u64 in_stride, u64* d_out, u64 out_stride, u32 log_n, u32 batch, u64 root, hipStream_t stream, int* route_out) {
    if (route_out) *route_out = NTT_ROUTE_DIRECT;
    if (log_n > 32 || batch == 0 || batch > 65535 || d_in == nullptr || d_out == nullptr) { set_error("bfs_ntt_tune: bad argument"); return BFS_ERR_BAD_ARG; }
    const u64 n = 1ull << log_n;
    if (batch > 1 && (out_stride < n || in_stride < n)) { set_error("bfs_ntt_tune: transforms of a batch overlap"); return BFS_ERR_BAD_ARG; }
    int rc = ntt_check_root(root, log_n);
    if (rc != BFS_OK) { set_error("bfs_ntt_tune: the root is not a primitive 2^%u-th root of unity", log_n); return rc; }
    NttPlan p;
    if (!ntt_make_plan(log_n, root, p)) { set_error("no NTT plan for log_n = %u", log_n); return BFS_ERR_BAD_ARG; }
    if (p.npass < 2 || ntt_buffers_overlap(d_in, n, in_stride, d_out, n, out_stride, batch) || ntt_env().route_mode == NttRouteMode::Forced ||
        (u64)n * batch * sizeof(u64) < NTT_ROUTE_MIN_BYTES)
        return BFS_OK;                                                           // nothing to choose
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone) {
        set_error("bfs_ntt_tune: the stream is being captured (the measurement synchronises it)");
        return BFS_ERR_BAD_ARG;
    }
    (void)hipGetLastError();
    const NttCall c{d_in, n, in_stride, d_out, out_stride, batch, root, 1, 1, (u64)n * batch * sizeof(u64) > NTT_STREAMING_BYTES ? (u32)NTT_NT_ALL : (u32)NTT_NT_NONE, stream};
    int dev = 0;
    BFS_HIP(hipGetDevice(&dev));
    int route = NTT_ROUTE_DIRECT;
    BFS_TRY(ntt_measure_route(c, p, route_key(dev, c, log_n), &route));
    if (route_out) *route_out = route;
    return BFS_OK;
}

}  // namespace bfs
