// ntt.hip -- gfx950 kernels and launcher for bfs_gl_ntt() (algorithm and reference citations: ntt_core.hpp)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// the four-instruction subtraction (gl.hpp: gl_sub4, explicit SGPR carries): 6.9 % fewer VALU instructions per launch of the tile kernels,
// 8 x 2^24 1.345 -> 1.31 ms on one box (profiles/r03/ab_sub4.txt)
#define BFS_GL_SUB4
#include "runtime.hpp"

namespace bfs {

// One workgroup per tile: T/16 threads hold 16 elements each.  LDS = tile (padded) + the stage-1 -> stage-2 twiddles.
// Used by single-pass plans (n <= 4096: up to three register stages).
// (A persistent variant with next-tile prefetch and 16-byte paired-lane accesses was measured slower: hardware workgroup turnover
//  already overlaps HBM latency)
template <int B1, int B2, int B3, int LOGC, int MODE, int NT>
__global__ void __launch_bounds__(256) ntt_tile_kernel(const PassArgs a) {
    extern __shared__ __attribute__((aligned(16))) u64 smem[];
    typedef TileCfg<B1, B2, B3, LOGC, MODE> Cfg;
    u64* tw = smem + (B2 > 0 ? ((Cfg::LDS_WORDS + 1) & ~1) : 0);
    // Everything a workgroup needs from memory is requested up front: its entries of the two twiddle tables first (so that
    // waiting for them -- vmcnt counts in order -- does not wait for the data), then the 16 elements of every thread; the
    // tables go to LDS behind ONE barrier while the data is still in flight.  (With the table copies and their two barriers in
    // front of the loads, a workgroup spent an L2 round trip and a half before its HBM loads were even issued.)
    static_assert(B1 == 4, "one sub-group of 16 elements per thread");
    constexpr u32 TW_N = Cfg::U >= 2 ? (1u << (B1 + B2)) : 0;
    const u64* tab = a.tw1;
    const u32 tw_shift = a.tb.t_in_log - (B1 + B2);
    const u32 tid = threadIdx.x;
    // this tile's row of a product table (one coalesced 2^S-entry read per workgroup): factors of its input rows (last pass of a
    // balanced plan) or of its output rows (first pass); never both
    const u64* lrow = tile_load_row<Cfg, LOGC, MODE>(a, blockIdx.x);
    const u64* srow_g = tile_store_row<Cfg, LOGC, MODE>(a, blockIdx.x);
    const u64* row = lrow ? lrow : srow_g;
    const bool has_row = row != nullptr;
    u64 tw0 = 0, rw0 = 0;
    if (TW_N && tid < TW_N) tw0 = tab[(u64)tid << tw_shift];
    if (has_row && tid < (1u << Cfg::S)) rw0 = row[tid];
    u64 x[16];
    ntt_stage1_load<B1, B2, B3, LOGC, MODE, NT>(a, tid, blockIdx.x, blockIdx.y, 0, x);
    u64* rw = tw + Cfg::TW_WORDS;
    if (TW_N && tid < TW_N) tw[tid] = tw0;
    if (has_row && tid < (1u << Cfg::S)) rw[tid] = rw0;
    for (u32 i = tid + blockDim.x; i < TW_N; i += blockDim.x) tw[i] = tab[(u64)i << tw_shift];
    if (has_row)
        for (u32 i = tid + blockDim.x; i < (1u << Cfg::S); i += blockDim.x) rw[i] = row[i];
    const u64* rowtw = lrow ? rw : nullptr;
    const u64* srow = srow_g && !lrow ? rw : nullptr;
    if (Cfg::U >= 2 || has_row) __syncthreads();
    ntt_stage1_compute<B1, B2, B3, LOGC, MODE, NT>(a, smem, tw, rowtw, threadIdx.x, blockIdx.x, blockIdx.y, 0, x, srow);
    if constexpr (B2 > 0) {
        __syncthreads();
        ntt_stage2<B1, B2, B3, LOGC, MODE, NT>(a, smem, threadIdx.x, blockIdx.x, blockIdx.y, srow);
    }
    if constexpr (B3 > 0) {
        __syncthreads();
        ntt_stage3<B1, B2, B3, LOGC, MODE, NT>(a, smem, threadIdx.x, blockIdx.x, blockIdx.y, srow);
    }
}

// Two-stage tiles of multi-pass plans: the stage 1 -> 2 exchange goes through LDS in two halves -- the low
// 32-bit words of all 4096 values, then the high words -- so that the tile buffer is 17 KiB instead of 34 and a workgroup needs
// 21.5 KiB of LDS instead of 39.  With 39 KiB four workgroups (4 waves per SIMD) fit a CU, and a SIMD whose four waves are all
// waiting -- for their loads, at a barrier -- idles: VALU issue was 82 % of the time.  A timing-only experiment (the same kernel
// launched with less LDS than it indexes) put five or more workgroups per CU at 1.34 ms against 1.51 (profiles/r02).  The
// price: 32 + 32 four-byte LDS accesses per thread instead of 16 + 16 eight-byte ones and two more barriers per tile.
// six waves per SIMD asked of the register allocator (80 VGPRs): the store-time row of the balanced schedule took the column
// instantiation from 78 to 82 registers, i.e. from six waves to five (the 5- and 6-bit digits would spill 20 bytes at 80: left as the compiler has them)
#ifndef BFS_NTT_SPLIT_WAVES
#define BFS_NTT_SPLIT_WAVES 6
#endif
template <int B1, int B2, int B3, int LOGC, int MODE, int NT>
__global__ void __launch_bounds__(256, B2 >= 3 ? BFS_NTT_SPLIT_WAVES : 0) ntt_tile_kernel_split(const PassArgs a) {
    static_assert(B1 == 4 && B2 > 0 && B3 == 0, "two register stages, 16 elements per thread");
    extern __shared__ __attribute__((aligned(16))) u64 smem[];
    typedef TileCfg<B1, B2, B3, LOGC, MODE> Cfg;
    constexpr u32 TILE_BYTES = (Cfg::LDS_WORDS * 4 + 15) & ~15u;
    u32* tile = (u32*)smem;
    u64* tw = (u64*)((char*)smem + TILE_BYTES);
    constexpr u32 TW_N = 1u << (B1 + B2);
    const u64* tab = a.tw1;                                                  // n^-1 folded in when this is the last pass
    const u32 tw_shift = a.tb.t_in_log - (B1 + B2);
    const u32 tid = threadIdx.x;
    const u32 bx = blockIdx.x, by = blockIdx.y;
    const u64* lrow = tile_load_row<Cfg, LOGC, MODE>(a, bx);
    const u64* srow_g = tile_store_row<Cfg, LOGC, MODE>(a, bx);
    const u64* row = lrow ? lrow : srow_g;
    const bool has_row = row != nullptr;
    // table entries first, then the data (see ntt_tile_kernel); W = 256 >= both table sizes
    u64 tw0 = 0, rw0 = 0;
    if (tid < TW_N) tw0 = tab[(u64)tid << tw_shift];
    if (has_row && tid < (1u << Cfg::S)) rw0 = row[tid];
    u64 x[16];
    ntt_stage1_load<B1, B2, B3, LOGC, MODE, NT>(a, tid, bx, by, 0, x);
    u64* rw = tw + Cfg::TW_WORDS;
    if (tid < TW_N) tw[tid] = tw0;
    if (has_row && tid < (1u << Cfg::S)) rw[tid] = rw0;
    __syncthreads();
    const u64* srow = srow_g && !lrow ? rw : nullptr;
    ntt_stage1_values<B1, B2, B3, LOGC, MODE>(a, tw, lrow ? rw : nullptr, tid, bx, by, 0, x);
    constexpr int Q2 = 1 << B2, SG2 = 16 / Q2;
    BFS_UNROLL
    for (int m = 0; m < 16; ++m) tile[stage1_out_index<B1, B2, B3, LOGC, MODE>(a, tid, 0, m)] = (u32)x[m];
    __syncthreads();
    u32 lo[16];
    BFS_UNROLL
    for (int s = 0; s < SG2; ++s)
        BFS_UNROLL
        for (int d = 0; d < Q2; ++d) lo[s * Q2 + d] = tile[stage2_in_index<B1, B2, B3, LOGC, MODE>(tid, s, d)];
    __syncthreads();
    BFS_UNROLL
    for (int m = 0; m < 16; ++m) tile[stage1_out_index<B1, B2, B3, LOGC, MODE>(a, tid, 0, m)] = (u32)(x[m] >> 32);
    __syncthreads();
    BFS_UNROLL
    for (int s = 0; s < SG2; ++s) {
        u64 y[Q2];
        BFS_UNROLL
        for (int d = 0; d < Q2; ++d) y[d] = ((u64)tile[stage2_in_index<B1, B2, B3, LOGC, MODE>(tid, s, d)] << 32) | lo[s * Q2 + d];
        ntt_stage2_from<B1, B2, B3, LOGC, MODE, NT>(a, smem, tid, bx, by, s, y, srow);
    }
}

__global__ void ntt_small_kernel(const SmallArgs a) { ntt_small_body(a, threadIdx.x, blockIdx.y); }

// one launch of the instance ntt_with_tile_shape (ntt_plan.hpp) picked: ntt_tile_kernel for single-pass plans, the split exchange for the
// 4096-element tiles of multi-pass plans
template <int B1, int B2, int B3, int LOGC, int MODE>
static int launch_tile(TileShape<B1, B2, B3, LOGC, MODE>, const PassArgs& a, u32 grid_x, u32 batch, hipStream_t stream) {
    typedef TileCfg<B1, B2, B3, LOGC, MODE> Cfg;
    const size_t row_words = (a.tb.row != nullptr || a.tb.srow != nullptr) ? (1u << Cfg::S) : 0;
    if constexpr (MODE == PASS_SINGLE) {
        const size_t lds = (size_t)((B2 > 0 ? ((Cfg::LDS_WORDS + 1) & ~1) + Cfg::TW_WORDS : 0) + row_words) * sizeof(u64);
        if (a.streaming)
            hipLaunchKernelGGL((ntt_tile_kernel<B1, B2, B3, LOGC, MODE, NTT_NT_ALL>), dim3(grid_x, batch), dim3(Cfg::W), lds, stream, a);
        else
            hipLaunchKernelGGL((ntt_tile_kernel<B1, B2, B3, LOGC, MODE, NTT_NT_NONE>), dim3(grid_x, batch), dim3(Cfg::W), lds, stream, a);
    } else {
        const size_t lds = ((Cfg::LDS_WORDS * 4 + 15) & ~15u) + (Cfg::TW_WORDS + row_words) * sizeof(u64);
        // (loads alone non-temporal: pass 0 of the column pipeline, the only launch that asks for it)
        constexpr int NT_FIRST = MODE == PASS_FIRST ? NTT_NT_LOADS : NTT_NT_ALL;
        if (a.streaming == NT_FIRST)
            hipLaunchKernelGGL((ntt_tile_kernel_split<B1, B2, B3, LOGC, MODE, NT_FIRST>), dim3(grid_x, batch), dim3(Cfg::W), lds, stream, a);
        else if (a.streaming)
            hipLaunchKernelGGL((ntt_tile_kernel_split<B1, B2, B3, LOGC, MODE, NTT_NT_ALL>), dim3(grid_x, batch), dim3(Cfg::W), lds, stream, a);
        else
            hipLaunchKernelGGL((ntt_tile_kernel_split<B1, B2, B3, LOGC, MODE, NTT_NT_NONE>), dim3(grid_x, batch), dim3(Cfg::W), lds, stream, a);
    }
    BFS_HIP(hipGetLastError());
    return BFS_OK;
}

enum { TBL_W_LO = 1, TBL_W_HI, TBL_T_IN, TBL_T_IN_LAST, TBL_S_LO, TBL_S_HI, TBL_ROW };

// the product tables of pass t (ntt_row_specs): <= 2^16 entries each (512 KiB, L2 resident), cached per (omega, shape)
static int get_row_tables(const NttPlan& p, u32 t, u64 root, const u64** d_row, const u64** d_srow) {
    *d_row = nullptr;
    *d_srow = nullptr;
    NttRowSpec load, store;
    ntt_row_specs(p, t, root, load, store);
    for (int which = 0; which < 2; ++which) {
        const NttRowSpec& sp = which ? store : load;
        if (sp.omega == 0) continue;
        const u64** out = which ? d_srow : d_row;
        const u64 key = ((u64)sp.a_bits << 24) | ((u64)sp.b_bits << 16) | TBL_ROW;
        if (cached_table_lookup(sp.omega, key, 0, out)) continue;
        std::vector<u64> host;
        ntt_product_table(sp.omega, sp.a_bits, sp.b_bits, host);
        BFS_TRY(cached_table(sp.omega, key, 0, host.data(), host.size(), out));
    }
    return BFS_OK;
}

static int get_tables(const NttPlan& p, u64 root, u64 shift, u64 post_scale, NttTables& tb) {
    tb = NttTables{};
    tb.lo_bits = p.lo_bits;
    tb.t_in_log = p.t_in_log;
    const u64 kb = ((u64)p.log_n << 8);
    bool have = cached_table_lookup(root, kb | TBL_W_LO, 0, &tb.w_lo) && cached_table_lookup(root, kb | TBL_W_HI, 0, &tb.w_hi) &&
                cached_table_lookup(root, kb | TBL_T_IN, 0, &tb.t_in) &&
                cached_table_lookup(root, kb | TBL_T_IN_LAST, post_scale, &tb.t_in_last);
    if (!have) {
        NttHostTables ht;
        ntt_build_tables(p, root, post_scale, ht);
        BFS_TRY(cached_table(root, kb | TBL_W_LO, 0, ht.w_lo.data(), ht.w_lo.size(), &tb.w_lo));
        BFS_TRY(cached_table(root, kb | TBL_W_HI, 0, ht.w_hi.data(), ht.w_hi.size(), &tb.w_hi));
        BFS_TRY(cached_table(root, kb | TBL_T_IN, 0, ht.t_in.data(), ht.t_in.size(), &tb.t_in));
        BFS_TRY(cached_table(root, kb | TBL_T_IN_LAST, post_scale, ht.t_in_last.data(), ht.t_in_last.size(), &tb.t_in_last));
    }
    if (shift != 1) {
        if (!(cached_table_lookup(shift, kb | TBL_S_LO, 0, &tb.s_lo) && cached_table_lookup(shift, kb | TBL_S_HI, 0, &tb.s_hi))) {
            CosetHostTables ct;
            ntt_build_coset_tables(p, shift, ct);
            BFS_TRY(cached_table(shift, kb | TBL_S_LO, 0, ct.s_lo.data(), ct.s_lo.size(), &tb.s_lo));
            BFS_TRY(cached_table(shift, kb | TBL_S_HI, 0, ct.s_hi.data(), ct.s_hi.size(), &tb.s_hi));
        }
    }
    return BFS_OK;
}

// (runtime.hpp; shared with the fold and the constraint kernels)
int ntt_power_tables(u64 root, u32 log_n, const u64** lo, const u64** hi, u32* lo_bits) {
    NttPlan p;
    if (!ntt_make_plan(log_n, root, p)) { set_error("no table plan for log_n = %u", log_n); return BFS_ERR_BAD_ARG; }
    NttTables tb;
    BFS_TRY(get_tables(p, root, 1, 1, tb));
    *lo = tb.w_lo; *hi = tb.w_hi; *lo_bits = tb.lo_bits;
    return BFS_OK;
}

// the pass runner: steps first..last of the schedule of plan p over the call's buffers (which step reads and writes what: ntt_make_schedule)
// every table the steps of one call read: fetched once per call (each lookup takes the table cache's lock), whatever the number of
// launches the call is then made of
struct NttCallTables {
    NttTables tb;
    const u64* row[4];
    const u64* srow[4];
};
static int get_call_tables(const NttCall& c, const NttPlan& p, NttCallTables& t) {
    BFS_TRY(get_tables(p, c.root, c.shift, c.post_scale, t.tb));
    for (u32 pass = p.expand ? 1 : 0; pass < p.npass && pass < 4; ++pass) BFS_TRY(get_row_tables(p, pass, c.root, &t.row[pass], &t.srow[pass]));   // (the passes of ntt_make_schedule)
    return BFS_OK;
}
// nt_in: the NTT_NT_* mask of the step that reads the caller's input; every other step takes c.streaming
static int run_steps(const NttCall& c, const NttPlan& p, u64* mid, u32 first, u32 last, const NttCallTables& t, u32 nt_in) {
    const NttSchedule s = ntt_make_schedule(p, c.n_in, mid != nullptr);
    const struct { u64* ptr; u64 stride; } buf[3] = {{const_cast<u64*>(c.in), c.in_stride}, {c.out, c.out_stride}, {mid, 1ull << p.log_n}};
    NttTables tb = t.tb;
    for (u32 k = first; k <= last && k < s.nsteps; ++k) {
        const NttStep& st = s.step[k];
        tb.row = t.row[st.pass];
        tb.srow = t.srow[st.pass];
        PassArgs a = ntt_pass_args(p, st.pass, buf[st.src].ptr, buf[st.dst].ptr, buf[st.src].stride, buf[st.dst].stride, st.count, tb, c.shift != 1, c.shift, c.post_scale);
        a.streaming = st.src == NTT_BUF_IN ? nt_in : c.streaming;
        const int rc = ntt_with_tile_shape(st.mode, st.S, [&](auto shape) { return launch_tile(shape, a, st.grid_x, c.batch, c.stream); });
        if (rc == BFS_ERR_BAD_ARG) set_error("internal: no tile kernel for a %u-bit digit in mode %u", st.S, st.mode);
        BFS_TRY(rc);
    }
    return BFS_OK;
}
int ntt_run_steps(const NttCall& c, const NttPlan& p, u64* mid, u32 first, u32 last) {
    NttCallTables t;
    BFS_TRY(get_call_tables(c, p, t));
    return run_steps(c, p, mid, first, last, t, c.streaming);
}

// The column pipeline.  A batch of three-pass transforms of 64-128 MiB each runs COLUMN BY COLUMN, even columns on the caller's
// stream and odd ones on the library's second stream of that stream (runtime.cpp: stream_pair): a column's three passes follow each
// other on one stream, so the column it is building stays in the 256 MiB Infinity Cache from its pass 0 to its pass 2 instead of
// going to HBM and back twice, and while one column runs its in-place passes out of the cache the other stream's pass 0 uses the HBM
// bandwidth they leave idle.  Exactly two streams: three and four measured slower than two, one stream slower than one launch per
// pass for the whole batch (profiles/r04/ab_l3_pipeline.txt: launch tails).  The second stream is forked from the caller's with an
// event before the first launch and joined back after the last, so the call stays ordered on the caller's stream like any other;
// the join is enqueued on every way out, a failed launch included, so that nothing the helper already holds can be overtaken.
// Cache policy (profiles/ntt_column_pipeline.md): pass 0 reads the caller's input once, non-temporal, so that it does not evict the
// columns in flight; everything else is an ordinary access.  BFS_NTT_STREAMING=0 / 1 forces all-ordinary / all-non-temporal.
static int ntt_run_columns(const NttCall& c, const NttPlan& p) {
    const NttEnv& env = ntt_env();
    StreamPair sp;
    BFS_TRY(stream_pair(c.stream, &sp));
    NttCallTables t;
    BFS_TRY(get_call_tables(c, p, t));
    const u32 nt_rest = env.force_streaming > 0 ? NTT_NT_ALL : NTT_NT_NONE;
    const u32 nt_in = env.force_streaming >= 0 ? nt_rest : NTT_NT_LOADS;
    BFS_HIP(hipEventRecord(sp.fork, c.stream));
    BFS_HIP(hipStreamWaitEvent(sp.helper, sp.fork, 0));
    int rc = BFS_OK;
    for (u32 col = 0; rc == BFS_OK && col < c.batch; ++col) {
        NttCall one = c;
        one.in = c.in + (u64)col * c.in_stride;
        one.out = c.out + (u64)col * c.out_stride;
        one.batch = 1;
        one.streaming = nt_rest;
        one.stream = (col & 1) ? sp.helper : c.stream;
        rc = run_steps(one, p, nullptr, 0, 3, t, nt_in);
    }
    if (hipEventRecord(sp.join, sp.helper) != hipSuccess || hipStreamWaitEvent(c.stream, sp.join, 0) != hipSuccess) {
        if (rc == BFS_OK) { set_error("bfs_gl_ntt: joining the column pipeline's second stream failed"); rc = BFS_ERR_HIP; }
    }
    return rc;
}

const NttEnv& ntt_env() {
    static const NttEnv env = [] {
        NttEnv v{NttRouteMode::Remembered, NTT_ROUTE_DIRECT, false, -1, true, false, NttPipeline::BySize};
        if (const char* e = getenv("BFS_NTT_WS_PROBE")) {
            if (e[0] == '0' || !strcmp(e, "direct")) v.route_mode = NttRouteMode::Forced;
            else if (!strncmp(e, "buffer", 6) && e[6] >= '0' && e[6] < '0' + NTT_ROUTE_CANDIDATES && !e[7]) { v.route_mode = NttRouteMode::Forced; v.forced_route = e[6] - '0'; }
            else if (!strcmp(e, "auto") || !strcmp(e, "1")) v.route_mode = NttRouteMode::Auto;
        }
        if (const char* e = getenv("BFS_NTT_WS_PROBE_LOG")) v.probe_log = e[0] == '1';
        if (const char* e = getenv("BFS_NTT_STREAMING")) v.force_streaming = atoi(e);
        if (const char* e = getenv("BFS_NTT_EXPAND")) v.allow_expand = e[0] != '0';
        v.plan_log = getenv("BFS_NTT_PLAN_LOG") != nullptr;
        if (const char* e = getenv("BFS_NTT_PIPELINE")) v.pipeline = !strcmp(e, "force") ? NttPipeline::Forced : e[0] == '0' ? NttPipeline::Off : NttPipeline::BySize;
        return v;
    }();
    return env;
}

int ntt_launch(const u64* d_in, u64 n_in, u64 in_stride, u64* d_out, u64 out_stride, u32 log_n, u32 batch, u64 root,
               u64 shift, u64 post_scale, hipStream_t stream) {
    if (log_n > 32) { set_error("field has no 2^%u-th root of unity (algebra.py:124-125)", log_n); return BFS_ERR_BAD_ARG; }
    const u64 n = 1ull << log_n;
    if (n_in > n) { set_error("more coefficients (%llu) than the evaluation order (%llu)", (unsigned long long)n_in, (unsigned long long)n); return BFS_ERR_TOO_MANY_COEFFS; }
    if (batch == 0) return BFS_OK;
    if (d_out == nullptr || (d_in == nullptr && n_in != 0)) { set_error("bfs_gl_ntt: null device pointer"); return BFS_ERR_BAD_ARG; }
    if (batch > 1 && (out_stride < n || in_stride < n_in)) {
        set_error("bfs_gl_ntt: transforms of a batch overlap (in_stride %llu < %llu coefficients or out_stride %llu < n = %llu)",
                  (unsigned long long)in_stride, (unsigned long long)n_in, (unsigned long long)out_stride, (unsigned long long)n);
        return BFS_ERR_BAD_ARG;
    }
    if (log_n <= NTT_TILE_LOG && n_in != 0) {
        // No pass or one: one workgroup per transform, which loads all it reads before it stores anything, so a transform may
        // overwrite its OWN input (d_in == d_out with equal strides).  Any other overlap lets transform b write where another
        // transform, possibly of a workgroup that has not started yet, still has to read: the input goes through the library
        // buffer first (multi-pass plans stage such calls below).  Decided on the whole batch, before it is sliced.
        if (ntt_buffers_overlap(d_in, n_in, in_stride, d_out, n, out_stride, batch) && !(d_in == d_out && in_stride == out_stride)) {
            void* w = nullptr;
            const size_t span = (size_t)((u64)(batch - 1) * in_stride + n_in) * sizeof(u64);
            BFS_TRY(workspace(0, span, stream, &w));
            BFS_HIP(hipMemcpyAsync(w, d_in, span, hipMemcpyDeviceToDevice, stream));
            d_in = (const u64*)w;
        }
    }
    if (batch > 65535) {
        // grid.y carries the batch index and is limited to 65535: larger batches go in slices (transforms are independent)
        for (u32 done = 0; done < batch;) {
            const u32 part = batch - done < 65535 ? batch - done : 65535;
            BFS_TRY(ntt_launch(d_in + (u64)done * in_stride, n_in, in_stride, d_out + (u64)done * out_stride, out_stride, log_n, part, root,
                               shift, post_scale, stream));
            done += part;
        }
        return BFS_OK;
    }
    int rc = ntt_check_root(root, log_n);
    if (rc == BFS_ERR_NOT_ROOT) { set_error("primitive root must be nth root of unity, where n is %llu", (unsigned long long)n); return rc; }
    if (rc == BFS_ERR_NOT_PRIMITIVE) { set_error("primitive root %llu is not primitive nth root of unity, where n is %llu", (unsigned long long)root, (unsigned long long)n); return rc; }
    const NttEnv& env = ntt_env();
    // input and output overlapping (a transform "in place" for the caller): a multi-pass plan then goes through the library's buffer
    const bool overlap = log_n > NTT_TILE_LOG && n_in != 0 && ntt_buffers_overlap(d_in, n_in, in_stride, d_out, n, out_stride, batch);
    NttPlan p;
    if (!ntt_choose_plan(log_n, n_in, root, overlap, env.allow_expand, p)) { set_error("no NTT plan for log_n = %u", log_n); return BFS_ERR_BAD_ARG; }
    if (p.npass == 0) {
        SmallArgs a{d_in, d_out, in_stride, out_stride, n_in, log_n, root, shift, post_scale};
        hipLaunchKernelGGL(ntt_small_kernel, dim3(1, batch), dim3(64), 0, stream, a);
        BFS_HIP(hipGetLastError());
        return BFS_OK;
    }
    // non-temporal data accesses once a buffer of the call no longer fits the Infinity Cache next to its neighbours (ntt_core.hpp)
    const bool nt = env.force_streaming >= 0 ? env.force_streaming != 0 : (u64)n * batch * sizeof(u64) > NTT_STREAMING_BYTES;
    const u32 streaming = nt ? NTT_NT_ALL : NTT_NT_NONE;
    const NttCall c{d_in, n_in, in_stride, d_out, out_stride, batch, root, shift, post_scale, streaming, stream};
    if (env.plan_log) fprintf(stderr, "ntt plan: log_n %u n_in %llu batch %u overlap %d allow %d in %p out %p\n", log_n, (unsigned long long)n_in, batch, (int)overlap, (int)env.allow_expand, (const void*)d_in, (void*)d_out);
    // Large out-of-place transforms: which buffer pass 0 writes to is chosen by measurement (ntt_route.cpp)
    int route = NTT_ROUTE_DIRECT;
    if (!overlap && !p.expand && p.npass > 1) BFS_TRY(ntt_route(c, p, &route));
    // Column by column on two streams (ntt_run_columns) where a column fits the Infinity Cache and two of them just do not: full-size
    // out-of-place batches of three-pass transforms of 64-128 MiB each; BFS_NTT_PIPELINE=force: of any multi-pass transform (what
    // lets the tests be small), =0: never.  A stream that is being captured keeps one launch per pass: the second stream and its
    // events are not part of the caller's graph.  The pipeline writes pass 0 straight to the output: a remembered route through an
    // intermediate buffer is ignored here, since a third 128 MiB buffer per column is what the cache has no room for.
    bool columns = batch >= 2 && !overlap && !p.expand && n_in == n && env.pipeline != NttPipeline::Off &&
                   (env.pipeline == NttPipeline::Forced ? p.npass >= 2 : p.npass == 3 && n * sizeof(u64) >= NTT_PIPELINE_MIN_BYTES && n * sizeof(u64) <= NTT_PIPELINE_MAX_BYTES);
    if (columns) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(stream, &cap) != hipSuccess) { (void)hipGetLastError(); columns = false; }
        else if (cap != hipStreamCaptureStatusNone) columns = false;
    }
    if (env.plan_log) fprintf(stderr, "ntt route: %s\n", columns ? "pipelined columns" : overlap ? "staged" : p.expand ? "expansion" : route >= 0 ? "single launch via buffer" : "single launch");
    if (columns) return ntt_run_columns(c, p);
    u64* mid = nullptr;
    if (overlap || route >= 0) {
        void* w = nullptr;
        BFS_TRY(workspace(route >= 0 ? NTT_ROUTE_SLOT0 + route : 0, (size_t)n * batch * sizeof(u64), stream, &w));
        mid = (u64*)w;
    }
    return ntt_run_steps(c, p, mid, 0, 3);
}

}  // namespace bfs
