// Host emulation of the NTT tile kernels (TEST INFRASTRUCTURE, never part of the product path).
// Compiles stark_brainfuck_amd/csrc/ntt_core.hpp for the host and runs every (block, thread) of every pass
// sequentially, stage by stage -- __syncthreads() becomes "finish the stage for all threads of the block".
// Lets tests/test_emulation.py check the planner and all index/twiddle arithmetic against the oracle on CPU.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../stark_brainfuck_amd/csrc/ntt_plan.hpp"

using namespace bfs;

template <int B1, int B2, int B3, int LOGC, int MODE>
static int run_pass(TileShape<B1, B2, B3, LOGC, MODE>, const PassArgs& a, u32 grid_x, u32 batch) {
    typedef TileCfg<B1, B2, B3, LOGC, MODE> Cfg;
    std::vector<u64> smem(Cfg::LDS_WORDS + 2);
    // dense stage-1 -> stage-2 twiddle table, as the kernel builds it in LDS
    std::vector<u64> tw(1u << (B1 + B2));
    const u64* tab = a.tw1;
    if (B2 > 0) for (u32 i = 0; i < tw.size(); ++i) tw[i] = tab[(u64)i << (a.tb.t_in_log - (B1 + B2))];
    for (u32 by = 0; by < batch; ++by)
        for (u32 bx = 0; bx < grid_x; ++bx) {
            // the tile's row of the load-time / store-time product table, copied as the kernel copies it to LDS
            std::vector<u64> row, srow_copy;
            const u64* lrow = tile_load_row<Cfg, LOGC, MODE>(a, bx);
            const u64* srow_g = tile_store_row<Cfg, LOGC, MODE>(a, bx);
            if (lrow) row.assign(lrow, lrow + (1u << Cfg::S));
            if (srow_g) srow_copy.assign(srow_g, srow_g + (1u << Cfg::S));
            const u64* rowtw = lrow ? row.data() : nullptr;
            const u64* srow = srow_g && !lrow ? srow_copy.data() : nullptr;
            for (u32 t = 0; t < (u32)Cfg::W; ++t) ntt_stage1<B1, B2, B3, LOGC, MODE>(a, smem.data(), tw.data(), rowtw, t, bx, by, srow);
            if (B2 > 0) for (u32 t = 0; t < (u32)Cfg::W; ++t) ntt_stage2<B1, B2, B3, LOGC, MODE>(a, smem.data(), t, bx, by, srow);
            if (B3 > 0) for (u32 t = 0; t < (u32)Cfg::W; ++t) ntt_stage3<B1, B2, B3, LOGC, MODE>(a, smem.data(), t, bx, by, srow);
        }
    return 0;
}

static int emu_allow_expand = 1;
static unsigned long long emu_expand_plans = 0;
// 0: zero-padded transforms take the plain plan too; returns how many calls have taken the expansion plan so far
extern "C" unsigned long long emu_set_expand(int allow) { emu_allow_expand = allow; return emu_expand_plans; }
static int emu_force_ws = 0;
extern "C" void emu_set_force_ws(int v) { emu_force_ws = v; }
// operands that had to be canonical and were not, since the last reset (gl.hpp, BFS_CHECK_CANONICAL)
extern "C" unsigned long long emu_canonical_violations(int reset) {
    const unsigned long long c = gl_canonical_violations();
    if (reset) gl_canonical_violations() = 0;
    return c;
}

// Sites of the tile kernels (ntt_core.hpp: BFS_NTT_SITE; tests/ntt_planted.py).  mode 0: off, 1: PLANT -- every thread that reaches the
// butterflies of (pass, stage) has its registers overwritten from buf, in call order --, 2: RECORD -- they are copied to buf.  `words`
// is the room in buf; the counts restart.  emu_site_words: the words planted / recorded since then; *overrun: the words the site asked
// for beyond the room (none of them was read or written).
extern "C" void emu_site_control(int mode, u32 pass, u32 stage, u64* buf, u64 words) {
    NttSiteControl& c = ntt_site_control();
    c.mode = mode; c.pass = pass; c.stage = stage; c.buf = buf; c.capacity = words; c.words = 0; c.overrun = 0;
}
extern "C" unsigned long long emu_site_words(unsigned long long* overrun) {
    const NttSiteControl& c = ntt_site_control();
    if (overrun) *overrun = c.overrun;
    return c.words;
}
// the event counters of gl.hpp: out[slot * events + event], slot 0 = before the first site of a call, slot 1 + 3 * pass + (stage - 1);
// returns the number of events per slot, *slots the number of slots (out may be null to ask for the shape)
extern "C" int emu_site_events(int reset, unsigned long long* out, int* slots) {
    GlSiteEvents& e = gl_site_events();
    if (slots) *slots = GL_SITE_SLOTS;
    if (out) memcpy(out, e.count, sizeof(e.count));
    if (reset) { memset(e.count, 0, sizeof(e.count)); e.slot = 0; }
    return GL_EV_COUNT;
}

extern "C" int emu_gl_ntt(const u64* in, u64 n_in, u64 in_stride, u64* out, u64 out_stride, u32 log_n, u32 batch,
                          u64 root, u64 shift, u64 post_scale) {
    gl_site_events().slot = 0;      // what runs before the first site (the tables) belongs to no site
    int rc = ntt_check_root(root, log_n);
    if (rc) return rc;
    const u64 n = 1ull << log_n;
    if (n_in > n) return BFS_ERR_TOO_MANY_COEFFS;
    // the product's decisions (ntt.hip: ntt_launch makes the same three calls): overlapping in / out of a multi-pass plan go through an
    // intermediate buffer in passes 0 and 1, and `force_ws` lets a test take that route with separate buffers too
    const bool overlap = log_n > NTT_TILE_LOG && n_in != 0 && (ntt_buffers_overlap(in, n_in, in_stride, out, n, out_stride, batch) || emu_force_ws);
    NttPlan p;
    if (!ntt_choose_plan(log_n, n_in, root, overlap, emu_allow_expand != 0, p)) return BFS_ERR_BAD_ARG;
    if (p.npass == 0) {
        SmallArgs a{in, out, in_stride, out_stride, n_in, log_n, root, shift, post_scale};
        for (u32 b = 0; b < batch; ++b)
            for (u32 k = 0; k < n; ++k) ntt_small_body(a, k, b);
        return 0;
    }
    emu_expand_plans += p.expand;
    NttHostTables ht;
    ntt_build_tables(p, root, post_scale, ht);
    CosetHostTables ct;
    const bool coset = shift != 1;
    if (coset) ntt_build_coset_tables(p, shift, ct);
    NttTables tb{ht.w_lo.data(), ht.w_hi.data(), p.lo_bits, p.t_in_log, ht.t_in.data(), ht.t_in_last.data(),
                 coset ? ct.s_lo.data() : nullptr, coset ? ct.s_hi.data() : nullptr, nullptr, nullptr};
    std::vector<u64> mid;
    if (overlap) mid.resize((size_t)n * batch);
    const NttSchedule s = ntt_make_schedule(p, n_in, overlap);
    const struct { u64* ptr; u64 stride; } buf[3] = {{const_cast<u64*>(in), in_stride}, {out, out_stride}, {mid.data(), n}};
    for (u32 k = 0; k < s.nsteps; ++k) {
        const NttStep& st = s.step[k];
        std::vector<u64> row, srow;
        NttRowSpec load, store;
        ntt_row_specs(p, st.pass, root, load, store);
        tb.row = nullptr; tb.srow = nullptr;
        if (load.omega) { ntt_product_table(load.omega, load.a_bits, load.b_bits, row); tb.row = row.data(); }
        if (store.omega) { ntt_product_table(store.omega, store.a_bits, store.b_bits, srow); tb.srow = srow.data(); }
        const PassArgs a = ntt_pass_args(p, st.pass, buf[st.src].ptr, buf[st.dst].ptr, buf[st.src].stride, buf[st.dst].stride, st.count, tb, shift != 1, shift, post_scale);
        if (ntt_with_tile_shape(st.mode, st.S, [&](auto shape) { return run_pass(shape, a, st.grid_x, batch); })) abort();
    }
    return 0;
}

// the step list a call would run (no arithmetic): row k of `steps` = {pass, mode, S, logC, grid_x, src, dst, count} of step k, src / dst
// 0 input, 1 output, 2 intermediate; *virtual_bits = the digit an expansion plan skips (0: plain plan).  Returns the number of steps, -1: no plan
extern "C" int emu_schedule(u32 log_n, u64 n_in, u64 root, int via_mid, int allow_expand, u64* steps, u32* virtual_bits) {
    NttPlan p;
    if (!ntt_choose_plan(log_n, n_in, root, via_mid != 0, allow_expand != 0, p)) return -1;
    const NttSchedule s = ntt_make_schedule(p, n_in, via_mid != 0);
    *virtual_bits = p.expand ? p.pass_bits[0] : 0;
    for (u32 k = 0; k < s.nsteps; ++k) {
        const NttStep& st = s.step[k];
        const u64 row[8] = {st.pass, st.mode, st.S, p.logC[st.pass], st.grid_x, st.src, st.dst, st.count};
        memcpy(steps + 8 * k, row, sizeof(row));
    }
    return (int)s.nsteps;
}

extern "C" int emu_plan(u32 log_n, u64 root, u32* npass, u32* bits, u32* logc, u32* uinv) {
    NttPlan p;
    if (!ntt_make_plan(log_n, root, p)) return 1;
    *npass = p.npass; *uinv = p.uinv;
    for (int i = 0; i < 4; ++i) { bits[i] = p.pass_bits[i]; logc[i] = p.logC[i]; }
    return 0;
}

// what ntt_launch decides for a zero-padded transform (no arithmetic): 0 the plain plan, 1 an expansion plan; main_bits / extras as planned
extern "C" int emu_expand_plan(u32 log_n, u64 n_in, u64 root, u32* main_bits, u32* extras) {
    NttPlan p, xp;
    if (!ntt_make_plan(log_n, root, p) || p.npass == 0) return 0;
    if (!ntt_make_expand_plan(log_n, n_in, root, p, xp)) return 0;
    *main_bits = xp.main_bits; *extras = xp.extras;
    return 1;
}

// the twiddle schedule of three-pass plans: -1 environment, 0 load-time, 1 balanced; returns what a plan for log_n then uses
extern "C" int emu_set_schedule(int mode, u32 log_n, u64 root) {
    ntt_schedule_override() = mode;
    NttPlan p;
    if (!ntt_make_plan(log_n, root, p)) return -1;
    return (int)p.sched;
}
