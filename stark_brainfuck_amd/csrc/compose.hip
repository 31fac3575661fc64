// compose.hip -- the composition polynomial of a proof by out-of-domain openings (include/bfstark_compose.h; BrainfuckStark.prove_deep):
//     H(x) = sum_t sum_q beta_{t,q} * quotient_{t,q}(x) + sum_j beta_j * (lhs_j - rhs_j)(x) / (x - 1)
// straight from the trace codewords, on every 2^log_step-th point x_i = offset * omega^i of the FRI domain.  The reference has no such
// sum (its prover combines columns AND quotients, each with a degree-shifted copy, brainfuck_stark.py:236-300); the quotients are its
// table.py:148-281 and permutation_argument.py:9-18, evaluated by the generated constraint code (air_generated.hpp) as in air.hip.
// Codewords are column-major: base column c at base[c * n + i], extension column c as three limb planes at ext[(3 c + limb) * n + i].
#include <cstddef>

#include "../../include/bfstark_compose.h"
#include "air_eval.hpp"
#include "lazy.hpp"
#include "runtime.hpp"

namespace bfs {

template <int TABLE>
struct ComposeLayout {
    typedef AirShape<TABLE> S;
    static constexpr int NQ = S::NB + S::NT + S::NZ;
    static constexpr bool q_ext(int q) {
        if constexpr (TABLE == 0) return airgen::PROCESSOR_Q_EXT[q];
        else if constexpr (TABLE == 1) return airgen::INSTRUCTION_Q_EXT[q];
        else if constexpr (TABLE == 2) return airgen::MEMORY_Q_EXT[q];
        else if constexpr (TABLE == 3) return airgen::INPUT_Q_EXT[q];
        else return airgen::OUTPUT_Q_EXT[q];
    }
    static constexpr int kind(int q) { return q < S::NB ? 0 : (q < S::NB + S::NT ? 1 : 2); }      // boundary, transition, terminal
    static constexpr int words(int q) { return q_ext(q) ? LAZY_W_EXT : LAZY_W_BASE; }
    static constexpr int offset(int q) {
        int o = 0;
        for (int j = 0; j < q; ++j) o += words(j);
        return o;
    }
    static constexpr int NW = offset(NQ);
};

// the weights as the lanes read them: per quotient 3 words (its value is a base element) or the 7 of lazy.hpp's weight matrix
template <int TABLE>
struct ComposeTerms {
    u64 w[ComposeLayout<TABLE>::NW];
};

template <int TABLE>
struct ComposeArgs {
    const u64* base;
    const u64* ext;
    u64* acc;            // three limb planes of `count`
    u64 n, count;        // count = n >> log_step: thread k works on point k << log_step
    u32 log_step, log_height, lo_bits, accumulate;
    u64 unit_distance;
    u64 height;          // 0: the transition zerofier has no inverse and the factor is 0 (table.py:181-184)
    u64 omicron_inv, offset;
    const u64* w_lo;
    const u64* w_hi;
    Xfe ch[11];
    Xfe tm[5];
    Xfe pr[1];
    ComposeTerms<TABLE> terms;
};

// The constraints arrive kind by kind; all quotients of a kind share their zerofier inverse, so the weighted VALUES of a kind are
// summed unreduced (lazy.hpp) and the inverse is applied once per kind -- three scalings per point whatever the table.
template <int TABLE>
struct ComposeSink {
    typedef ComposeLayout<TABLE> Lay;
    const u64* w;                        // in LDS
    u64 boundary, transition, terminal;  // the zerofier inverses at this point
    Xfe acc;
    LazyX sum;

    template <int KIND> __device__ __forceinline__ void close_kind() {
        acc = xfe_add(acc, xfe_scale(lazyx_reduce(sum), KIND == 0 ? boundary : (KIND == 1 ? transition : terminal)));
        sum = lazyx_zero();
    }
    template <int Q> __device__ __forceinline__ void open() {
        if constexpr (Q > 0) {
            if constexpr (Lay::kind(Q) != Lay::kind(Q - 1)) close_kind<Lay::kind(Q - 1)>();
        }
    }
    __device__ __forceinline__ void finish() { close_kind<Lay::kind(Lay::NQ - 1)>(); }
    // the generated code's interface
    template <int Q> __device__ __forceinline__ void put(const Xfe& v) {
        static_assert(Lay::q_ext(Q), "layout and generated code disagree");
        open<Q>();
        lazyx_mac_ext(sum, w + Lay::offset(Q), v);
    }
    template <int Q> __device__ __forceinline__ void put_base(u64 v) {
        static_assert(!Lay::q_ext(Q), "layout and generated code disagree");
        open<Q>();
        lazyx_mac_base(sum, w + Lay::offset(Q), v);
    }
};

struct ComposeNextBase {
    const u64* p;
    __device__ __forceinline__ u64 operator[](int k) const { return p[k * 256]; }
};
struct ComposeNextExt {
    const u64* p;
    __device__ __forceinline__ Xfe operator[](int k) const { return Xfe{{p[(3 * k) * 256], p[(3 * k + 1) * 256], p[(3 * k + 2) * 256]}}; }
};

constexpr int compose_waves(int table) { return table < 2 ? 3 : 4; }      // air_combine_kernel's choice (air.hip: BFS_COMBINE_WAVES)
constexpr bool compose_lds_next(int table) { return table == 0; }         // and its BFS_COMBINE_LDS_NEXT

template <int TABLE>
__global__ void __launch_bounds__(256, compose_waves(TABLE)) air_compose_kernel(const ComposeArgs<TABLE> a) {
    typedef AirShape<TABLE> S;
    // relied on from air_combine_kernel: the weights are staged in LDS from the raw kernel-argument segment with a per-thread index (as
    // scalar kernel arguments the compiler fetches all of them up front and spills them to register lanes) ...
    __shared__ ComposeTerms<TABLE> T;
    {
        const u64* karg = (const u64*)__builtin_amdgcn_kernarg_segment_ptr();
        constexpr u32 first = offsetof(ComposeArgs<TABLE>, terms) / 8, words = sizeof(ComposeTerms<TABLE>) / 8;
        static_assert(offsetof(ComposeArgs<TABLE>, terms) % 8 == 0 && sizeof(ComposeTerms<TABLE>) % 8 == 0, "staged as 64-bit words");
        u64* dst = reinterpret_cast<u64*>(&T);
        for (u32 k = threadIdx.x; k < words; k += 256) dst[k] = karg[first + k];
    }
    __syncthreads();
    // ... and one point per thread, no grid-stride loop (a loop lets the compiler hoist the challenges into registers)
    const u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < a.count) {
        const u64 i = k << a.log_step;
        u64 j = i + a.unit_distance;
        if (j >= a.n) j -= a.n;
        constexpr bool LDS_NEXT = compose_lds_next(TABLE);      // the processor table's next row waits in LDS ([value][thread]): 19 values
        __shared__ u64 next_row[LDS_NEXT ? (S::BW + 3 * S::XW) * 256 : 1];
        u64 bc[S::BW], bn[LDS_NEXT ? 1 : S::BW];
        Xfe xc[S::XW], xn[LDS_NEXT ? 1 : S::XW];
#pragma unroll
        for (int c = 0; c < S::BW; ++c) {
            bc[c] = a.base[(u64)c * a.n + i];
            if constexpr (LDS_NEXT) next_row[c * 256 + threadIdx.x] = a.base[(u64)c * a.n + j];
            else bn[c] = a.base[(u64)c * a.n + j];
        }
#pragma unroll
        for (int c = 0; c < S::XW; ++c)
#pragma unroll
            for (int l = 0; l < 3; ++l) {
                xc[c].c[l] = a.ext[(u64)(3 * c + l) * a.n + i];
                if constexpr (LDS_NEXT) next_row[(S::BW + 3 * c + l) * 256 + threadIdx.x] = a.ext[(u64)(3 * c + l) * a.n + j];
                else xn[c].c[l] = a.ext[(u64)(3 * c + l) * a.n + j];
            }
        // zerofier inverses with ONE field inversion (Montgomery's trick over za = x - 1, xo = x - omicron^-1, zc = x^h - 1)
        const u64 x = gl_mul(a.offset, tw_pow(a.w_lo, a.w_hi, a.lo_bits, i));
        const u64 za = gl_sub(x, 1), xo = gl_sub(x, a.omicron_inv);
        u64 zc = 1;
        if (a.height != 0) {
            u64 xh = x;
            for (u32 s = 0; s < a.log_height; ++s) xh = gl_sqr(xh);
            zc = gl_sub(xh, 1);
        }
        const u64 ab = gl_mul(za, xo);
        const u64 iabc = gl_inv(gl_mul(ab, zc));
        const u64 iab = gl_mul(iabc, zc);
        Xfe acc = Xfe{{0, 0, 0}};
        if (a.accumulate) acc = Xfe{{a.acc[k], a.acc[a.count + k], a.acc[2 * a.count + k]}};
        ComposeSink<TABLE> sink{T.w, gl_mul(iab, xo), a.height != 0 ? gl_mul(xo, gl_mul(iabc, ab)) : 0, gl_mul(iab, za), acc, lazyx_zero()};
        if constexpr (LDS_NEXT) air_eval<TABLE>(bc, ComposeNextBase{next_row + threadIdx.x}, xc, ComposeNextExt{next_row + S::BW * 256 + threadIdx.x}, a, sink);
        else air_eval<TABLE>(bc, (const u64*)bn, xc, (const Xfe*)xn, a, sink);
        sink.finish();
        a.acc[k] = sink.acc.c[0];
        a.acc[a.count + k] = sink.acc.c[1];
        a.acc[2 * a.count + k] = sink.acc.c[2];
    }
}

// acc[k] (+)= weight * (lhs - rhs)(x_i) / (x_i - 1), i = k << log_step
__global__ void __launch_bounds__(256) difference_compose_kernel(const u64* lhs, const u64* rhs, u64* acc, u64 n, u64 count, u32 log_step, u32 accumulate,
                                                                 u64 offset, const u64* w_lo, const u64* w_hi, u32 lo_bits, Xfe weight) {
    const u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const u64 i = k << log_step;
    const u64 z = gl_inv(gl_sub(gl_mul(offset, tw_pow(w_lo, w_hi, lo_bits, i)), 1));
    Xfe q;
#pragma unroll
    for (int l = 0; l < 3; ++l) q.c[l] = gl_mul(gl_sub(lhs[(u64)l * n + i], rhs[(u64)l * n + i]), z);
    Xfe r = xfe_mul(weight, q);
    if (accumulate) r = xfe_add(r, Xfe{{acc[k], acc[count + k], acc[2 * count + k]}});
    acc[k] = r.c[0];
    acc[count + k] = r.c[1];
    acc[2 * count + k] = r.c[2];
}

static Xfe canonical_xfe(const u64* p) { return Xfe{{p[0] % GL_P, p[1] % GL_P, p[2] % GL_P}}; }

template <int TABLE>
static int air_compose_launch(ComposeArgs<TABLE>& a, const uint64_t* h_weights, hipStream_t stream) {
    typedef ComposeLayout<TABLE> Lay;
    for (int q = 0; q < Lay::NQ; ++q) {
        const Xfe w = canonical_xfe(h_weights + 3 * q);
        u64* out = a.terms.w + Lay::offset(q);
        if (Lay::q_ext(q)) lazy_weight_matrix(w, out);
        else for (int l = 0; l < 3; ++l) out[l] = w.c[l];
    }
    static_assert(sizeof(ComposeArgs<TABLE>) <= 4096, "kernel arguments");
    hipLaunchKernelGGL(air_compose_kernel<TABLE>, dim3((u32)((a.count + 255) / 256)), dim3(256), 0, stream, a);
    BFS_HIP(hipGetLastError());
    return BFS_OK;
}

template <int TABLE>
static int air_compose_table(const uint64_t* d_base, const uint64_t* d_ext, uint32_t log_n, uint64_t unit_distance, uint64_t height, uint64_t omicron_inv,
                             uint64_t offset, uint64_t omega, const uint64_t* h_challenges, const uint64_t* h_terminals, const uint64_t* h_params,
                             const uint64_t* h_weights, uint32_t log_step, int accumulate, uint64_t* d_acc, hipStream_t stream) {
    ComposeArgs<TABLE> a{};
    a.base = d_base; a.ext = d_ext; a.acc = d_acc;
    a.n = 1ull << log_n;
    a.count = a.n >> log_step;
    a.log_step = log_step;
    a.accumulate = accumulate ? 1u : 0u;
    a.unit_distance = unit_distance % a.n;
    a.height = height;
    while ((1ull << a.log_height) < height) ++a.log_height;
    a.omicron_inv = omicron_inv % GL_P; a.offset = offset % GL_P;
    BFS_TRY(ntt_power_tables(omega, log_n, &a.w_lo, &a.w_hi, &a.lo_bits));
    for (int i = 0; i < 11; ++i) a.ch[i] = canonical_xfe(h_challenges + 3 * i);
    for (int i = 0; i < 5; ++i) a.tm[i] = canonical_xfe(h_terminals + 3 * i);
    a.pr[0] = h_params ? canonical_xfe(h_params) : Xfe{{1, 0, 0}};
    return air_compose_launch<TABLE>(a, h_weights, stream);
}

static int check_compose(const char* who, uint32_t log_n, uint32_t log_step) {
    if (log_n > 32 || log_step > log_n) {
        set_error("%s: need log_step <= log_n <= 32 (got %u and %u)", who, log_step, log_n);
        return BFS_ERR_BAD_ARG;
    }
    return BFS_OK;
}

}  // namespace bfs

using namespace bfs;

extern "C" {

int bfsc_air_compose(int table, const uint64_t* d_base, const uint64_t* d_ext, uint32_t log_n, uint64_t unit_distance, uint64_t height,
                     uint64_t omicron_inv, uint64_t offset, uint64_t omega, const uint64_t* h_challenges, const uint64_t* h_terminals,
                     const uint64_t* h_params, const uint64_t* h_weights, uint32_t log_step, int accumulate, uint64_t* d_acc, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (table < 0 || table > 4) { set_error("bfsc_air_compose: table index %d", table); return BFS_ERR_BAD_ARG; }
    BFS_TRY(check_compose("bfsc_air_compose", log_n, log_step));
    if (!d_base || !d_ext || !d_acc || !h_challenges || !h_terminals || !h_weights) { set_error("bfsc_air_compose: null pointer"); return BFS_ERR_BAD_ARG; }
    if (height & (height - 1)) { set_error("bfsc_air_compose: table height must be zero or a power of two"); return BFS_ERR_NOT_POW2; }
#define BFSC_TABLE(T) air_compose_table<T>(d_base, d_ext, log_n, unit_distance, height, omicron_inv, offset, omega, h_challenges, h_terminals, h_params, \
                                           h_weights, log_step, accumulate, d_acc, stream)
    switch (table) {
        case 0: return BFSC_TABLE(0);
        case 1: return BFSC_TABLE(1);
        case 2: return BFSC_TABLE(2);
        case 3: return BFSC_TABLE(3);
        default: return BFSC_TABLE(4);
    }
#undef BFSC_TABLE
}

int bfsc_difference_compose(const uint64_t* d_lhs, const uint64_t* d_rhs, uint32_t log_n, uint64_t offset, uint64_t omega,
                            const uint64_t* h_weight, uint32_t log_step, int accumulate, uint64_t* d_acc, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    BFS_TRY(check_compose("bfsc_difference_compose", log_n, log_step));
    if (!d_lhs || !d_rhs || !d_acc || !h_weight) { set_error("bfsc_difference_compose: null pointer"); return BFS_ERR_BAD_ARG; }
    const u64 n = 1ull << log_n;
    const u64 *lo, *hi;
    u32 lo_bits;
    BFS_TRY(ntt_power_tables(omega, log_n, &lo, &hi, &lo_bits));
    const u64 count = n >> log_step;
    hipLaunchKernelGGL(difference_compose_kernel, dim3((u32)((count + 255) / 256)), dim3(256), 0, stream, d_lhs, d_rhs, d_acc, n, count, log_step,
                       accumulate ? 1u : 0u, offset % GL_P, lo, hi, lo_bits, canonical_xfe(h_weight));
    BFS_HIP(hipGetLastError());
    return BFS_OK;
}

}  // extern "C"
