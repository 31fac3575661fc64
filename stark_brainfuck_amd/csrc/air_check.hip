// air_check.hip -- the AIR checked on the rows of an execution trace (the reference's Table.test / Table.xtest,
// /root/reference/code/table.py:48-110), reduced to "which constraint fails, on which row first, on how many rows".
//
// Unlike the quotient kernels, which evaluate the constraints on the FRI coset, this kernel evaluates them on the trace rows
// themselves: boundary constraints on row 0, transition constraints on the pairs (r, r + 1) for r < rows - 1 (NO cyclic wrap:
// Table.test stops at the last pair), terminal constraints on row rows - 1.  Base mode runs the base AIR
// (air_base_generated.hpp, TableAir.base()), extended mode the full AIR (air_generated.hpp, through air_eval).
// Base column c of the trace is at base[c * ld + r], limb l of extension column k at ext[(3 k + l) * ld + r].
#include <cstddef>

#include "../../include/bfstark.h"
#include "air_base_generated.hpp"
#include "air_eval.hpp"
#include "runtime.hpp"

namespace bfs {

struct AirCheckArgs {
    const u64* base;
    const u64* ext;
    u64* out;            // [first_row of constraint 0..NQ-1][count of constraint 0..NQ-1]
    u64 rows, ld;
    Xfe ch[11];
    Xfe tm[5];
    Xfe pr[1];
};

// the constraint counts of the base AIR
template <int TABLE> struct BaseShape;
template <> struct BaseShape<0> { static constexpr int NB = airgen::PROCESSOR_BASE_NUM_BOUNDARY, NT = airgen::PROCESSOR_BASE_NUM_TRANSITION; };
template <> struct BaseShape<1> { static constexpr int NB = airgen::INSTRUCTION_BASE_NUM_BOUNDARY, NT = airgen::INSTRUCTION_BASE_NUM_TRANSITION; };
template <> struct BaseShape<2> { static constexpr int NB = airgen::MEMORY_BASE_NUM_BOUNDARY, NT = airgen::MEMORY_BASE_NUM_TRANSITION; };
template <> struct BaseShape<3> { static constexpr int NB = airgen::INPUT_BASE_NUM_BOUNDARY, NT = airgen::INPUT_BASE_NUM_TRANSITION; };
template <> struct BaseShape<4> { static constexpr int NB = airgen::OUTPUT_BASE_NUM_BOUNDARY, NT = airgen::OUTPUT_BASE_NUM_TRANSITION; };

// boundary, transition, terminal counts of the set a launch checks
template <int TABLE, bool EXT> struct CheckShape {
    static constexpr int NB = EXT ? AirShape<TABLE>::NB : BaseShape<TABLE>::NB;
    static constexpr int NT = EXT ? AirShape<TABLE>::NT : BaseShape<TABLE>::NT;
    static constexpr int NQ = NB + NT + (EXT ? AirShape<TABLE>::NZ : 0);
};

template <int TABLE, class Sink>
__device__ __forceinline__ void air_base_eval(const u64* bc, const u64* bn, Sink& sink) {
    if constexpr (TABLE == 0) airgen::air_processor_base(bc, bn, sink);
    else if constexpr (TABLE == 1) airgen::air_instruction_base(bc, bn, sink);
    else if constexpr (TABLE == 2) airgen::air_memory_base(bc, bn, sink);
    else if constexpr (TABLE == 3) airgen::air_input_base(bc, bn, sink);
    else airgen::air_output_base(bc, bn, sink);
}

__device__ __forceinline__ bool gl_nonzero(u64 v) { return v != 0 && v != GL_P; }     // 0 in canonical form (P is the only other residue of 0)

// records, per constraint, whether its value at this row is non-zero AND the constraint applies to this row; the values of a kind that
// does not apply here (a transition constraint on the last row, which read no real next row) are dropped
template <int NB, int NT>
struct ViolationSink {
    u64 flags;
    bool first, has_next, last;
    template <int Q> __device__ __forceinline__ void mark(bool nonzero) {
        const bool applies = Q < NB ? first : (Q < NB + NT ? has_next : last);
        if (nonzero && applies) flags |= 1ull << Q;
    }
    template <int Q> __device__ __forceinline__ void put(const Xfe& v) { mark<Q>(gl_nonzero(v.c[0]) || gl_nonzero(v.c[1]) || gl_nonzero(v.c[2])); }
    template <int Q> __device__ __forceinline__ void put_base(u64 v) { mark<Q>(gl_nonzero(v)); }
};

template <int TABLE, bool EXT>
__global__ void __launch_bounds__(256) air_check_kernel(const AirCheckArgs a) {
    typedef CheckShape<TABLE, EXT> S;
    constexpr int BW = AirShape<TABLE>::BW, XW = AirShape<TABLE>::XW;
    static_assert(S::NQ <= 64, "one ballot bit and one lane per constraint");
    // one row per thread, no grid-stride loop (see air_quotient_kernel: the loop-invariant challenges would be hoisted into registers)
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    ViolationSink<S::NB, S::NT> sink{0, r == 0, r + 1 < a.rows, r + 1 == a.rows};
    if (r < a.rows) {
        const u64 rn = r + 1 < a.rows ? r + 1 : r;       // the last row has no next row: read an in-bounds one, the sink drops the values
        u64 bc[BW], bn[BW];
#pragma unroll
        for (int c = 0; c < BW; ++c) { bc[c] = gl_canon(a.base[(u64)c * a.ld + r]); bn[c] = gl_canon(a.base[(u64)c * a.ld + rn]); }
        if constexpr (EXT) {
            Xfe xc[XW], xn[XW];
#pragma unroll
            for (int c = 0; c < XW; ++c)
#pragma unroll
                for (int l = 0; l < 3; ++l) {
                    xc[c].c[l] = gl_canon(a.ext[(u64)(3 * c + l) * a.ld + r]);
                    xn[c].c[l] = gl_canon(a.ext[(u64)(3 * c + l) * a.ld + rn]);
                }
            air_eval<TABLE>(bc, (const u64*)bn, xc, (const Xfe*)xn, a, sink);
        } else {
            air_base_eval<TABLE>(bc, bn, sink);
        }
    }
    // per wave: one ballot per constraint (every lane takes part, rows past the end with no flags), lane q keeps constraint q's; then one
    // lane per failing constraint adds the popcount and lowers the first row with 64-bit atomics in global memory
    const u32 lane = threadIdx.x & 63;
    u64 mine = 0;
#pragma unroll
    for (int q = 0; q < S::NQ; ++q) {
        const u64 b = __ballot((sink.flags >> q) & 1);
        if (lane == (u32)q) mine = b;
    }
    if (mine) {
        const u64 wave_row = r - lane;
        atomicAdd((unsigned long long*)(a.out + S::NQ + lane), (unsigned long long)__popcll(mine));
        atomicMin((unsigned long long*)(a.out + lane), (unsigned long long)(wave_row + (u64)(__ffsll((long long)mine) - 1)));
    }
}

template <int TABLE, bool EXT>
static int air_check_launch(const AirCheckArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL((air_check_kernel<TABLE, EXT>), dim3((u32)((a.rows + 255) / 256)), dim3(256), 0, stream, a);
    BFS_HIP(hipGetLastError());
    return BFS_OK;
}

template <bool EXT>
static int air_check_dispatch(int table, const AirCheckArgs& a, hipStream_t stream) {
    switch (table) {
        case 0: return air_check_launch<0, EXT>(a, stream);
        case 1: return air_check_launch<1, EXT>(a, stream);
        case 2: return air_check_launch<2, EXT>(a, stream);
        case 3: return air_check_launch<3, EXT>(a, stream);
        default: return air_check_launch<4, EXT>(a, stream);
    }
}

static int check_counts(int table, int extended) {
    switch (table) {
        case 0: return extended ? CheckShape<0, true>::NQ : CheckShape<0, false>::NQ;
        case 1: return extended ? CheckShape<1, true>::NQ : CheckShape<1, false>::NQ;
        case 2: return extended ? CheckShape<2, true>::NQ : CheckShape<2, false>::NQ;
        case 3: return extended ? CheckShape<3, true>::NQ : CheckShape<3, false>::NQ;
        default: return extended ? CheckShape<4, true>::NQ : CheckShape<4, false>::NQ;
    }
}

static int table_ext_width(int table) {
    switch (table) {
        case 0: return AirShape<0>::XW;
        case 1: return AirShape<1>::XW;
        case 2: return AirShape<2>::XW;
        case 3: return AirShape<3>::XW;
        default: return AirShape<4>::XW;
    }
}

}  // namespace bfs

using namespace bfs;

extern "C" {

int bfs_air_base_counts(int table, int counts[2]) {
    switch (table) {
        case 0: counts[0] = BaseShape<0>::NB; counts[1] = BaseShape<0>::NT; return BFS_OK;
        case 1: counts[0] = BaseShape<1>::NB; counts[1] = BaseShape<1>::NT; return BFS_OK;
        case 2: counts[0] = BaseShape<2>::NB; counts[1] = BaseShape<2>::NT; return BFS_OK;
        case 3: counts[0] = BaseShape<3>::NB; counts[1] = BaseShape<3>::NT; return BFS_OK;
        case 4: counts[0] = BaseShape<4>::NB; counts[1] = BaseShape<4>::NT; return BFS_OK;
    }
    set_error("bfs_air_base_counts: table index %d", table);
    return BFS_ERR_BAD_ARG;
}

int bfs_air_check(int table, int extended, const uint64_t* d_base, const uint64_t* d_ext, uint64_t rows, uint64_t ld,
                  const uint64_t* h_challenges, const uint64_t* h_terminals, const uint64_t* h_params, bfs_air_violation* h_out, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (table < 0 || table > 4) { set_error("bfs_air_check: table index %d", table); return BFS_ERR_BAD_ARG; }
    if (extended != 0 && extended != 1) { set_error("bfs_air_check: extended must be 0 or 1"); return BFS_ERR_BAD_ARG; }
    const int nq = check_counts(table, extended);
    if (nq > 0 && !h_out) { set_error("bfs_air_check: h_out is NULL"); return BFS_ERR_BAD_ARG; }
    for (int q = 0; q < nq; ++q) { h_out[q].first_row = UINT64_MAX; h_out[q].count = 0; }
    if (rows == 0 || nq == 0) return BFS_OK;
    if (ld < rows) { set_error("bfs_air_check: ld %llu < rows %llu", (unsigned long long)ld, (unsigned long long)rows); return BFS_ERR_BAD_ARG; }
    if (rows > (1ull << 31)) { set_error("bfs_air_check: at most 2^31 rows"); return BFS_ERR_BAD_ARG; }
    if (!d_base) { set_error("bfs_air_check: d_base is NULL"); return BFS_ERR_BAD_ARG; }
    AirCheckArgs a{};
    a.base = d_base;
    a.ext = d_ext;
    a.rows = rows;
    a.ld = ld;
    a.pr[0] = Xfe{{1, 0, 0}};
    if (extended) {
        if (table_ext_width(table) > 0 && !d_ext) { set_error("bfs_air_check: d_ext is NULL"); return BFS_ERR_BAD_ARG; }
        if (!h_challenges || !h_terminals) { set_error("bfs_air_check: challenges and terminals are required in extended mode"); return BFS_ERR_BAD_ARG; }
        // every operand reduced on the way in, as bfs_air_evaluate does: the generated code assumes canonical residues
        auto canon = [](const uint64_t* l) { return Xfe{{l[0] % GL_P, l[1] % GL_P, l[2] % GL_P}}; };
        for (int i = 0; i < 11; ++i) a.ch[i] = canon(h_challenges + 3 * i);
        for (int i = 0; i < 5; ++i) a.tm[i] = canon(h_terminals + 3 * i);
        if (h_params) a.pr[0] = canon(h_params);
    }
    void* d_out = nullptr;
    BFS_TRY(device_alloc(2 * (size_t)nq * sizeof(u64), stream, &d_out));
    a.out = (u64*)d_out;
    u64 result[128];
    int rc = BFS_OK;
    if (hipMemsetAsync(a.out, 0xFF, (size_t)nq * sizeof(u64), stream) != hipSuccess ||
        hipMemsetAsync(a.out + nq, 0, (size_t)nq * sizeof(u64), stream) != hipSuccess) {
        set_error("bfs_air_check: hipMemsetAsync failed");
        rc = BFS_ERR_HIP;
    }
    if (rc == BFS_OK) rc = extended ? air_check_dispatch<true>(table, a, stream) : air_check_dispatch<false>(table, a, stream);
    if (rc == BFS_OK) {
        hipError_t e = hipMemcpyAsync(result, a.out, 2 * (size_t)nq * sizeof(u64), hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) { set_error("bfs_air_check: %s", hipGetErrorString(e)); rc = BFS_ERR_HIP; }
    }
    (void)device_release(d_out, stream);
    if (rc != BFS_OK) return rc;
    for (int q = 0; q < nq; ++q) { h_out[q].first_row = result[q]; h_out[q].count = result[nq + q]; }
    return BFS_OK;
}

}  // extern "C"
