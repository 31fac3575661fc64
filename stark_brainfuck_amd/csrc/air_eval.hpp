// air_eval.hpp -- the shapes of the five tables' constraint sets and the dispatch to their generated constraint code
// (air_generated.hpp), shared by the quotient / combination kernels (air.hip) and the trace checker (air_check.hip).
#pragma once
#include "air_generated.hpp"

namespace bfs {

template <int TABLE> struct AirShape;
template <> struct AirShape<0> { static constexpr int BW = airgen::PROCESSOR_BASE_WIDTH, XW = airgen::PROCESSOR_EXT_WIDTH, NB = airgen::PROCESSOR_NUM_BOUNDARY, NT = airgen::PROCESSOR_NUM_TRANSITION, NZ = airgen::PROCESSOR_NUM_TERMINAL; };
template <> struct AirShape<1> { static constexpr int BW = airgen::INSTRUCTION_BASE_WIDTH, XW = airgen::INSTRUCTION_EXT_WIDTH, NB = airgen::INSTRUCTION_NUM_BOUNDARY, NT = airgen::INSTRUCTION_NUM_TRANSITION, NZ = airgen::INSTRUCTION_NUM_TERMINAL; };
template <> struct AirShape<2> { static constexpr int BW = airgen::MEMORY_BASE_WIDTH, XW = airgen::MEMORY_EXT_WIDTH, NB = airgen::MEMORY_NUM_BOUNDARY, NT = airgen::MEMORY_NUM_TRANSITION, NZ = airgen::MEMORY_NUM_TERMINAL; };
template <> struct AirShape<3> { static constexpr int BW = airgen::INPUT_BASE_WIDTH, XW = airgen::INPUT_EXT_WIDTH, NB = airgen::INPUT_NUM_BOUNDARY, NT = airgen::INPUT_NUM_TRANSITION, NZ = airgen::INPUT_NUM_TERMINAL; };
template <> struct AirShape<4> { static constexpr int BW = airgen::OUTPUT_BASE_WIDTH, XW = airgen::OUTPUT_EXT_WIDTH, NB = airgen::OUTPUT_NUM_BOUNDARY, NT = airgen::OUTPUT_NUM_TRANSITION, NZ = airgen::OUTPUT_NUM_TERMINAL; };

// the extended AIR of table TABLE at one point; `a` carries the challenges, terminals and parameters (members ch, tm, pr)
template <int TABLE, class Sink, class BN, class XN, class Args>
__device__ __forceinline__ void air_eval(const u64* bc, BN bn, const Xfe* xc, XN xn, const Args& a, Sink& sink) {
    if constexpr (TABLE == 0) airgen::air_processor(bc, bn, xc, xn, a.ch, a.tm, a.pr, sink);
    else if constexpr (TABLE == 1) airgen::air_instruction(bc, bn, xc, xn, a.ch, a.tm, a.pr, sink);
    else if constexpr (TABLE == 2) airgen::air_memory(bc, bn, xc, xn, a.ch, a.tm, a.pr, sink);
    else if constexpr (TABLE == 3) airgen::air_input(bc, bn, xc, xn, a.ch, a.tm, a.pr, sink);
    else airgen::air_output(bc, bn, xc, xn, a.ch, a.tm, a.pr, sink);
}

}  // namespace bfs
