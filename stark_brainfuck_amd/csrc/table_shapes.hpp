// table_shapes.hpp -- the column counts of the five tables for host code that walks them by index (prover.cpp, verifier.cpp), taken
// from the constants tools/gen_air.py writes into air_generated.hpp: stark_brainfuck_amd/air.py is the one statement of the AIR.
#pragma once
#include "air_generated.hpp"

namespace bfs {

constexpr int NT = 5;                                       // processor, instruction, memory, input, output (brainfuck_stark.py:56-60)
constexpr u32 BASE_W[NT] = {airgen::PROCESSOR_BASE_WIDTH, airgen::INSTRUCTION_BASE_WIDTH, airgen::MEMORY_BASE_WIDTH, airgen::INPUT_BASE_WIDTH,
                            airgen::OUTPUT_BASE_WIDTH};
constexpr u32 EXT_W[NT] = {airgen::PROCESSOR_EXT_WIDTH, airgen::INSTRUCTION_EXT_WIDTH, airgen::MEMORY_EXT_WIDTH, airgen::INPUT_EXT_WIDTH,
                           airgen::OUTPUT_EXT_WIDTH};     // extension columns only (full width - base width); three limb planes each

}  // namespace bfs
