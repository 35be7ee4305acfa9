// pmx_jit.hpp — user ODE models compiled at run time for gfx950 with hiprtc.
// What is compiled - JitSpec and the generated text - is pmx_jit_source.hpp's.
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "pmx_jit_source.hpp"

namespace pmx {

// Compile for gfx950 (needs no device).  Returns true and fills *code (an AMDGPU code object); on failure *log has
// the compiler's diagnostics.
bool jit_compile(const JitSpec& spec, std::vector<char>* code, std::string* log);

struct JitModule {
  hipModule_t module = nullptr;
  hipFunction_t fn[2][2][2][SOLV_AUTO + 1] = {};  // [mode: 0 GRID, 1 PAIR][LAG][LL][SOLV_*]
};
// Load a compiled code object on the CURRENT device and resolve the entry points the translation unit of `spec` holds.
hipError_t jit_load(const std::vector<char>& code, JitModule* out, const JitSpec& spec);
void jit_unload(JitModule* m);

}  // namespace pmx
