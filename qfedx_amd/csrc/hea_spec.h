// Per-plan build of the MFMA pass kernels (hea_spec.cpp): what the bindings pass in and call.
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "hea_args.h"

namespace qfx {

// One pass program and the constants its kernel is compiled with.
struct HeaSpecDesc {
  bool adjoint = false, bf16 = false, stamps = false;
  int gate_lo = -1;                 // -1: the source's default (QFX_HEA_GATE_LO)
  int n = 0, t = 0, c = 0, lo = 0, hi = 0, ncls = 0;
  int gen = 0, load_lam = 0, store_lam = 0, n_regions = 0;
  int hrow[5] = {0, 0, 0, 0, 0};
  bool obs_load = false;            // requested: the tile load seeds lambda in place of a leading OP_OBS record
  int lean = 0;                     // requested HEA_LEAN_* parts (hea_spec_lean: what this pass compiles)
  std::vector<int> ops;             // [nops][128] op records
  std::vector<int> fidx;            // [nops][2] fragment indices
};

// obs_load as compiled: only an adjoint pass that loads no lambda and whose first op is OP_OBS has a seeding load
bool hea_spec_obs_load(const HeaSpecDesc& d);

// Work the per-plan kernels leave out (QFX_HEA_SPEC_LEAN, a bit mask; every part is bitwise neutral):
//   IM     adjoint pair ops multiply by the im-row fragments frag_regs formed once per op, not re-derived per block
//   NOBAR  no op barrier between two cross-only gradient ops (neither writes the tile nor reads fragments)
//   STORE  the pass's tile store is issued at the barrier behind the last op that writes the tile, ahead of a
//          read-only tail (forward: the readout; adjoint with store_lam: trailing cross-only gradient ops)
enum { HEA_LEAN_IM = 1, HEA_LEAN_NOBAR = 2, HEA_LEAN_STORE = 4 };
// What of d.lean takes effect in this pass: its mask (0: the text of before the knob), per op whether it starts
// without an op barrier, and the op at whose opening barrier the tile store is issued (-1: after the op loop).
struct HeaSpecLean {
  int mask = 0;
  std::vector<int> nobar;
  int early = -1;
};
HeaSpecLean hea_spec_lean(const HeaSpecDesc& d);
std::string hea_spec_prelude(const HeaSpecDesc& d);
std::string hea_spec_source(const HeaSpecDesc& d);
std::string hea_spec_key(const HeaSpecDesc& d, const std::string& include_dir, const std::string& arch);
int hea_spec_prepare(const HeaSpecDesc& d, const std::string& cache_dir, const std::string& include_dir,
                     const std::string& arch, std::string* key_out);
int hea_spec_load(int handle);
int hea_spec_launch(int handle, int adjoint, bool bf16, const HeaPassArgs* args, int n_samples, hipStream_t st);
const std::vector<char>* hea_spec_code(int handle);

}  // namespace qfx
