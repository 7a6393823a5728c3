// check_store_kind.cpp — the importance launch's variant rule, printed on the host (no GPU, nothing is compiled for the device):
// one line per (passes, bytes written, outputs, forced kind of store) with what ImportanceVariant::of_launch answers, then
// every variant a launch can take with its slot.  tests/test_store_kind_cpu.py reads the lines.
//   hipcc -x hip --offload-host-only -std=c++17 -Iinclude -Igenjax-chi_amd/csrc -o check_store_kind tools/check_store_kind.cpp
// (the headers the library itself includes, in its order; gjx_plan_jit.hpp embeds gjx_device_embed.inc, which the build writes
// next to it.)
#include "gjx.h"
#include "gjx_guided.h"
#include "gjx_backsim.h"
#include "gjx_backmove.h"
#include "gjx_smc_params.h"
#include "gjx_csmc.h"
#include "gjx_temper.h"
#include "gjx_plate.h"
#include "gjx_pointwise.h"
#include "gjx_predictive.h"
#include "gjx_temper_cov.h"
#include "gjx_counts.h"
#include "gjx_group.h"
#include "gjx_group_checks.h"
#include "gjx_device.hpp"

#include <hip/hip_runtime.h>

#include "gjx_plan_jit.hpp"

#include <cstdint>
#include <cstdio>

int main() {
  using V = gjx_jit::ImportanceVariant;
  const uint64_t kBytes[] = {12288, 48000000ull, 1536000000ull};  // 3 x 1024 particles; one flagship pass; a 32-pass flagship batch
  for (int n_pass : {1, 2, 32})
    for (uint64_t bytes : kBytes)
      for (int outputs = 0; outputs < 3; ++outputs)  // 0 some outputs, 1 every output, 2 fused tail
        for (int pref = -1; pref < 4; ++pref) {
          const V v = V::of_launch(1, 4, 4, outputs == 2, n_pass, bytes, outputs == 1, pref);
          printf("launch passes %d bytes %llu outputs %d pref %d -> particles %d fused %d stores %d full %d slot %d launched %d\n", n_pass,
                 (unsigned long long)bytes, outputs, pref, v.lane_particles, (int)v.fused_tail, v.stores, (int)v.full_outputs, v.slot(), (int)v.launched());
        }
  // below four particles per lane there is one kind of store, whatever is asked
  for (int allowed : {1, 2})
    for (int pref = -1; pref < 4; ++pref) {
      const V v = V::of_launch(1, allowed, 4, false, 32, kBytes[2], true, pref);
      printf("narrow allowed %d pref %d -> particles %d stores %d full %d slot %d\n", allowed, pref, v.lane_particles, v.stores, (int)v.full_outputs, v.slot());
    }
  for (int impl = 0; impl < 2; ++impl)
    for (int P : {1, 2, 4})
      for (int fused = 0; fused < 2; ++fused)
        for (int stores = 0; stores < 4; ++stores)
          for (int full = 0; full < 2; ++full) {
            const V v{impl, P, fused != 0, stores, full != 0};
            if (v.launched()) printf("variant impl %d particles %d fused %d stores %d full %d slot %d of %d\n", impl, P, fused, stores, full, v.slot(), V::kSlots);
          }
  return 0;
}
