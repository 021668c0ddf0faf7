// pgo4_ops.cc -- osh_host_pgo4_apply (include/orbslam3_hip_host.h): the device's 4-DoF header csrc/pgo4_se3.h compiled for the
// host, applied over arrays, so that its branches and operation order can be checked on a machine with no GPU.
#include <cstdint>

#include "../pgo4_se3.h"
#include "orbslam3_hip.h"
#include "orbslam3_hip_host.h"

using namespace osh::pgo4;

extern "C" int osh_host_pgo4_apply(int32_t op, int32_t n, const double* a, const double* b, const double* c, double* out) {
  if (n < 0 || !a || !out) return -1;
  if ((op == OSH_PGO4_UPDATE || op == OSH_PGO4_EDGE_ERROR) && (!b || !c)) return -1;
  for (int32_t k = 0; k < n; ++k) {
    switch (op) {
      case OSH_PGO4_EXP: exp_so3(a[3 * k], a[3 * k + 1], a[3 * k + 2], out + 9 * (size_t)k); break;
      case OSH_PGO4_LOG: log_so3(a + 9 * (size_t)k, out + 3 * (size_t)k); break;
      case OSH_PGO4_NORMALIZE:
        for (int i = 0; i < 9; ++i) out[9 * (size_t)k + i] = a[9 * (size_t)k + i];
        normalize_rotation(out + 9 * (size_t)k);
        break;
      case OSH_PGO4_UPDATE: {
        State s = state_load(a + kStateDoubles * (size_t)k);
        update_w(s, const_load(b + kConstDoubles * (size_t)k), c + 4 * (size_t)k);
        state_store(s, out + kStateDoubles * (size_t)k);
        break;
      }
      case OSH_PGO4_EDGE_ERROR: {
        const double* m = a + 12 * (size_t)k;
        const State si = state_load(b + kStateDoubles * (size_t)k), sj = state_load(c + kStateDoubles * (size_t)k);
        edge_error(m, m + 9, si.Rcw, si.tcw, sj.Rcw, sj.tcw, out + 6 * (size_t)k);
        break;
      }
      default: return -1;
    }
  }
  return 0;
}

extern "C" void osh_host_pgo4_sizes(int64_t* out) {
  out[0] = (int64_t)sizeof(osh_pgo4_problem);
  out[1] = (int64_t)sizeof(osh_pgo4_result);
}
