// sim3_ops.cc -- osh_host_sim3_apply (include/orbslam3_hip_host.h): the device's Sim3 header csrc/pgo_sim3.h compiled for the
// host, applied over arrays, so that its branches and operation order can be checked on a machine with no GPU.
#include <cstdint>

#include "../pgo_sim3.h"
#include "orbslam3_hip.h"
#include "orbslam3_hip_host.h"

using namespace osh::pgo;

extern "C" int osh_host_sim3_apply(int32_t op, int32_t n, const double* a, const double* b, const double* c, const uint8_t* flag,
                                   double* out) {
  if (n < 0 || !a || !out) return -1;
  const bool needs_b = op == OSH_SIM3_MUL || op == OSH_SIM3_MAP || op == OSH_SIM3_EDGE_ERROR || op == OSH_SIM3_OPLUS || op == OSH_SIM3_SOLVE3;
  if ((needs_b && !b) || (op == OSH_SIM3_EDGE_ERROR && !c) || (op == OSH_SIM3_OPLUS && !flag)) return -1;
  for (int32_t k = 0; k < n; ++k) {
    switch (op) {
      case OSH_SIM3_EXP: sim3_store(sim3_exp(a + 7 * (size_t)k), out + 8 * (size_t)k); break;
      case OSH_SIM3_LOG: sim3_log(sim3_load(a + 8 * (size_t)k), out + 7 * (size_t)k); break;
      case OSH_SIM3_MUL: sim3_store(sim3_mul(sim3_load(a + 8 * (size_t)k), sim3_load(b + 8 * (size_t)k)), out + 8 * (size_t)k); break;
      case OSH_SIM3_INVERSE: sim3_store(sim3_inverse(sim3_load(a + 8 * (size_t)k)), out + 8 * (size_t)k); break;
      case OSH_SIM3_MAP: sim3_map(sim3_load(a + 8 * (size_t)k), b + 3 * (size_t)k, out + 3 * (size_t)k); break;
      case OSH_SIM3_EDGE_ERROR:
        edge_error(sim3_load(a + 8 * (size_t)k), sim3_load(b + 8 * (size_t)k), sim3_load(c + 8 * (size_t)k), out + 7 * (size_t)k);
        break;
      case OSH_SIM3_OPLUS: sim3_store(vertex_oplus(sim3_load(a + 8 * (size_t)k), b + 7 * (size_t)k, flag[k] != 0), out + 8 * (size_t)k); break;
      case OSH_SIM3_QUAT_TO_R: quat_to_R(a + 4 * (size_t)k, out + 9 * (size_t)k); break;
      case OSH_SIM3_R_TO_QUAT: R_to_quat(a + 9 * (size_t)k, out + 4 * (size_t)k); break;
      case OSH_SIM3_SOLVE3: solve3_lu(a + 9 * (size_t)k, b + 3 * (size_t)k, out + 3 * (size_t)k); break;
      default: return -1;
    }
  }
  return 0;
}
