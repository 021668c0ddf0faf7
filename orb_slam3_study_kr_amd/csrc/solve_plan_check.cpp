// solve_plan_check.cpp -- host-only view of the rule that gives a batch's reduced camera systems their factorisation
// (solve_plan.h): the plan osh_lba_upload would take for a largest window of n_max unknowns in a batch of n_windows, with the
// values of the three switches passed in place of the environment.  Needs no GPU and makes no HIP call.
#include "common.h"
#include "solve_plan.h"

using namespace osh;

extern "C" int osh_lba_solve_plan_check(int32_t n_max, int32_t n_windows, int32_t force_nb, int32_t force_threads, int32_t force_big,
                                        int32_t out[4]) {
  if (n_max < 0 || n_windows <= 0 || !out) { set_error("osh_lba_solve_plan_check: bad arguments"); return OSH_ERR_INVALID; }
  const SolvePlan p = lba_solve_plan(n_max, n_windows, force_nb, force_threads, force_big);
  out[0] = p.big ? 1 : 0; out[1] = p.nb; out[2] = p.threads; out[3] = (int32_t)p.lds_bytes;
  return OSH_OK;
}
