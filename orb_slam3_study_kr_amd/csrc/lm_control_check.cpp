// lm_control_check.cpp -- host-only self check of the Levenberg-Marquardt controller (g2o_lm.h).  Needs no GPU.
// Plays optimize() the way every solver site does -- an iteration opens with iniChi = currentChi (the first one also sets
// ni = 2, nBad = 0), runs `do lm_judge_trial while (rho < 0 && qmax < kLmMaxTrials)` and closes with lm_iteration_goes_on --
// except that each trial's chi2, computeScale sum and solver verdict come from the caller's script instead of a linear solve.
#include "common.h"
#include "g2o_lm.h"
#include <cfloat>

using namespace osh;

extern "C" int osh_lm_control_check(double current_chi, double lambda, int32_t n_script, const double* script, int32_t* accepted,
                                    double* rho_out, double* lambda_out, double* ni_out, int32_t* iter_go_on, int32_t* iter_nbad,
                                    int32_t* iter_trials, int32_t* n_played) {
  if (n_script < 0 || (n_script > 0 && !script) || !accepted || !rho_out || !lambda_out || !ni_out || !iter_go_on || !iter_nbad || !iter_trials || !n_played) {
    set_error("osh_lm_control_check: bad arguments"); return OSH_ERR_INVALID;
  }
  double currentChi = current_chi, ni = 2.0;
  int nBad = 0, k = 0, iters = 0;
  bool ok = true;
  for (int it = 0; ok && k < n_script; ++it) {
    const double iniChi = currentChi;
    if (it == 0) { ni = 2.0; nBad = 0; }
    double rho = 0.0;
    int qmax = 0;
    do {
      double tempChi = script[3 * k];
      if (script[3 * k + 2] == 0.0) tempChi = DBL_MAX;   // the linear solve failed
      const LmTrial t = lm_judge_trial(lambda, ni, currentChi, tempChi, script[3 * k + 1]);
      rho = t.rho;
      if (t.accepted) currentChi = tempChi;
      accepted[k] = t.accepted ? 1 : 0; rho_out[k] = rho; lambda_out[k] = lambda; ni_out[k] = ni;
      ++qmax; ++k;
    } while (rho < 0 && qmax < kLmMaxTrials && k < n_script);
    if (rho < 0 && qmax < kLmMaxTrials) break;   // the script ended inside an iteration: that iteration is not reported
    ok = lm_iteration_goes_on(nBad, iniChi, currentChi, qmax, rho);
    iter_go_on[iters] = ok ? 1 : 0; iter_nbad[iters] = nBad; iter_trials[iters] = qmax;
    ++iters;
  }
  n_played[0] = k; n_played[1] = iters;
  return OSH_OK;
}
