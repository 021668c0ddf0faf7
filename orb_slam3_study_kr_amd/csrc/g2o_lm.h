// g2o_lm.h -- the Levenberg-Marquardt controller of g2o's OptimizationAlgorithmLevenberg, stated once for every solver of
// this library, host and device: the one-block kernels k_pose_opt and k_sim3_opt, the block group of k_liba, the state machine
// of k_control (local / global BA) and the host loop PgoRun::solve of the two pose graphs.
//
//   lm_judge_trial        optimization_algorithm_levenberg.cpp:129-147  gain ratio, accept / reject, the lambda and ni update
//   lm_iteration_goes_on  :151-155 (qmax == maxTrials || rho == 0 -> Terminate) and :157-168, the three-bad-iterations stop
//                         this copy of g2o adds
//   kLmTau                :47 / :171-185  _tau of computeLambdaInit (lambda = tau * max |H_dd|; each site finds its own maximum)
//   kLmMaxTrials          :51  _maxTrialsAfterFailure
//
// What differs between the sites stays there: which buffer becomes current after an accepted trial, the traces and counters,
// where tempChi and the computeScale sum come from, and the trial loop `do ... while (rho < 0 && qmax < kLmMaxTrials)` itself.
//
// The functions keep no state and set no `fp contract` pragma; they take whatever the including file has in force.  None of
// their expressions can be contracted into an FMA with a different result: 2 * rho is exact, and no other product feeds an
// addition.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

namespace osh {

constexpr double kLmTau = 1e-5;   // OptimizationAlgorithmLevenberg::_tau
constexpr int kLmMaxTrials = 10;  // _maxTrialsAfterFailure

struct LmTrial { bool accepted; double rho; };

// One trial's verdict.  tempChi is the trial's activeRobustChi2, already replaced by DBL_MAX when the linear solve failed;
// scale_sum is computeScale's sum x^T (lambda x + b) (the 1e-3 is added here).  Accepted: lambda shrinks by
// max(1/3, min(1 - (2 rho - 1)^3, 2/3)), ni = 2, and the caller makes the trial estimate current (discardTop).
// Rejected: lambda *= ni, ni *= 2, the trial estimate is dropped (pop).
__host__ __device__ __forceinline__ LmTrial lm_judge_trial(double& lambda, double& ni, double currentChi, double tempChi, double scale_sum) {
  double rho = currentChi - tempChi;
  double scale = scale_sum;
  scale += 1e-3;
  rho /= scale;
  const bool accepted = rho > 0 && std::isfinite(tempChi);
  if (accepted) {
    double alpha = 1. - std::pow((2 * rho - 1), 3);
    alpha = fmin(alpha, 2. / 3.);
    lambda *= fmax(1. / 3., alpha);
    ni = 2;
  } else {
    lambda *= ni;
    ni *= 2;
  }
  return {accepted, rho};
}

// After the trials of an iteration (qmax of them, the last gain ratio rho): does optimize() run another iteration?
// The Terminate exit leaves nBad untouched.
__host__ __device__ __forceinline__ bool lm_iteration_goes_on(int& nBad, double iniChi, double currentChi, int qmax, double rho) {
  if (qmax == kLmMaxTrials || rho == 0) return false;
  if ((iniChi - currentChi) * 1e3 < iniChi) nBad++; else nBad = 0;
  return nBad < 3;
}

}  // namespace osh
