// solve_plan.h -- which factorisation osh_lba_upload gives the reduced camera systems of a batch: the LDS-resident blocked LDL^T of
// ldlt_block.h (k_solve<NB, threads>, one block per window) with the widest panel NB in {24, 12, 6} whose scratch fits the LDS budget,
// or, when not even NB = 6 fits, the global-memory factorisation of big_solve.h.  With ldlt_lds_doubles as it stands (one LDS panel)
// the panels are: NB = 24 up to 115 optimisable poses, 12 up to 234, 6 up to 438 (437 with 512 threads), big_solve.h from 439.
// Plain host arithmetic (no HIP call): osh_lba_solve_plan_check (solve_plan_check.cpp) returns it to the CPU tests.
#pragma once
#include "ldlt_block.h"

namespace osh {

constexpr int kSolveThreadsBatch = 256, kSolveThreadsLatency = 512;
constexpr size_t kSolveLdsBudget = (size_t)150 * 1024;   // bytes of dynamic LDS a k_solve block may ask for
constexpr int kSolveBatchWindows = 128;                  // from this many windows on a batch takes the 256-thread blocks

struct SolvePlan {
  int nb, threads;
  bool big;            // big_solve.h (then nb = 6, the panel of the unused k_solve, and lds_bytes = 0)
  size_t lds_bytes;    // dynamic LDS of k_solve<nb, threads>
};

// n_max: unknowns of the largest window (6 per optimisable pose).  The overrides are the values of OSH_LBA_SOLVE_NB,
// OSH_LBA_SOLVE_THREADS and OSH_LBA_SOLVE_BIG (0: not set; a value that is not one of the instantiations is ignored).
// OSH_LBA_SOLVE_NB can only narrow the panel: a wider one than the rule's would not fit.
__host__ inline SolvePlan lba_solve_plan(int n_max, int n_windows, int force_nb, int force_threads, int force_big) {
  SolvePlan p;
  p.threads = n_windows >= kSolveBatchWindows ? kSolveThreadsBatch : kSolveThreadsLatency;
  const int W = ldlt_row_stride(n_max);
  auto need = [&](int b) { return ldlt_lds_doubles(b, W, p.threads) * sizeof(double); };
  int nb = 24;
  while (nb > 6 && need(nb) > kSolveLdsBudget) nb /= 2;  // 24 -> 12 -> 6 (template instantiations of k_solve)
  if (force_threads == kSolveThreadsBatch || force_threads == kSolveThreadsLatency) p.threads = force_threads;
  if ((force_nb == 24 || force_nb == 12 || force_nb == 6) && force_nb <= nb) nb = force_nb;
  p.big = force_big != 0 || need(nb) > kSolveLdsBudget;
  if (p.big) nb = 6;
  p.nb = nb;
  p.lds_bytes = p.big ? 0 : need(nb);
  return p;
}

}  // namespace osh
