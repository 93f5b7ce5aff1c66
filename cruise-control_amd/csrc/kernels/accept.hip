// gfx950 kernel for batched Goal.actionAcceptance (ccmi_actions_acceptance).
//
// K9  accept_actions : every (action, goal) verdict of a batch — what AnalyzerUtils.isProposalAcceptableForOptimizedGoals
//                      (AnalyzerUtils.java:169-179) asks of each optimized goal, for a whole candidate list at once and
//                      without the first-fit early exit of the scans: a JVM goal late in a mixed chain needs the verdict
//                      of every goal (BROKER_REJECT ends a broker's candidates, REPLICA_REJECT only the replica's).
// One lane takes one action; a workgroup is one wavefront. The host resolved each action to an AcceptRow (replica
// ids, destination broker), so the lane gathers its replica, partition and two broker records once, with independent
// loads, and keeps them in registers for every goal (about 0.45 KB per action instead of per cell). The goal loop is
// outermost and the goal comes from the kernel arguments, so the dispatch in predicates.h (uniform(g.kind)) branches on
// a scalar. The host puts moves and leadership moves in one segment and swaps in another, each padded to whole
// wavefronts with copies of one of its rows, so a wave runs goalAcceptMove or goalAcceptSwap, never both. A wave's
// verdicts go through LDS and leave as one contiguous run of 64 * nGoals bytes in dword stores.
// Built with -ffp-contract=off: every predicate is the reference's IEEE double expression.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../engine/accept_view.h"
#include "../engine/devtypes.h"
#include "../engine/predicates.h"

namespace ccmi {

namespace {

constexpr int kAcceptWave = 64;

}  // namespace

// rows[0, nRows): nRows is a multiple of 64 and the grid is nRows / 64 wavefronts; out[row * nGoals + g].
__global__ __launch_bounds__(kAcceptWave) void accept_actions(DevTables T, DevProgram prog,
                                                              const AcceptRow* __restrict__ rows,
                                                              int8_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) int8_t cells[kAcceptWave * kMaxGoals];
  const size_t wave = blockIdx.x;
  const int lane = threadIdx.x;
  const AcceptRow a = rows[wave * kAcceptWave + lane];
  AcceptView v;
  v.load(T, a);
  const int src = v.b0;
  const bool swap = uniform(a.action) == DA_SWAP;  // one kind of row per wave (the host's segments)
  const int nGoals = uniform(prog.nGoals);
  for (int g = 0; g < nGoals; ++g) {
    const DevGoal& goal = prog.goals[g];
    int verdict;
    if (swap) {
      verdict = goalAcceptSwap(goal, v, a.sr, src, a.dr, a.dst);
    } else if (goalAcceptMove(goal, v, a.action, a.sr, src, a.dst)) {
      verdict = 0;
    } else {
      // a replica move the rack-aware goals or BrokerSetAwareGoal refuse is a BROKER_REJECT (AbstractRackAwareGoal.java:
      // 100-106, BrokerSetAwareGoal.java:240-246); every other refused move or leadership move a REPLICA_REJECT
      const int kind = uniform(goal.kind);
      const bool rack = kind == DG_RACK_AWARE || kind == DG_RACK_AWARE_DISTRIBUTION || kind == DG_BROKER_SET_AWARE;
      verdict = rack && a.action == DA_MOVE ? 2 : 1;
    }
    cells[lane * nGoals + g] = (int8_t)verdict;
  }
  __syncthreads();
  const int words = kAcceptWave / 4 * nGoals;
  int32_t* dst = reinterpret_cast<int32_t*>(out + wave * kAcceptWave * (size_t)nGoals);
  for (int w = lane; w < words; w += kAcceptWave) dst[w] = reinterpret_cast<const int32_t*>(cells)[w];
}

hipError_t launchAcceptActions(const DevTables& T, const DevProgram& prog, const AcceptRow* rows, int64_t nRows,
                               int8_t* out, hipStream_t st) {
  if (nRows <= 0 || nRows % kAcceptWave != 0 || prog.nGoals < 1 || prog.nGoals > kMaxGoals)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(accept_actions, dim3((unsigned)(nRows / kAcceptWave)), dim3(kAcceptWave), 0, st, T, prog, rows, out);
  return hipGetLastError();
}

}  // namespace ccmi
