// gfx950 kernel for swap-candidate grids (ccmi_swaps_acceptance_grid).
//
// K11 accept_swaps : for each (source replica, candidate replica) pair one code — what the loop body of
//                    AbstractGoal.maybeApplySwapAction (AbstractGoal.java:287-338) asks before its own selfSatisfied:
//                    3 when legitMove(source, candidate's broker) fails (:308), else 4 when legitMove(candidate, source's
//                    broker) fails (:313), else the first verdict of the program's goals that is not ACCEPT
//                    (AnalyzerUtils.java:169-179: 1 REPLICA_REJECT, 2 BROKER_REJECT), else 0.
// One wavefront (a workgroup) produces 64 consecutive candidates of one source. The candidate block is blockIdx.x (the
// dimension that can be large) and the source blockIdx.y, so the SourceRow, the source's replica, partition and broker
// records and everything derived from them are wave-uniform: scalar loads, scalar registers. A lane loads its
// candidate's replica id, then its ReplicaRec, then that replica's PartitionRec and BrokerRec (three dependent levels),
// plus the topic cells the topic goals ask for. The goal loop is outermost with a scalar trip count; every lane
// evaluates the goal and a lane still at 0 takes the verdict, and a wave leaves the loop once no lane is at 0. Lanes
// past the last candidate (the tail block) read candidate m - 1 and store nothing. A row of the output is `pitch` bytes,
// a multiple of 64, so a wave's codes are one aligned 64-byte run of ordinary byte stores. No atomics, no LDS.
// Built with -ffp-contract=off: every predicate is the reference's IEEE double expression.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../engine/accept_view.h"
#include "../engine/devtypes.h"
#include "../engine/predicates.h"

namespace ccmi {

namespace {

constexpr int kSwapWave = 64;

}  // namespace

// rows[0, gridDim.y), cands[0, m); grid (pitch / 64, nSources); out[source * pitch + candidate].
__global__ __launch_bounds__(kSwapWave) void accept_swaps(DevTables T, DevProgram prog,
                                                          const SourceRow* __restrict__ rows,
                                                          const int32_t* __restrict__ cands, int m, int64_t pitch,
                                                          int8_t* __restrict__ out) {
  const size_t source = blockIdx.y;
  const int lane = threadIdx.x;
  const SourceRow a = rows[source];
  const int64_t j = (int64_t)blockIdx.x * kSwapWave + lane;
  const bool inRange = j < m;
  const int dr = cands[inRange ? j : (int64_t)m - 1];
  AcceptView v;
  v.loadSwap(T, a, dr);
  const int db = v.R1.broker;
  int code = !legitMove(v, a.sr, db, DA_MOVE) ? 3 : (!legitMove(v, dr, a.src, DA_MOVE) ? 4 : 0);
  const int nGoals = uniform(prog.nGoals);
  for (int g = 0; g < nGoals && __ballot(inRange && code == 0) != 0; ++g) {
    const int verdict = goalAcceptSwap(prog.goals[g], v, a.sr, a.src, dr, db);
    code = code == 0 ? verdict : code;
  }
  if (inRange) out[source * (size_t)pitch + (size_t)j] = (int8_t)code;
}

hipError_t launchAcceptSwaps(const DevTables& T, const DevProgram& prog, const SourceRow* rows, int64_t nSources,
                             const int32_t* cands, int64_t m, int8_t* out, hipStream_t st) {
  const int64_t blocks = (m + kSwapWave - 1) / kSwapWave;
  if (nSources <= 0 || nSources > 65535 || m <= 0 || m > kMaxSwapCandidates || prog.nGoals < 0 || prog.nGoals > kMaxGoals)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(accept_swaps, dim3((unsigned)blocks, (unsigned)nSources), dim3(kSwapWave), 0, st, T, prog, rows,
                     cands, (int)m, blocks * kSwapWave, out);
  return hipGetLastError();
}

}  // namespace ccmi
