// gfx950 kernel for destination-broker masks (ccmi_moves_acceptance_mask).
//
// K10 accept_mask : for each source (a replica that moves, or a leader that gives up leadership) the set of destination
//                   brokers that are legit (GoalUtils.legitMove) and that every goal of the program ACCEPTs — what the
//                   loop of AbstractGoal.maybeApplyBalancingAction (AbstractGoal.java:243-270) asks of each candidate
//                   broker, for all brokers at once, one bit per broker.
// One wavefront (a workgroup) produces one output word: 64 consecutive destination brokers of one source. The source
// index is blockIdx.x (the dimension that can be large) and the word index blockIdx.y, so the SourceRow, the source's
// replica, partition and broker records and everything derived from them are wave-uniform: scalar loads, scalar
// registers. A lane loads only its destination's BrokerRec (64 consecutive 128-byte records per wave), plus the topic
// count cells the topic goals ask for. The goal loop is outermost with a scalar trip count; a wave leaves it once its
// ballot of still-accepted lanes is empty. Lanes past the last broker (the tail word) read broker B - 1 and contribute 0.
// Lane 0 stores the ballot with one ordinary 8-byte store. No atomics, no LDS.
// Built with -ffp-contract=off: every predicate is the reference's IEEE double expression.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../engine/accept_view.h"
#include "../engine/devtypes.h"
#include "../engine/predicates.h"

namespace ccmi {

namespace {

constexpr int kMaskWave = 64;

}  // namespace

// rows[0, nSources); grid (nSources, W), W = (T.B + 63) / 64 words per source; out[source * W + word].
__global__ __launch_bounds__(kMaskWave) void accept_mask(DevTables T, DevProgram prog,
                                                         const SourceRow* __restrict__ rows,
                                                         unsigned long long* __restrict__ out) {
  const size_t source = blockIdx.x;
  const int word = blockIdx.y;
  const int lane = threadIdx.x;
  const SourceRow a = rows[source];
  const int b = word * kMaskWave + lane;
  const bool inRange = b < T.B;
  const int dst = inRange ? b : T.B - 1;
  AcceptView v;
  v.loadMove(T, a, dst);
  bool ok = inRange && dst != a.src && legitMove(v, a.sr, dst, a.action);
  unsigned long long accepted = __ballot(ok);
  const int nGoals = prog.nGoals;
  for (int g = 0; g < nGoals && accepted != 0; ++g) {
    ok &= goalAcceptMove(prog.goals[g], v, a.action, a.sr, a.src, dst);
    accepted = __ballot(ok);
  }
  if (lane == 0) out[source * gridDim.y + word] = accepted;
}

hipError_t launchAcceptMask(const DevTables& T, const DevProgram& prog, const SourceRow* rows, int64_t nSources,
                            unsigned long long* out, hipStream_t st) {
  const int64_t W = ((int64_t)T.B + kMaskWave - 1) / kMaskWave;
  if (nSources <= 0 || nSources > INT32_MAX || T.B < 1 || W > 65535 || prog.nGoals < 0 || prog.nGoals > kMaxGoals)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(accept_mask, dim3((unsigned)nSources, (unsigned)W), dim3(kMaskWave), 0, st, T, prog, rows, out);
  return hipGetLastError();
}

}  // namespace ccmi
