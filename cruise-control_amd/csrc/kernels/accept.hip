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

#include "../engine/devtypes.h"
#include "../engine/predicates.h"

namespace ccmi {

namespace {

constexpr int kAcceptWave = 64;

// The predicates' view (predicates.h) of one action: the records of replicas r0 / r1 (r1 = r0 unless a swap), their
// partitions and the brokers b0 (source) / b1 (destination) are values in registers, picked by id; an accessor answers
// only for those ids. Topic tables and host capacities are read where a goal asks for them.
struct AcceptView {
  DevTables t;
  int r0, r1, p0, b0;
  ReplicaRec R0, R1;
  PartitionRec P0, P1;
  BrokerRec B0, B1;

  static __device__ __forceinline__ double pick(const double (&a)[4], int k) {
    return k == 0 ? a[0] : (k == 1 ? a[1] : (k == 2 ? a[2] : a[3]));
  }
  static __device__ __forceinline__ double pick3(const double (&a)[3], int k) {
    return k == 0 ? a[0] : (k == 1 ? a[1] : a[2]);
  }
  __device__ __forceinline__ void load(const DevTables& T, const AcceptRow& a) {
    t = T;
    r0 = a.sr;
    r1 = a.dr >= 0 ? a.dr : a.sr;
    R0 = T.replicas[r0];
    R1 = T.replicas[r1];
    B1 = T.brokers[a.dst];
    p0 = R0.part;
    b0 = R0.broker;
    P0 = T.parts[p0];
    P1 = T.parts[R1.part];
    B0 = T.brokers[b0];
  }

  __device__ __forceinline__ double bu(int b, int res) const { return b == b0 ? pick(B0.util, res) : pick(B1.util, res); }
  __device__ __forceinline__ double bcap(int b, int res) const { return b == b0 ? pick(B0.cap, res) : pick(B1.cap, res); }
  __device__ __forceinline__ bool hostMode() const { return t.hostCap != nullptr; }
  __device__ __forceinline__ double hu(int b, int res) const {
    if (!t.hostCap) return bu(b, res);
    return b == b0 ? pick3(B0.hutil, res) : pick3(B1.hutil, res);
  }
  __device__ __forceinline__ double hcap(int b, int res) const {
    return t.hostCap ? t.hostCap[3 * (size_t)b + res] : bcap(b, res);
  }
  __device__ __forceinline__ int nrep(int b) const { return b == b0 ? B0.nrep : B1.nrep; }
  __device__ __forceinline__ bool alive(int b) const { return (b == b0 ? B0.alive : B1.alive) != 0; }
  __device__ __forceinline__ bool allowed(int slot, int b) const {
    return ((b == b0 ? B0.allowedBits : B1.allowedBits) >> slot) & 1u;
  }
  __device__ __forceinline__ double ru(int r, int res) const { return r == r0 ? pick(R0.util, res) : pick(R1.util, res); }
  __device__ __forceinline__ int flags(int r) const { return r == r0 ? R0.flags : R1.flags; }
  __device__ __forceinline__ int rbroker(int r) const { return r == r0 ? R0.broker : R1.broker; }
  __device__ __forceinline__ int rorig(int r) const { return r == r0 ? R0.orig : R1.orig; }
  __device__ __forceinline__ bool origOff(int r) const { return (flags(r) & (RF_ORIG_OFFLINE | RF_ORIG_DEAD)) != 0; }
  __device__ __forceinline__ int rpart(int r) const { return r == r0 ? R0.part : R1.part; }
  __device__ __forceinline__ int rack(int b) const { return b == b0 ? B0.rack : B1.rack; }
  __device__ __forceinline__ bool otherOnRack(int p, int self, int rk) const {
    const bool first = p == p0;
    const int n = first ? P0.n : P1.n;
    bool any = false;
#pragma unroll
    for (int i = 0; i < kMaxRf; ++i) {
      const int br = first ? P0.brokers[i] : P1.brokers[i];
      const int rki = first ? P0.racks[i] : P1.racks[i];
      any |= i < n && br != self && rki == rk;
    }
    return any;
  }
  __device__ __forceinline__ int slotRack(int /*p*/, int b) const { return rack(b); }
  __device__ __forceinline__ int rackCount(int p, int rk) const {
    const bool first = p == p0;
    const int n = first ? P0.n : P1.n;
    int c = 0;
#pragma unroll
    for (int i = 0; i < kMaxRf; ++i) c += (i < n && (first ? P0.racks[i] : P1.racks[i]) == rk) ? 1 : 0;
    return c;
  }
  __device__ __forceinline__ int nlead(int b) const { return b == b0 ? B0.nlead : B1.nlead; }
  __device__ __forceinline__ double pot(int b) const { return b == b0 ? B0.pot : B1.pot; }
  __device__ __forceinline__ double lnwin(int b) const { return b == b0 ? B0.lbi : B1.lbi; }
  __device__ __forceinline__ double pLeadNwOut(int p) const { return p == p0 ? P0.leadNwOut : P1.leadNwOut; }
  __device__ __forceinline__ int ptopic(int p) const { return p == p0 ? P0.topic : P1.topic; }
  __device__ __forceinline__ int tcount(int tp, int b) const { return t.topicCount[(size_t)tp * t.ldB + b]; }
  __device__ __forceinline__ int tUpper(int tp) const { return t.tUpper[tp]; }
  __device__ __forceinline__ int tLower(int tp) const { return t.tLower[tp]; }
  __device__ __forceinline__ int bset(int b) const { return b == b0 ? B0.bset : B1.bset; }
  __device__ __forceinline__ int rbset(int r) const { return r == r0 ? R0.bset : R1.bset; }
  __device__ __forceinline__ int tlead(int tp, int b) const { return t.topicLead[(size_t)tp * t.ldB + b]; }
  __device__ __forceinline__ int tMinLead(int tp) const { return t.tMinLead ? t.tMinLead[tp] : -1; }
  __device__ __forceinline__ int tLeadUpper(int tp) const { return t.tLeadLim[2 * tp]; }
  __device__ __forceinline__ int tLeadLower(int tp) const { return t.tLeadLim[2 * tp + 1]; }
};

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
