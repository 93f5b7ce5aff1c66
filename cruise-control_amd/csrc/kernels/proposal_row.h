// One partition's ExecutionProposal in registers: AnalyzerUtils.getDiff's test and swap (AnalyzerUtils.java:80-88) and the
// sets of ExecutionProposal.java:72-78, read from the tables of PdTables. Shared by the kernels of ccmi_proposal_diff
// (proposal_diff.hip) and of ccmi_execution_plan (execution_plan.hip), so both see the same proposals.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../engine/devtypes.h"

namespace ccmi {

static_assert(kMaxRf == 8, "a proposal has eight slots");
static_assert(R_DISK == 3 && offsetof(ReplicaRec, util) == 0 && offsetof(ReplicaRec, broker) == 32,
              "pdDiff reads util[R_DISK] and broker by their 16-byte words");

// (int) of a double as Java narrows it (JLS 5.1.3): toward zero, saturating, NaN -> 0
__device__ __forceinline__ int32_t pdJavaInt(double x) {
  if (x != x) return 0;
  if (x >= 2147483647.0) return INT32_MAX;
  if (x <= -2147483648.0) return INT32_MIN;
  return (int32_t)x;
}

// One partition's proposal, in registers. `changed` is getDiff's test (:80); the rest is meaningful when it holds.
struct PdRow {
  bool changed;
  int32_t n, size, oldLeader, oldLeaderDisk, flags, nAdd, nRemove, nBetween;
  int32_t oldR[kMaxRf], newR[kMaxRf], oldD[kMaxRf], newD[kMaxRf];
};

__device__ __forceinline__ void pdDiff(const PdTables& T, int p, PdRow& w) {
  const PartitionRec rec = T.parts[p];  // 64 bytes, aligned: four 16-byte loads
  const int a = T.pOff[p];
  const int n = max(0, min(min(T.pOff[p + 1] - a, (int)kMaxRf), T.R - a));
  const int lr = T.pLeader[p];
  const bool disks = T.curDisks != nullptr;
  // the leader: its broker and DISK utilization from its replica record (util[2..3] and {broker, part, orig, flags} are
  // the second and third 16 bytes), its disk from the slot that holds its replica id (getDiff's indexOf, not "slot 0")
  int lb = rec.brokers[0], ld = -1;
  double du = 0.0;
  if ((unsigned)lr < (unsigned)T.R) {
    const uint4* q = reinterpret_cast<const uint4*>(T.replicas + lr);
    const uint4 u23 = q[1], ids = q[2];
    du = __longlong_as_double((long long)(((unsigned long long)u23.w << 32) | u23.z));
    lb = (int)ids.x;
  }
  bool differs = false;
#pragma unroll
  for (int k = 0; k < kMaxRf; ++k) {
    const bool in = k < n;
    w.oldR[k] = in ? T.initDist[a + k] : -1;
    w.newR[k] = in ? rec.brokers[k] : -1;
    w.oldD[k] = in && disks ? T.initDisks[a + k] : -1;
    w.newD[k] = in && disks ? T.curDisks[a + k] : -1;
    if (in && disks && T.pSlots[a + k] == lr) ld = w.newD[k];
    differs = differs || w.oldR[k] != w.newR[k] || w.oldD[k] != w.newD[k];
  }
  w.n = n;
  w.size = pdJavaInt(du);
  w.oldLeader = T.initLeaders[p];
  w.oldLeaderDisk = disks ? T.initLeaderDisks[p] : -1;
  w.changed = differs || w.oldLeader != lb || w.oldLeaderDisk != ld;
  // finalReplicas.indexOf(the leader's placement), then that position and position 0 swap (:84-88)
  int pos = 0;
#pragma unroll
  for (int k = kMaxRf - 1; k >= 0; --k) pos = (k < n && w.newR[k] == lb && w.newD[k] == ld) ? k : pos;
  const int r0 = w.newR[0], d0 = w.newD[0];
  int rp = r0, dp = d0;
#pragma unroll
  for (int k = 1; k < kMaxRf; ++k) {
    rp = k == pos ? w.newR[k] : rp;
    dp = k == pos ? w.newD[k] : dp;
  }
#pragma unroll
  for (int k = 1; k < kMaxRf; ++k) {
    w.newR[k] = k == pos ? r0 : w.newR[k];
    w.newD[k] = k == pos ? d0 : w.newD[k];
  }
  w.newR[0] = rp;
  w.newD[0] = dp;
  // ExecutionProposal.java:72-78 (a partition has no two replicas on one broker, so the sets count list entries)
  int nAdd = 0, nRemove = 0, nBetween = 0;
  bool setsDiffer = false;
#pragma unroll
  for (int k = 0; k < kMaxRf; ++k) {
    bool brokerInOld = false, pairInOld = false, oldInNew = false;
#pragma unroll
    for (int j = 0; j < kMaxRf; ++j) {
      const bool inj = j < n;
      brokerInOld = brokerInOld || (inj && w.newR[k] == w.oldR[j]);
      pairInOld = pairInOld || (inj && w.newR[k] == w.oldR[j] && w.newD[k] == w.oldD[j]);
      oldInNew = oldInNew || (inj && w.oldR[k] == w.newR[j]);
    }
    if (k < n) {
      nAdd += brokerInOld ? 0 : 1;
      nBetween += brokerInOld && !pairInOld ? 1 : 0;
      nRemove += oldInNew ? 0 : 1;
      setsDiffer = setsDiffer || !pairInOld;
    }
  }
  w.nAdd = nAdd;
  w.nRemove = nRemove;
  w.nBetween = nBetween;
  // hasReplicaAction (:212-214), hasLeaderAction (:219-221)
  w.flags = (setsDiffer ? 1 : 0) | ((w.oldLeader != w.newR[0] || w.oldLeaderDisk != w.newD[0]) ? 2 : 0);
}

}  // namespace ccmi
