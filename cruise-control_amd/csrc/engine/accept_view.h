// The predicates' view (predicates.h) of the acceptance kernels: K9 accept_actions (kernels/accept.hip), K10
// accept_mask (kernels/accept_mask.hip) and K11 accept_swaps (kernels/accept_swap.hip). Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "devtypes.h"

namespace ccmi {

// One action: the records of replicas r0 / r1 (r1 = r0 unless a swap), their partitions and the brokers b0 (source) /
// b1 (destination) are values in registers, picked by id; an accessor answers only for those ids. Topic tables, the
// ineligible-broker lists and host capacities are read where a predicate asks for them.
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
  // A move or leadership move of replica a.sr (of partition a.p, on broker a.src) to broker dst: one replica and one
  // partition, so the second of each is the first. Every load but the destination's depends on the row alone — in K10 on
  // wave-uniform values, which the compiler keeps in scalar registers.
  __device__ __forceinline__ void loadMove(const DevTables& T, const SourceRow& a, int dst) {
    t = T;
    r0 = r1 = a.sr;
    p0 = a.p;
    b0 = a.src;
    R0 = T.replicas[a.sr];
    P0 = T.parts[a.p];
    B0 = T.brokers[a.src];
    B1 = T.brokers[dst];
    R1 = R0;
    P1 = P0;
  }
  // A swap of replica a.sr (of partition a.p, on broker a.src) with replica `cand`, whose broker is the destination. The
  // first of each record depends on the row alone (in K11 wave-uniform, scalar registers); the second hangs off the
  // candidate: its ReplicaRec, then that replica's partition and broker.
  __device__ __forceinline__ void loadSwap(const DevTables& T, const SourceRow& a, int cand) {
    t = T;
    r0 = a.sr;
    r1 = cand;
    p0 = a.p;
    b0 = a.src;
    R0 = T.replicas[a.sr];
    P0 = T.parts[a.p];
    B0 = T.brokers[a.src];
    R1 = T.replicas[cand];
    P1 = T.parts[R1.part];
    B1 = T.brokers[R1.broker];
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
  // Partition.brokers of p contains b (GoalUtils.legitMove)
  __device__ __forceinline__ bool hosts(int p, int b) const {
    const bool first = p == p0;
    const int n = first ? P0.n : P1.n;
    bool any = false;
#pragma unroll
    for (int i = 0; i < kMaxRf; ++i) any |= i < n && (first ? P0.brokers[i] : P1.brokers[i]) == b;
    return any;
  }
  // Partition._ineligibleBrokers of p contains b: the CSR list, null when the model has none
  __device__ __forceinline__ bool ineligible(int p, int b) const {
    if (!t.pIneligOff) return false;
    bool in = false;
    for (int k = t.pIneligOff[p]; k < t.pIneligOff[p + 1]; ++k) in |= t.pIneligB[k] == b;
    return in;
  }
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

}  // namespace ccmi
