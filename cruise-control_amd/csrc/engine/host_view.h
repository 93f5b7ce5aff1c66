// HostView: the host model as predicates.h sees it (the same expressions the kernels evaluate). Used by the engine's
// host prefixes and single acceptance calls, and by the queue diagnostics' reference loop (ccmi_queue_probe.cpp).
#pragma once
#include <cstdint>
#include <vector>

#include "devtypes.h"
#include "model.h"

namespace ccmi {

struct HostView {
  const Model& m;
  const std::vector<const std::vector<uint8_t>*>& allowedBySlot;
  const std::vector<int32_t>& tUp;
  const std::vector<int32_t>& tLo;
  const std::vector<int32_t>& bSet;  // BrokerSetAwareGoal: broker set of every broker / replica (empty: none)
  const std::vector<int32_t>& rSet;
  const std::vector<int32_t>& tMin;  // MinTopicLeadersPerBrokerGoal minima (empty: none)
  const std::vector<int32_t>& tLim;  // TopicLeaderReplicaDistributionGoal limits [T][2] (empty: none)
  double bu(int b, int res) const { return m.bu(b, res); }
  double bcap(int b, int res) const { return m.cap(b, res); }
  bool hostMode() const { return m.hostMode(); }
  double hu(int b, int res) const { return m.hu(b, res); }
  double hcap(int b, int res) const { return m.hcap(b, res); }
  int nrep(int b) const { return m.nrep(b); }
  bool alive(int b) const { return m.alive(b); }
  bool allowed(int slot, int b) const { return (*allowedBySlot[slot])[b] != 0; }
  double ru(int r, int res) const { return m.ru(r, res); }
  int flags(int r) const { return (m.rLeader[r] ? RF_LEADER : 0) | (m.rOrigOff[r] ? RF_ORIG_OFFLINE : 0); }
  int rbroker(int r) const { return m.rBroker[r]; }
  int rorig(int r) const { return m.rOrig[r]; }
  bool origOff(int r) const { return m.origOffline(r); }
  int rpart(int r) const { return m.rPart[r]; }
  int pbegin(int p) const { return m.pOff[p]; }
  int pend(int p) const { return m.pOff[p + 1]; }
  int pbroker(int i) const { return m.rBroker[m.pSlots[i]]; }
  bool hosts(int p, int b) const {
    bool has = false;
    for (int i = pbegin(p); i < pend(p); ++i) has |= (pbroker(i) == b);
    return has;
  }
  int rack(int b) const { return m.bRack[b]; }
  bool ineligible(int p, int b) const { return m.ineligible(p, b); }
  bool otherOnRack(int p, int self, int rk) const {
    for (int i = pbegin(p); i < pend(p); ++i)
      if (pbroker(i) != self && m.bRack[pbroker(i)] == rk) return true;
    return false;
  }
  int slotRack(int, int b) const { return m.bRack[b]; }
  int rackCount(int p, int rk) const {
    int c = 0;
    for (int i = pbegin(p); i < pend(p); ++i) c += m.bRack[pbroker(i)] == rk ? 1 : 0;
    return c;
  }
  int nlead(int b) const { return m.bNlead[b]; }
  double pot(int b) const { return m.potNwOut(b); }
  double lnwin(int b) const { return m.leadNwIn(b); }
  double pLeadNwOut(int p) const { return m.pLeadNwOut(p); }
  int ptopic(int p) const { return m.pTopic[p]; }
  int tcount(int t, int b) const { return m.tcount(t, b); }
  int tUpper(int t) const { return tUp[t]; }
  int tLower(int t) const { return tLo[t]; }
  int bset(int b) const { return bSet.empty() ? -1 : bSet[b]; }
  int rbset(int r) const { return rSet.empty() ? -1 : rSet[r]; }
  int tlead(int t, int b) const { return m.tlead(t, b); }
  int tMinLead(int t) const { return tMin.empty() ? -1 : tMin[t]; }
  int tLeadUpper(int t) const { return tLim[2 * t]; }
  int tLeadLower(int t) const { return tLim[2 * t + 1]; }
};

}  // namespace ccmi
