// ccmi_broker_stats (additive at ABI v13): ClusterModel.brokerStats of the session's current model, computed on the
// device from the resident tables (Device::brokerStats, kernels/broker_stats.hip). A translation unit of its own: it
// holds the only caller of that launcher, which the test emulation of Device does not have. No per-broker arithmetic
// happens here: the host sends the static host CSR once and the disks' member list when it changed.
#include <algorithm>
#include <numeric>
#include <stdexcept>
#include <vector>

#include "ccmi.h"
#include "ccmi_session.h"
#include "engine/threadpin.h"

namespace {

// Once per session: every broker's desc host index and state, the distinct hosts in ascending host index with their
// brokers in ascending broker index, every disk's broker.
void uploadStatic(const ccmi::Model& m, ccmi::Device& dev) {
  std::vector<ccmi::BrokerStatic> meta((size_t)m.B);
  for (int b = 0; b < m.B; ++b) meta[(size_t)b] = ccmi::BrokerStatic{m.bHostDesc[b], (int32_t)m.bState[b]};
  std::vector<int32_t> hBrk((size_t)m.B), hOff, hIdx;
  std::iota(hBrk.begin(), hBrk.end(), 0);
  std::stable_sort(hBrk.begin(), hBrk.end(), [&](int x, int y) { return m.bHostDesc[x] < m.bHostDesc[y]; });
  for (int k = 0; k < m.B; ++k)
    if (k == 0 || m.bHostDesc[hBrk[k]] != m.bHostDesc[hBrk[k - 1]]) {
      hOff.push_back(k);
      hIdx.push_back(m.bHostDesc[hBrk[k]]);
    }
  hOff.push_back(m.B);
  dev.uploadStatsStatic(meta.data(), (int)hIdx.size(), hOff.data(), hBrk.data(), hIdx.data(), m.dBroker.data());
}

}  // namespace

extern "C" ccmi_status ccmi_broker_stats(ccmi_session* s, ccmi_basic_stats* brokers, ccmi_basic_stats* hosts,
                                         int32_t* num_hosts, ccmi_disk_stats* disks) {
  return guarded([&] {
    if (!s) throw std::invalid_argument("null session");
    if (!brokers) throw std::invalid_argument("null argument");
    ccmi::Model& m = s->model;
    ccmi::Device& dev = *s->device;
    if (m.B < 1) throw std::invalid_argument("a model without brokers has no broker stats");
    const ccmi::ThreadPin pin(s->deviceOrdinal);  // restored when the call returns
    if (!dev.statsStaticUploaded()) uploadStatic(m, dev);
    m.flushToDevice();  // the rows the host changed since the last launch (ccmi_session_apply, a goal's moves)
    const bool withDisks = disks && m.D > 0;
    // every Disk._replicas entry as {replica, disk}: rebuilt only when a set changed since the list the device holds
    std::vector<ccmi::DiskMember> members;
    if (withDisks) {
      if (m.diskDirty) {  // Disk._utilization, as ccmi_compute_cluster_stats brings it current
        dev.setDiskUtil(m.dUtil.data());
        m.diskDirty = false;
      }
      if (dev.statsMemberVer() != m.diskMemberVer) {
        size_t n = 0;
        for (const auto& v : m.dMembers) n += v.size();
        members.reserve(n);
        for (int d = 0; d < m.D; ++d)
          for (int r : m.dMembers[(size_t)d]) members.push_back(ccmi::DiskMember{r, d});
      }
    }
    dev.brokerStats(brokers, hosts, withDisks ? disks : nullptr, members.data(), (int64_t)members.size(),
                    m.diskMemberVer);
    if (num_hosts) *num_hosts = dev.statsHosts();
    return CCMI_OK;
  });
}
