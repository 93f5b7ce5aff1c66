// gfx950 kernels for ClusterModel.brokerStats (ccmi_broker_stats).
//
// K12 broker_stats_rows  : BasicStats(Broker, potentialBytesOutRate) (BasicStats.java:73-86) of every broker from its
//                          BrokerRec, and the utilization half of Disk.diskStats() (Disk.java:259-264) of every disk.
//     broker_stats_hosts : SingleHostStats.addBasicStats (BasicStats.java:142-155) over each host's broker rows.
//     broker_stats_disks : the sizes of every Disk._replicas and of its leader subset.
// Three launches on the session stream, in that order: the host rows read the broker rows, the member counts land in
// the disk rows the first launch wrote.
// Rows: one lane reads one 128-byte BrokerRec (a whole aligned line pair, eight 16-byte loads) and writes one 128-byte
// ccmi_basic_stats row with eight 16-byte stores; a wavefront's 64 rows are one contiguous 8 KiB run either way, so a
// wave-cooperative transpose would only add lane exchanges to a launch that moves B * 256 bytes. No LDS.
// Hosts: one lane per host walks the host's brokers in ascending index (a static CSR) and adds their rows in double in
// that order — the order of the additions is part of the result, so no atomics and no tree over doubles.
// Disks: one lane per member of a Disk._replicas (the host's flat list of {replica, disk}); integer atomics, which are
// order-free, and the leader bit of the replica's record as the device holds it.
// Built with -ffp-contract=off: every expression is the reference's IEEE double expression.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ccmi.h"
#include "../engine/devtypes.h"

namespace ccmi {

namespace {

constexpr int kStatsRowBlock = 256;

static_assert(sizeof(ccmi_basic_stats) == 128 && sizeof(ccmi_disk_stats) == 40, "ccmi.h row sizes");

// a row leaves as eight 16-byte stores (the struct itself is only 8-byte aligned)
__device__ __forceinline__ void storeRow(ccmi_basic_stats* dst, const ccmi_basic_stats& row) {
  union {
    ccmi_basic_stats s;
    uint4 q[8];
  } u;
  u.s = row;
  uint4* d = reinterpret_cast<uint4*>(dst);
#pragma unroll
  for (int k = 0; k < 8; ++k) d[k] = u.q[k];
}

// BasicStats.diskUtilPct (BasicStats.java:94-96)
__device__ __forceinline__ double diskUtilPct(double diskMb, double diskCap) {
  return diskCap > 0 ? 100 * diskMb / diskCap : -1.0;
}

}  // namespace

// grid over max(B, D) indices: index i < B writes broker row i, index i < D disk row i (counts 0)
__global__ __launch_bounds__(kStatsRowBlock) void broker_stats_rows(
    const BrokerRec* __restrict__ brokers, const BrokerStatic* __restrict__ meta, int B,
    ccmi_basic_stats* __restrict__ out, int D, const double* __restrict__ dUtil, const double* __restrict__ dCap,
    const int32_t* __restrict__ dBroker, ccmi_disk_stats* __restrict__ diskOut) {
  const int i = blockIdx.x * kStatsRowBlock + threadIdx.x;
  if (i < B) {
    const BrokerRec rec = brokers[i];
    const BrokerStatic st = meta[i];
    ccmi_basic_stats r;
    r.disk_mb = ldMax0(rec.nrep == 0 ? 0.0 : rec.util[R_DISK]);
    r.cpu_pct = ldMax0(100.0 * rec.util[R_CPU] / rec.cap[R_CPU]);
    r.leader_nw_in_rate = ldMax0(rec.lbi);
    r.follower_nw_in_rate = ldMax0(rec.util[R_NW_IN] - r.leader_nw_in_rate);
    r.nw_out_rate = ldMax0(rec.util[R_NW_OUT]);
    r.pnw_out_rate = ldMax0(rec.pot);
    r.disk_capacity_mb = ldMax0(rec.cap[R_DISK]);
    r.network_in_capacity = ldMax0(rec.cap[R_NW_IN]);
    r.network_out_capacity = ldMax0(rec.cap[R_NW_OUT]);
    r.num_core = ldMax0(rec.cap[R_CPU] / 100);
    r.disk_pct = diskUtilPct(r.disk_mb, r.disk_capacity_mb);
    r.replicas = rec.nrep;
    r.leaders = rec.nlead;
    r.broker = i;
    r.state = st.state;
    r.host = st.host;
    r.rack = rec.rack;
    r.reserved[0] = r.reserved[1] = r.reserved[2] = r.reserved[3] = 0;
    storeRow(out + i, r);
  }
  if (i < D) {
    const double cap = dCap[i], util = dUtil[i];
    ccmi_disk_stats d;
    const bool dead = !(cap > 0);  // DiskStats: utilization null unless capacity > 0
    d.disk_mb = dead ? -1.0 : util;
    d.disk_pct = dead ? -1.0 : util * 100.0 / cap;
    d.capacity = cap;
    d.num_replicas = 0;
    d.num_leader_replicas = 0;
    d.disk = i;
    d.broker = dBroker[i];
    diskOut[i] = d;
  }
}

// one lane per host: hBrk[hOff[h], hOff[h + 1]) are the host's brokers in ascending index, hIdx[h] its host index
__global__ __launch_bounds__(kStatsRowBlock) void broker_stats_hosts(
    const ccmi_basic_stats* __restrict__ rows, const int32_t* __restrict__ hOff, const int32_t* __restrict__ hBrk,
    const int32_t* __restrict__ hIdx, int H, int B, ccmi_basic_stats* __restrict__ out) {
  const int h = blockIdx.x * kStatsRowBlock + threadIdx.x;
  if (h >= H) return;
  ccmi_basic_stats a;  // SingleHostStats starts from BasicStats' zeros
  a.disk_mb = a.cpu_pct = a.leader_nw_in_rate = a.follower_nw_in_rate = a.nw_out_rate = a.pnw_out_rate = 0.0;
  a.disk_capacity_mb = a.network_in_capacity = a.network_out_capacity = a.num_core = 0.0;
  a.replicas = a.leaders = 0;
  a.rack = -1;
  const int k0 = hOff[h], k1 = hOff[h + 1];
  for (int k = k0; k < k1; ++k) {
    const int b = hBrk[k];
    if ((unsigned)b >= (unsigned)B) continue;
    const ccmi_basic_stats r = rows[b];
    a.disk_mb += r.disk_mb;
    a.cpu_pct += r.cpu_pct;
    a.leader_nw_in_rate += r.leader_nw_in_rate;
    a.follower_nw_in_rate += r.follower_nw_in_rate;
    a.nw_out_rate += r.nw_out_rate;
    a.pnw_out_rate += r.pnw_out_rate;
    a.replicas += r.replicas;
    a.leaders += r.leaders;
    a.disk_capacity_mb += r.disk_capacity_mb;
    a.num_core += r.num_core;
    a.network_in_capacity += r.network_in_capacity;
    a.network_out_capacity += r.network_out_capacity;
    if (k == k0) a.rack = r.rack;
  }
  a.disk_pct = diskUtilPct(a.disk_mb, a.disk_capacity_mb);
  a.broker = -1;
  a.state = -1;
  a.host = hIdx[h];
  a.reserved[0] = a.reserved[1] = a.reserved[2] = a.reserved[3] = 0;
  storeRow(out + h, a);
}

// one lane per Disk._replicas member
__global__ __launch_bounds__(kStatsRowBlock) void broker_stats_disks(const DiskMember* __restrict__ members, int64_t E,
                                                                     const ReplicaRec* __restrict__ replicas, int R,
                                                                     int D, ccmi_disk_stats* __restrict__ diskOut) {
  const int64_t e = (int64_t)blockIdx.x * kStatsRowBlock + threadIdx.x;
  if (e >= E) return;
  const DiskMember m = members[e];
  if ((unsigned)m.replica >= (unsigned)R || (unsigned)m.disk >= (unsigned)D) return;
  atomicAdd(&diskOut[m.disk].num_replicas, 1);
  if (replicas[m.replica].flags & RF_LEADER) atomicAdd(&diskOut[m.disk].num_leader_replicas, 1);
}

hipError_t launchBrokerStatsRows(const BrokerRec* brokers, const BrokerStatic* meta, int B, ccmi_basic_stats* out, int D,
                                 const double* dUtil, const double* dCap, const int32_t* dBroker,
                                 ccmi_disk_stats* diskOut, hipStream_t st) {
  if (B < 1 || D < 0 || !brokers || !meta || !out || (D > 0 && (!dUtil || !dCap || !dBroker || !diskOut)))
    return hipErrorInvalidValue;
  const int n = B > D ? B : D;
  hipLaunchKernelGGL(broker_stats_rows, dim3((unsigned)((n + kStatsRowBlock - 1) / kStatsRowBlock)),
                     dim3(kStatsRowBlock), 0, st, brokers, meta, B, out, D, dUtil, dCap, dBroker, diskOut);
  return hipGetLastError();
}

hipError_t launchBrokerStatsHosts(const ccmi_basic_stats* rows, const int32_t* hOff, const int32_t* hBrk,
                                  const int32_t* hIdx, int H, int B, ccmi_basic_stats* out, hipStream_t st) {
  if (H < 1 || H > B || !rows || !hOff || !hBrk || !hIdx || !out) return hipErrorInvalidValue;
  hipLaunchKernelGGL(broker_stats_hosts, dim3((unsigned)((H + kStatsRowBlock - 1) / kStatsRowBlock)),
                     dim3(kStatsRowBlock), 0, st, rows, hOff, hBrk, hIdx, H, B, out);
  return hipGetLastError();
}

hipError_t launchBrokerStatsDisks(const DiskMember* members, int64_t E, const ReplicaRec* replicas, int R, int D,
                                  ccmi_disk_stats* diskOut, hipStream_t st) {
  if (E < 1 || E > (int64_t)INT32_MAX * kStatsRowBlock || R < 1 || D < 1 || !members || !replicas || !diskOut)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(broker_stats_disks, dim3((unsigned)((E + kStatsRowBlock - 1) / kStatsRowBlock)),
                     dim3(kStatsRowBlock), 0, st, members, E, replicas, R, D, diskOut);
  return hipGetLastError();
}

}  // namespace ccmi
