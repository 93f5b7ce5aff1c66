// Device::acceptBatch, Device::maskBatch and Device::swapGridBatch (device.h): the launchers of K9 accept_actions
// (kernels/accept.hip), K10 accept_mask (kernels/accept_mask.hip) and K11 accept_swaps (kernels/accept_swap.hip), which
// share one chunk protocol (Device::acceptChunk); and Device::brokerStats, the launcher of K12
// (kernels/broker_stats.hip), Device::partitionLoad, the launcher of K13 (kernels/partition_load.hip), and
// Device::proposalDiff, the launcher of K14 (kernels/proposal_diff.hip), and Device::sortedReplicas, the launcher of K15
// (kernels/sorted_replicas.hip), and Device::executionPlan, the launcher of K16 (kernels/execution_plan.hip), which
// share its scope and timing. A translation unit of its own, linked into libccmi.so
// only: the test emulation of Device has none of these kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>

#include "ccmi.h"
#include "device.h"
#include "hip_check.h"
#include "prof.h"

namespace ccmi {

hipError_t launchAcceptActions(const DevTables& T, const DevProgram& prog, const AcceptRow* rows, int64_t nRows,
                               int8_t* out, hipStream_t st);
hipError_t launchAcceptMask(const DevTables& T, const DevProgram& prog, const SourceRow* rows, int64_t nSources,
                            unsigned long long* out, hipStream_t st);
hipError_t launchAcceptSwaps(const DevTables& T, const DevProgram& prog, const SourceRow* rows, int64_t nSources,
                             const int32_t* cands, int64_t m, int8_t* out, hipStream_t st);
hipError_t launchBrokerStatsRows(const BrokerRec* brokers, const BrokerStatic* meta, int B, ccmi_basic_stats* out, int D,
                                 const double* dUtil, const double* dCap, const int32_t* dBroker,
                                 ccmi_disk_stats* diskOut, hipStream_t st);
hipError_t launchBrokerStatsHosts(const ccmi_basic_stats* rows, const int32_t* hOff, const int32_t* hBrk,
                                  const int32_t* hIdx, int H, int B, ccmi_basic_stats* out, hipStream_t st);
hipError_t launchBrokerStatsDisks(const DiskMember* members, int64_t E, const ReplicaRec* replicas, int R, int D,
                                  ccmi_disk_stats* diskOut, hipStream_t st);
hipError_t launchSyncLoads(const ChainTables& C, const LoadRow* lrows, int nl, const SlotRow* srows, int ns,
                           hipStream_t st);
hipError_t launchPartitionLoad(const PlTables& T, const PlQuery& q, PlState* st, PlEntry* bufA, PlEntry* bufB,
                               uint32_t* counts, int tiles, int slots, ccmi_partition_load_record* out, int cap,
                               int* launches, hipStream_t stream);
hipError_t launchProposalDiff(const PdTables& T, uint32_t* counts, int tiles, PdSums* sums, ccmi_proposal_record* out,
                              int cap, int* launches, hipStream_t stream);
hipError_t launchSortedReplicasCount(const SrTables& T, const SrQuery& q, int n, uint64_t* keys, int32_t* segOf,
                                     uint32_t* counts, uint32_t* cursor, unsigned long long* state, int* launches,
                                     hipStream_t stream);
hipError_t launchSortedReplicasFill(const SrTables& T, const SrQuery& q, int n, const uint64_t* keys,
                                    const int32_t* segOf, uint32_t* cursor, const unsigned long long* state,
                                    long long total, long long maxLen, SortEntry* bufA, SortEntry* bufB,
                                    ccmi_swap_replica* records, double* scores, int* launches, hipStream_t stream);
hipError_t launchExecutionPlanCount(const EpTables& T, int tiles, EpRow* rows, uint32_t* tileInter,
                                    uint32_t* tileLeader, uint32_t* counts, uint32_t* cursors, EpSums* sums,
                                    unsigned long long* state, int* launches, hipStream_t stream);
hipError_t launchExecutionPlanFill(const EpTables& T, const EpQuery& q, int tiles, const EpRow* rows,
                                   const uint32_t* tileInter, const uint32_t* tileLeader, uint32_t* cursors,
                                   const unsigned long long* state, long long numInter, long long numLeader,
                                   long long interTotal, long long interMax, long long intraTotal, long long intraMax,
                                   SortEntry* bufA, SortEntry* bufB, int32_t* idOf, ccmi_plan_task* tasks,
                                   int32_t* interOut, int32_t* order, int32_t* intraOut, int32_t* leaderOut,
                                   int* launches, hipStream_t stream);

namespace {
constexpr double kAcceptWaitSeconds = 120.0;

// one table of a static block: a synchronous copy of the host's n elements
template <class P>
void upload(P* d, const P* h, size_t n, const char* what) {
  if (h && n) hipCheck(hipMemcpy(d, h, n * sizeof(P), hipMemcpyHostToDevice), what);
}
}  // namespace

// The session's device current and the device-scan phase open for the call; plain launches on the session stream, so the
// server stops first (none is resident between API calls anyway).
struct Device::PlainLaunch {
  DeviceGuard dg;
  PhaseScope ps;
  Device& d;
  explicit PlainLaunch(Device& dev) : dg(dev.ordinal_), ps(PH_DEV_SCAN), d(dev) { d.stopServer(); }
  // a call with nothing to launch still takes the pending row updates to the tables
  bool nothingToDo(bool empty) {
    if (empty) d.flushPending();
    return empty;
  }
};

template <class Launch>
void Device::timedLaunch(Launch launch) {
  if (timing) (void)hipEventRecord((hipEvent_t)ev0_, (hipStream_t)st_);
  launch();
  if (timing) (void)hipEventRecord((hipEvent_t)ev1_, (hipStream_t)st_);
}

void Device::addKernelMs(double& total) {
  if (!timing) return;
  float ms = 0.f;
  hipCheck(hipEventElapsedTime(&ms, (hipEvent_t)ev0_, (hipEvent_t)ev1_), "hipEventElapsedTime");
  total += ms;
}

template <class Fill, class Launch>
void Device::acceptChunk(size_t req, Fill fill, size_t outBytes, Launch launch, void* dst, const char* kernel,
                         const char* copy) {
  const hipStream_t st = (hipStream_t)st_;
  // the chunk's request goes into HBM with the pending row updates (prep; the first chunk carries them all)
  const Staged g = packUpdates(req);
  fill(hStage_ + g.end);
  launchPrepFor(g, req, false);
  acceptOut_.ensure(outBytes);
  timedLaunch([&] { hipCheck(launch(st), kernel); });
  hipCheck(hipMemcpyAsync(dst, dAccept(), outBytes, hipMemcpyDeviceToHost, st), copy);
  streamWait(kernel, kAcceptWaitSeconds);
  perf.syncs++;
  perf.acceptLaunches++;  // acceptCells is the caller's count: it knows which rows are padding and which exits were early
  addKernelMs(perf.acceptKernelMs);
}

void Device::acceptBatch(const DevProgram& prog, const AcceptRow* rows, int64_t nRows, int64_t nMoveRows, int8_t* out) {
  PlainLaunch call(*this);
  if (nRows % 64 != 0 || nMoveRows % 64 != 0 || nMoveRows < 0 || nMoveRows > nRows)
    throw std::logic_error("acceptBatch takes whole wavefronts of each row kind");
  if (prog.nGoals < 1 || prog.nGoals > kMaxGoals) throw std::logic_error("acceptBatch: goal count");
  if (call.nothingToDo(nRows == 0)) return;
  const size_t G = (size_t)prog.nGoals;
  const int64_t chunk = acceptChunkRows_;  // a multiple of 64, so a chunk boundary never splits a wavefront
  for (int64_t r0 = 0; r0 < nRows; r0 += chunk) {
    const int64_t n = std::min(chunk, nRows - r0);
    const size_t req = (size_t)n * sizeof(AcceptRow);
    acceptChunk(
        req, [&](char* p) { std::memcpy(p, rows + r0, req); }, (size_t)n * G,
        [&](hipStream_t st) { return launchAcceptActions(tables(), prog, (const AcceptRow*)dReq_, n, dAccept(), st); },
        out + (size_t)r0 * G, "accept_actions", "D2H acceptance");
  }
}

void Device::maskBatch(const DevProgram& prog, const SourceRow* rows, int64_t nSources, uint64_t* out) {
  PlainLaunch call(*this);
  if (nSources < 0 || prog.nGoals < 0 || prog.nGoals > kMaxGoals) throw std::logic_error("maskBatch: counts");
  if (call.nothingToDo(nSources == 0)) return;
  const size_t W = (size_t)maskWords();
  const int64_t chunk = maskChunkSources_;
  for (int64_t s0 = 0; s0 < nSources; s0 += chunk) {
    const int64_t n = std::min(chunk, nSources - s0);
    const size_t req = (size_t)n * sizeof(SourceRow);
    acceptChunk(
        req, [&](char* p) { std::memcpy(p, rows + s0, req); }, (size_t)n * W * sizeof(uint64_t),
        [&](hipStream_t st) {
          return launchAcceptMask(tables(), prog, (const SourceRow*)dReq_, n, (unsigned long long*)dAccept(), st);
        },
        out + (size_t)s0 * W, "accept_mask", "D2H masks");
  }
}

void Device::swapGridBatch(const DevProgram& prog, const SourceRow* rows, int64_t nSources, const int32_t* cands,
                           int64_t m, int8_t* out) {
  PlainLaunch call(*this);
  if (nSources < 0 || m < 0 || prog.nGoals < 0 || prog.nGoals > kMaxGoals) throw std::logic_error("swapGridBatch: counts");
  if (m > kMaxSwapCandidates)
    throw std::invalid_argument("a swap grid takes at most " + std::to_string(kMaxSwapCandidates) + " candidates");
  if (call.nothingToDo(nSources == 0 || m == 0)) return;
  // a row of the device buffer is whole wavefronts: a wave's 64 codes are one aligned 64-byte run
  const size_t pitch = (size_t)((m + 63) / 64 * 64);
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(65535, swapChunkCells_ / (int64_t)pitch));
  const size_t oCand = (size_t)std::min(chunk, nSources) * sizeof(SourceRow);  // 16-byte rows: the ids stay aligned
  const bool compact = pitch != (size_t)m;
  for (int64_t s0 = 0; s0 < nSources; s0 += chunk) {
    const int64_t n = std::min(chunk, nSources - s0);
    // back without the pitch: one contiguous copy of the chunk, then a host compaction of its rows (a 2-D copy of the
    // same 64 x 825 codes took 0.6 ms against 0.08 ms for the whole call this way)
    int8_t* dst = out + (size_t)s0 * (size_t)m;
    if (compact) swapHost_.resize((size_t)n * pitch);
    acceptChunk(
        oCand + (size_t)m * sizeof(int32_t),  // the chunk's sources, then the candidate ids
        [&](char* p) {
          std::memcpy(p, rows + s0, (size_t)n * sizeof(SourceRow));
          std::memcpy(p + oCand, cands, (size_t)m * sizeof(int32_t));
        },
        (size_t)n * pitch,
        [&](hipStream_t st) {
          return launchAcceptSwaps(tables(), prog, (const SourceRow*)dReq_, n, (const int32_t*)(dReq_ + oCand), m, dAccept(),
                                   st);
        },
        compact ? swapHost_.data() : dst, "accept_swaps", "D2H swap codes");
    if (compact)
      for (int64_t i = 0; i < n; ++i) std::memcpy(dst + (size_t)i * (size_t)m, swapHost_.data() + (size_t)i * pitch, (size_t)m);
  }
}

void Device::uploadStatsStatic(const BrokerStatic* meta, int H, const int32_t* hOff, const int32_t* hBrk,
                               const int32_t* hIdx, const int32_t* dBroker) {
  DeviceGuard cur(ordinal_);
  stopServer();
  if (statStatic_) throw std::logic_error("uploadStatsStatic: once per session");
  if (H < 1 || H > B_) throw std::logic_error("uploadStatsStatic: host count");
  statH_ = H;
  DevBuf block;  // becomes statStatic_ once every table is up: statsStaticUploaded()
  carve(block, [&](Carver& c) { layoutStat(c); });
  upload(stat_.hOff, hOff, (size_t)H + 1, "upload stats host offsets");
  upload(stat_.hBrk, hBrk, (size_t)B_, "upload stats host brokers");
  upload(stat_.hIdx, hIdx, (size_t)H, "upload stats host indices");
  if (D_ > 0) upload(stat_.dBroker, dBroker, (size_t)D_, "upload stats disk brokers");
  upload(stat_.meta, meta, (size_t)B_, "upload stats broker columns");
  statStatic_ = std::move(block);
}

void Device::layoutStat(Carver& c) {
  c.take(stat_.hOff, (size_t)statH_ + 1);
  c.take(stat_.hBrk, (size_t)B_);
  c.take(stat_.hIdx, (size_t)statH_);
  c.take(stat_.rows, (size_t)B_ + (size_t)statH_);
  if (D_ > 0) {
    c.take(stat_.dBroker, (size_t)D_);
    c.take(stat_.disks, (size_t)D_);
  }
  c.take(stat_.meta, (size_t)B_);
}

void Device::brokerStats(ccmi_basic_stats* brokers, ccmi_basic_stats* hosts, ccmi_disk_stats* disks,
                         const DiskMember* members, int64_t nMembers, uint64_t memberVer) {
  PlainLaunch call(*this);
  if (!statStatic_) throw std::logic_error("brokerStats before uploadStatsStatic");
  if (!brokers || nMembers < 0) throw std::logic_error("brokerStats: arguments");
  const bool withDisks = disks && D_ > 0;
  const hipStream_t st = (hipStream_t)st_;
  // the rows the host changed since the last launch reach the tables first (prep, on the same stream)
  if (!brows.empty() || !rrows.empty() || !prows.empty() || !tdeltas.empty()) {
    const Staged g = packUpdates(0);
    launchPrepFor(g, 0, false);
  }
  if (withDisks && memberVer != statMemberVer_) {
    DiskMember* dMembers = (DiskMember*)statMembersBuf_.ensure((size_t)nMembers * sizeof(DiskMember));
    if (nMembers)
      hipCheck(hipMemcpyAsync(dMembers, members, (size_t)nMembers * sizeof(DiskMember), hipMemcpyHostToDevice, st),
               "upload disk members");
    statMembers_ = nMembers;
    statMemberVer_ = memberVer;
  }
  ccmi_basic_stats* dHosts = stat_.rows + B_;
  int launches = 1;
  timedLaunch([&] {
    hipCheck(launchBrokerStatsRows(brokers_, stat_.meta, B_, stat_.rows, withDisks ? D_ : 0, dDUtilIn_, dDCap_,
                                   stat_.dBroker, stat_.disks, st),
             "broker_stats_rows");
    if (hosts) {
      hipCheck(launchBrokerStatsHosts(stat_.rows, stat_.hOff, stat_.hBrk, stat_.hIdx, statH_, B_, dHosts, st),
               "broker_stats_hosts");
      launches++;
    }
    if (withDisks && statMembers_ > 0) {
      hipCheck(launchBrokerStatsDisks((const DiskMember*)statMembersBuf_.get(), statMembers_, replicas_, R_, D_,
                                      stat_.disks, st),
               "broker_stats_disks");
      launches++;
    }
  });
  hipCheck(hipMemcpyAsync(brokers, stat_.rows, (size_t)B_ * sizeof(ccmi_basic_stats), hipMemcpyDeviceToHost, st),
           "D2H broker stats");
  if (hosts)
    hipCheck(hipMemcpyAsync(hosts, dHosts, (size_t)statH_ * sizeof(ccmi_basic_stats), hipMemcpyDeviceToHost, st),
             "D2H host stats");
  if (withDisks)
    hipCheck(hipMemcpyAsync(disks, stat_.disks, (size_t)D_ * sizeof(ccmi_disk_stats), hipMemcpyDeviceToHost, st),
             "D2H disk stats");
  streamWait("broker_stats", kAcceptWaitSeconds);
  perf.syncs++;
  // ClusterModelStats' counters take it (a statistics read-back), not the acceptance ones: BrokerRec in, one row out per
  // broker; a row in and out per host; two doubles in and a row out per disk, and a member entry plus the flags word
  perf.statsLaunches += launches;
  perf.statsBytes += (int64_t)B_ * (int64_t)(sizeof(BrokerRec) + sizeof(BrokerStatic) + sizeof(ccmi_basic_stats)) +
                     (hosts ? (int64_t)B_ * (int64_t)sizeof(ccmi_basic_stats) + (int64_t)statH_ * 136 : 0) +
                     (withDisks ? (int64_t)D_ * (16 + 4 + (int64_t)sizeof(ccmi_disk_stats)) + statMembers_ * 12 : 0);
  addKernelMs(perf.statsKernelMs);
}

void Device::uploadPartitionNumbers(const int32_t* pNumber) {
  DeviceGuard cur(ordinal_);
  stopServer();
  if (plStatic_) throw std::logic_error("uploadPartitionNumbers: once per session");
  if (P_ < 1 || !pNumber) throw std::logic_error("uploadPartitionNumbers: arguments");
  DevBuf block;  // the one table [P]
  upload((int32_t*)block.ensure((size_t)P_ * sizeof(int32_t)), pNumber, (size_t)P_, "upload partition numbers");
  plStatic_ = std::move(block);
}

void Device::layoutPl(Carver& c) {
  c.take(pl_.rank, (size_t)P_);
  c.take(pl_.topicSel, (size_t)T_);
  c.take(pl_.brokerSel, (size_t)B_);
  c.take(pl_.buf[0], (size_t)P_);
  c.take(pl_.buf[1], (size_t)P_);
  c.take(pl_.counts, (size_t)256 * (size_t)((P_ + kPlSortTile - 1) / kPlSortTile));
  c.take(pl_.state, 1);
}

// What stageChainCopy does in front of a chain, without a request: the load and slot rows behind the staged row
// updates, sync_loads, then prep for the row updates.
void Device::syncChainLoads() {
  if (!dRLoad_) throw std::runtime_error("device chain state not uploaded");
  const size_t nl = lrows.size(), ns = srows.size();
  const bool rows = !brows.empty() || !rrows.empty() || !prows.empty() || !tdeltas.empty();
  if (!nl && !ns && !rows) return;
  const size_t oS = (nl * sizeof(LoadRow) + 15) & ~(size_t)15;
  const Staged g = packUpdates(oS + ns * sizeof(SlotRow) + 16);
  if (nl) std::memcpy(hStage_ + g.end, lrows.data(), nl * sizeof(LoadRow));
  if (ns) std::memcpy(hStage_ + g.end + oS, srows.data(), ns * sizeof(SlotRow));
  hipCheck(launchSyncLoads(chainTables(), (const LoadRow*)(hStageDev_ + g.end), (int)nl,
                           (const SlotRow*)(hStageDev_ + g.end + oS), (int)ns, (hipStream_t)st_),
           "sync_loads");
  lrows.clear();
  srows.clear();
  launchPrepFor(g, 0, false);
}

void Device::partitionLoad(const PlQuery& q, const uint8_t* topicSel, const uint8_t* brokerSel, const int32_t* tieRank,
                           ccmi_partition_load_record* records, int64_t* numRecords, int64_t* numSelected) {
  PlainLaunch call(*this);
  if (!plStatic_) throw std::logic_error("partitionLoad before uploadPartitionNumbers");
  if (!numRecords || q.entries < 0 || q.resource < 0 || q.resource > 3 || q.mode < 0 || q.mode > 2)
    throw std::logic_error("partitionLoad: arguments");
  const int cap = std::min(q.entries, P_);
  if (cap > 0 && !records) throw std::logic_error("partitionLoad: no room for the records");
  const hipStream_t st = (hipStream_t)st_;
  const int tiles = (P_ + kPlSortTile - 1) / kPlSortTile;
  // first use: the query arrays, the sort buffers, the digit counts, the state
  if (!plWork_) carve(plWork_, [&](Carver& c) { layoutPl(c); });
  ccmi_partition_load_record* dOut =
      (ccmi_partition_load_record*)plOut_.ensure((size_t)cap * sizeof(ccmi_partition_load_record));
  // the device's tables current: the pending row updates (prep) and the pending chain loads (sync_loads)
  syncChainLoads();
  if (topicSel)
    hipCheck(hipMemcpyAsync(pl_.topicSel, topicSel, (size_t)T_, hipMemcpyHostToDevice, st), "upload topic mask");
  if (brokerSel)
    hipCheck(hipMemcpyAsync(pl_.brokerSel, brokerSel, (size_t)B_, hipMemcpyHostToDevice, st), "upload broker mask");
  if (tieRank)
    hipCheck(hipMemcpyAsync(pl_.rank, tieRank, (size_t)P_ * sizeof(int32_t), hipMemcpyHostToDevice, st),
             "upload tie ranks");
  PlTables T;
  T.parts = parts_;
  T.replicas = replicas_;
  T.rLoad = dRLoad_;
  T.pLeader = dPLeader_;
  T.pNumber = (const int32_t*)plStatic_.get();
  T.topicSel = topicSel ? pl_.topicSel : nullptr;
  T.brokerSel = brokerSel ? pl_.brokerSel : nullptr;
  T.tieRank = tieRank ? pl_.rank : nullptr;
  T.B = B_;
  T.R = R_;
  T.P = P_;
  T.T = T_;
  T.W = W_;
  // the most passes the query can need: the left-out flag only under a selection, the rank digits only with ranks
  const bool selects = topicSel || brokerSel || q.lower > INT32_MIN || q.upper < INT32_MAX;
  const int slots = (selects ? 1 : 0) + 8 + (tieRank ? 4 : 0);
  int launches = 0;
  timedLaunch([&] {
    hipCheck(launchPartitionLoad(T, q, pl_.state, pl_.buf[0], pl_.buf[1], pl_.counts, tiles, slots, dOut, cap,
                                 &launches, st),
             "partition_load");
  });
  uint32_t head[2] = {0, 0};  // PlState.nKept, nRecords
  hipCheck(hipMemcpyAsync(head, pl_.state, sizeof(head), hipMemcpyDeviceToHost, st), "D2H partition load counts");
  streamWait("partition_load", kAcceptWaitSeconds);
  perf.syncs++;
  const int64_t nrec = std::min<int64_t>(head[1], cap);
  if (nrec > 0) {
    hipCheck(hipMemcpyAsync(records, dOut, (size_t)nrec * sizeof(ccmi_partition_load_record), hipMemcpyDeviceToHost,
                            st),
             "D2H load records");
    streamWait("partition_load records", kAcceptWaitSeconds);
    perf.syncs++;
  }
  *numRecords = nrec;
  if (numSelected) *numSelected = (int64_t)head[0];
  // a statistics read-back, as brokerStats: per partition its record, leader id, number and LoadVec in and an entry
  // out; per launched pass slot an entry in and out twice at most; per returned record the same reads and a row out
  perf.statsLaunches += launches;
  perf.statsBytes += (int64_t)P_ * (int64_t)(sizeof(PartitionRec) + 8 + sizeof(LoadVec) + sizeof(PlEntry)) +
                     (int64_t)slots * (int64_t)P_ * 3 * (int64_t)sizeof(PlEntry) +
                     nrec * (int64_t)(sizeof(PlEntry) + sizeof(PartitionRec) + sizeof(LoadVec) +
                                      sizeof(ccmi_partition_load_record));
  addKernelMs(perf.statsKernelMs);
}

void Device::uploadInitialPlacement(const int32_t* initDist, const int32_t* initLeaders, const int32_t* initDisks,
                                    const int32_t* initLeaderDisks) {
  DeviceGuard cur(ordinal_);
  stopServer();
  if (pdStatic_) throw std::logic_error("uploadInitialPlacement: once per session");
  if (P_ < 1 || R_ < 1 || !initDist || !initLeaders || (D_ > 0 && (!initDisks || !initLeaderDisks)))
    throw std::logic_error("uploadInitialPlacement: arguments");
  DevBuf block;  // becomes pdStatic_ once every table is up: initialPlacementUploaded()
  carve(block, [&](Carver& c) { layoutPdStatic(c); });
  upload(pdInit_.initLeaders, initLeaders, (size_t)P_, "upload initial leaders");
  if (D_ > 0) {
    upload(pdInit_.initDisks, initDisks, (size_t)R_, "upload initial disks");
    upload(pdInit_.initLeaderDisks, initLeaderDisks, (size_t)P_, "upload initial leader disks");
  }
  upload(pdInit_.initDist, initDist, (size_t)R_, "upload initial placement");
  pdStatic_ = std::move(block);
}

void Device::layoutPdStatic(Carver& c) {
  c.take(pdInit_.initLeaders, (size_t)P_);
  if (D_ > 0) {
    c.take(pdInit_.initDisks, (size_t)R_);
    c.take(pdInit_.initLeaderDisks, (size_t)P_);
  }
  c.take(pdInit_.initDist, (size_t)R_);
}

void Device::layoutPd(Carver& c) {
  c.take(pd_.counts, (size_t)((P_ + kPdTile - 1) / kPdTile) + 1);
  if (D_ > 0) c.take(pd_.curDisks, (size_t)R_);
  c.take(pd_.sums, 1);
}

void Device::proposalDiff(const int32_t* curDisks, ccmi_proposal_record* records, int64_t capacity, int64_t* numRecords,
                          ccmi_proposal_summary* summary) {
  PlainLaunch call(*this);
  if (!pdStatic_) throw std::logic_error("proposalDiff before uploadInitialPlacement");
  if (!numRecords || capacity < 0 || (D_ > 0) != (curDisks != nullptr)) throw std::logic_error("proposalDiff: arguments");
  const int cap = (int)std::min<int64_t>(capacity, P_);
  if (cap > 0 && !records) throw std::logic_error("proposalDiff: no room for the records");
  const hipStream_t st = (hipStream_t)st_;
  const int tiles = (P_ + kPdTile - 1) / kPdTile;
  // first use: the tile counts, the current disks, the sums
  if (!pdWork_) carve(pdWork_, [&](Carver& c) { layoutPd(c); });
  ccmi_proposal_record* dOut = (ccmi_proposal_record*)pdOut_.ensure((size_t)cap * sizeof(ccmi_proposal_record));
  // the device's tables current: the pending row updates (prep) and the pending slot orders and leaders (sync_loads)
  syncChainLoads();
  if (curDisks)
    hipCheck(hipMemcpyAsync(pd_.curDisks, curDisks, (size_t)R_ * sizeof(int32_t), hipMemcpyHostToDevice, st),
             "upload current disks");
  PdTables T;
  T.parts = parts_;
  T.replicas = replicas_;
  T.pOff = dPOff_;
  T.pSlots = dPSlots_;
  T.pLeader = dPLeader_;
  T.initDist = pdInit_.initDist;
  T.initLeaders = pdInit_.initLeaders;
  T.initDisks = curDisks ? pdInit_.initDisks : nullptr;
  T.initLeaderDisks = curDisks ? pdInit_.initLeaderDisks : nullptr;
  T.curDisks = curDisks ? pd_.curDisks : nullptr;
  T.R = R_;
  T.P = P_;
  int launches = 0;
  timedLaunch([&] {
    hipCheck(launchProposalDiff(T, pd_.counts, tiles, pd_.sums, dOut, cap, &launches, st), "proposal_diff");
  });
  static_assert(sizeof(PdSums) == sizeof(ccmi_proposal_summary), "the device sums are the summary");
  ccmi_proposal_summary sum;
  hipCheck(hipMemcpyAsync(&sum, pd_.sums, sizeof(sum), hipMemcpyDeviceToHost, st), "D2H proposal summary");
  streamWait("proposal_diff", kAcceptWaitSeconds);
  perf.syncs++;
  const int64_t nrec = std::min<int64_t>(sum.num_proposals, cap);
  if (nrec > 0) {
    hipCheck(hipMemcpyAsync(records, dOut, (size_t)nrec * sizeof(ccmi_proposal_record), hipMemcpyDeviceToHost, st),
             "D2H proposal records");
    streamWait("proposal_diff records", kAcceptWaitSeconds);
    perf.syncs++;
  }
  *numRecords = nrec;
  if (summary) *summary = sum;
  // a statistics read-back, as brokerStats: per partition and pass (flags, and gather when records are wanted) its
  // record, offsets, leader id, the leader's replica record words, the initial brokers and leader and, with disks, three
  // more words per slot; a count per tile; a row out per returned record
  const int64_t passes = cap > 0 ? 2 : 1;
  const int64_t slotWords = curDisks ? 4 : 1;
  perf.statsLaunches += launches;
  perf.statsBytes += passes * ((int64_t)P_ * (int64_t)(sizeof(PartitionRec) + 8 + 4 + 32 + 4 + (curDisks ? 4 : 0)) +
                               (int64_t)R_ * 4 * slotWords) +
                     (int64_t)tiles * 12 + nrec * (int64_t)sizeof(ccmi_proposal_record);
  addKernelMs(perf.statsKernelMs);
}


void Device::uploadSortedStatic(const int32_t* rStatic) {
  DeviceGuard cur(ordinal_);
  stopServer();
  if (srStatic_) throw std::logic_error("uploadSortedStatic: once per session");
  if (R_ < 1 || B_ < 1 || !rStatic) throw std::logic_error("uploadSortedStatic: arguments");
  DevBuf block;  // becomes srStatic_ once the ranks are up: sortedStaticUploaded()
  carve(block, [&](Carver& c) { layoutSr(c); });
  upload(sr_.rStatic, rStatic, (size_t)R_, "upload static ranks");
  srStatic_ = std::move(block);
}

void Device::layoutSr(Carver& c) {
  c.take(sr_.seg, (size_t)B_);
  c.take(sr_.counts, (size_t)B_);
  c.take(sr_.cursor, (size_t)B_);
  c.take(sr_.state, (size_t)B_ + 3);
  c.take(sr_.topicExcl, (size_t)T_);
  c.take(sr_.topicIncl, (size_t)T_);
  c.take(sr_.keys, (size_t)R_);
  c.take(sr_.segOf, (size_t)R_);
  c.take(sr_.buf, (size_t)R_);
  c.take(sr_.rStatic, (size_t)R_);
}

void Device::sortedReplicas(const SrQuery& q, const int32_t* seg, int n, const uint8_t* topicExcluded,
                            const uint8_t* topicIncluded, int64_t* offsets, ccmi_swap_replica* records, double* scores,
                            int64_t capacity, int64_t* numRecords) {
  PlainLaunch call(*this);
  if (!srStatic_) throw std::logic_error("sortedReplicas before uploadSortedStatic");
  if (!seg || n < 1 || n > B_ || !offsets || !numRecords || capacity < 0)
    throw std::logic_error("sortedReplicas: arguments");
  const hipStream_t st = (hipStream_t)st_;
  // the device's tables current: the pending row updates (prep) and the pending chain loads (sync_loads)
  syncChainLoads();
  hipCheck(hipMemcpyAsync(sr_.seg, seg, (size_t)B_ * sizeof(int32_t), hipMemcpyHostToDevice, st), "upload segment map");
  if (topicExcluded)
    hipCheck(hipMemcpyAsync(sr_.topicExcl, topicExcluded, (size_t)T_, hipMemcpyHostToDevice, st), "upload excluded topics");
  if (topicIncluded)
    hipCheck(hipMemcpyAsync(sr_.topicIncl, topicIncluded, (size_t)T_, hipMemcpyHostToDevice, st), "upload included topics");
  SrTables T;
  T.brokers = brokers_;
  T.replicas = replicas_;
  T.parts = parts_;
  T.rLoad = dRLoad_;
  T.rStatic = sr_.rStatic;
  T.seg = sr_.seg;
  T.topicExcluded = topicExcluded ? sr_.topicExcl : nullptr;
  T.topicIncluded = topicIncluded ? sr_.topicIncl : nullptr;
  T.B = B_;
  T.R = R_;
  T.P = P_;
  T.T = T_;
  T.W = W_;
  int launches = 0;
  timedLaunch([&] {
    hipCheck(launchSortedReplicasCount(T, q, n, sr_.keys, sr_.segOf, sr_.counts, sr_.cursor, sr_.state, &launches, st),
             "sorted_replicas keys");
  });
  // one small read-back: the total, the longest segment and the offsets, which the caller gets whatever the capacity
  srHost_.resize((size_t)n + 3);
  hipCheck(hipMemcpyAsync(srHost_.data(), sr_.state, ((size_t)n + 3) * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                          st),
           "D2H segment offsets");
  streamWait("sorted_replicas keys", kAcceptWaitSeconds);
  perf.syncs++;
  addKernelMs(perf.statsKernelMs);
  const int64_t total = (int64_t)srHost_[0], maxLen = (int64_t)srHost_[1];
  if (total < 0 || total > R_ || maxLen > total) throw std::runtime_error("device sorted_replicas: impossible counts");
  std::memcpy(offsets, srHost_.data() + 2, ((size_t)n + 1) * sizeof(int64_t));
  *numRecords = total;
  // per replica its record, the broker's alive word, the segment, the rank and (with a score) the load's windows in, a
  // key and a segment out
  perf.statsBytes += (int64_t)R_ * (int64_t)(sizeof(ReplicaRec) + 4 + 4 + 4 + (q.scoreRes >= 0 ? 2 * sizeof(Window) : 0) + 12) +
                     (int64_t)n * 24;
  if (total > 0 && total <= capacity) {
    if (!records) throw std::logic_error("sortedReplicas: no room for the records");
    // a segment longer than a tile: the merge passes' second buffer, from then on
    if (maxLen > kSegSortTile) srMerge_.ensure((size_t)R_ * sizeof(SortEntry));
    // records and scores grow together; the gather's whole 16-byte stores stay inside the pieces' rounding
    ccmi_swap_replica* dRecords;
    double* dScores;
    carve(srOut_, [&](Carver& c) {
      c.take(dRecords, (size_t)total);
      c.take(dScores, (size_t)total);
    });
    int fill = 0;
    timedLaunch([&] {
      hipCheck(launchSortedReplicasFill(T, q, n, sr_.keys, sr_.segOf, sr_.cursor, sr_.state, total, maxLen, sr_.buf,
                                        (SortEntry*)srMerge_.get(), dRecords, scores ? dScores : nullptr, &fill, st),
               "sorted_replicas sort");
    });
    hipCheck(hipMemcpyAsync(records, dRecords, (size_t)total * sizeof(ccmi_swap_replica), hipMemcpyDeviceToHost, st),
             "D2H sorted records");
    if (scores)
      hipCheck(hipMemcpyAsync(scores, dScores, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, st),
               "D2H sorted scores");
    streamWait("sorted_replicas sort", kAcceptWaitSeconds);
    perf.syncs++;
    addKernelMs(perf.statsKernelMs);
    launches += fill;
    // per replica a key and a segment in; per entry one write, the sort's read and write, a read and a write per merge
    // pass, the gather's entry and replica words in and a record (and a score) out
    perf.statsBytes += (int64_t)R_ * 12 + total * (int64_t)(sizeof(SortEntry) * (4 + 2 * (fill - 3)) + 16 + 8 + (scores ? 8 : 0));
  }
  perf.statsLaunches += launches;
}

void Device::layoutEp(Carver& c) {
  const size_t tiles = (size_t)((P_ + kPdTile - 1) / kPdTile);
  c.take(ep_.rows, (size_t)P_);
  c.take(ep_.idOf, (size_t)P_);
  c.take(ep_.rank, (size_t)P_);
  c.take(ep_.pstate, (size_t)P_);
  if (D_ > 0) c.take(ep_.curDisks, (size_t)R_);
  c.take(ep_.order, (size_t)B_);
  c.take(ep_.tiles, 2 * (tiles + 1));
  c.take(ep_.counts, 2 * (size_t)B_);
  c.take(ep_.cursors, 2 * (size_t)B_);
  c.take(ep_.state, 2 * ((size_t)B_ + 3) + 4);
  c.take(ep_.sums, 1);
}

void Device::executionPlan(const EpQuery& q, const int32_t* curDisks, const int32_t* rank, const uint8_t* state,
                           ccmi_plan_summary* summary, ccmi_plan_task* tasks, int64_t taskCap, int64_t* interOffsets,
                           int32_t* interEntries, int64_t interCap, int32_t* brokerOrder, int64_t* intraOffsets,
                           int32_t* intraEntries, int64_t intraCap, int32_t* leaderTasks, int64_t leaderCap) {
  PlainLaunch call(*this);
  if (!pdStatic_) throw std::logic_error("executionPlan before uploadInitialPlacement");
  if (!summary || !interOffsets || !intraOffsets || taskCap < 0 || interCap < 0 || intraCap < 0 || leaderCap < 0 ||
      (D_ > 0) != (curDisks != nullptr) || P_ < 1 || B_ < 1)
    throw std::logic_error("executionPlan: arguments");
  const hipStream_t st = (hipStream_t)st_;
  const int tiles = (P_ + kPdTile - 1) / kPdTile;
  const size_t stateWords = 2 * ((size_t)B_ + 3) + 4;
  if (!epWork_) carve(epWork_, [&](Carver& c) { layoutEp(c); });  // first use
  // the device's tables current: the pending row updates (prep) and the pending slot orders and leaders (sync_loads)
  syncChainLoads();
  if (curDisks)
    hipCheck(hipMemcpyAsync(ep_.curDisks, curDisks, (size_t)R_ * sizeof(int32_t), hipMemcpyHostToDevice, st),
             "upload current disks");
  if (rank)
    hipCheck(hipMemcpyAsync(ep_.rank, rank, (size_t)P_ * sizeof(int32_t), hipMemcpyHostToDevice, st),
             "upload proposal ranks");
  if (state)
    hipCheck(hipMemcpyAsync(ep_.pstate, state, (size_t)P_, hipMemcpyHostToDevice, st), "upload partition states");
  EpTables T;
  T.pd.parts = parts_;
  T.pd.replicas = replicas_;
  T.pd.pOff = dPOff_;
  T.pd.pSlots = dPSlots_;
  T.pd.pLeader = dPLeader_;
  T.pd.initDist = pdInit_.initDist;
  T.pd.initLeaders = pdInit_.initLeaders;
  T.pd.initDisks = curDisks ? pdInit_.initDisks : nullptr;
  T.pd.initLeaderDisks = curDisks ? pdInit_.initLeaderDisks : nullptr;
  T.pd.curDisks = curDisks ? ep_.curDisks : nullptr;
  T.pd.R = R_;
  T.pd.P = P_;
  T.rank = rank ? ep_.rank : nullptr;
  T.state = state ? ep_.pstate : nullptr;
  T.B = B_;
  uint32_t* tileInter = ep_.tiles;
  uint32_t* tileLeader = ep_.tiles + tiles + 1;
  int launches = 0;
  timedLaunch([&] {
    hipCheck(launchExecutionPlanCount(T, tiles, ep_.rows, tileInter, tileLeader, ep_.counts, ep_.cursors, ep_.sums,
                                      ep_.state, &launches, st),
             "execution_plan classify");
  });
  // one small read-back: the sums, and both lists' totals, longest segments and offsets, which the caller gets whatever
  // the capacities
  EpSums sums;
  epHost_.resize(stateWords);
  hipCheck(hipMemcpyAsync(&sums, ep_.sums, sizeof(sums), hipMemcpyDeviceToHost, st), "D2H plan sums");
  hipCheck(hipMemcpyAsync(epHost_.data(), ep_.state, stateWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, st),
           "D2H plan offsets");
  streamWait("execution_plan classify", kAcceptWaitSeconds);
  perf.syncs++;
  addKernelMs(perf.statsKernelMs);
  const unsigned long long* hInter = epHost_.data();
  const unsigned long long* hIntra = epHost_.data() + (size_t)B_ + 3;
  const int64_t interTasks = (int64_t)sums.v[0], intraTasks = (int64_t)sums.v[2], leaderAll = (int64_t)sums.v[3];
  const bool dropped = intraTasks > 0;                // maybeDropReplicaSwapTasks
  const bool mingled = dropped && sums.v[5] > 0;      // sanityCheckExecutionTasks throws
  const int64_t interTotal = mingled ? 0 : (int64_t)hInter[0], interMax = mingled ? 0 : (int64_t)hInter[1];
  const int64_t intraTotal = mingled ? 0 : (int64_t)hIntra[0], intraMax = mingled ? 0 : (int64_t)hIntra[1];
  const int64_t numTasks = dropped ? 0 : interTasks, numLeader = mingled ? 0 : leaderAll;
  if (interTasks > P_ || leaderAll > P_ || (int64_t)hIntra[0] != intraTasks || interMax > interTotal ||
      intraMax > intraTotal || interTotal > 9 * (int64_t)P_ || intraTotal > (int64_t)R_ ||
      hInter[0] != (dropped ? 0ull : sums.v[1]))
    throw std::runtime_error("device execution_plan: impossible counts");
  int64_t withTasks = 0;
  for (int b = 0; b <= B_; ++b) {
    interOffsets[b] = mingled ? 0 : (int64_t)hInter[2 + b];
    intraOffsets[b] = mingled ? 0 : (int64_t)hIntra[2 + b];
    if (b > 0 && interOffsets[b] > interOffsets[b - 1]) withTasks++;
  }
  *summary = ccmi_plan_summary{};
  summary->num_inter_tasks = interTasks;
  summary->num_inter_entries = interTotal;
  summary->num_intra_tasks = intraTasks;
  summary->num_leader_tasks = leaderAll;
  summary->num_brokers_with_tasks = withTasks;
  summary->size_overflow = sums.v[4] > 0 ? 1 : 0;
  summary->mingled = mingled ? 1 : 0;
  // per partition its record, offsets, leader id, the leader's replica record words, the initial brokers and leader (and
  // the disks), a row out; per broker two counts, two cursors and two offsets
  perf.statsBytes += (int64_t)P_ * (int64_t)(sizeof(PartitionRec) + 8 + 4 + 32 + 4 + (curDisks ? 4 : 0) + sizeof(EpRow)) +
                     (int64_t)R_ * 4 * (curDisks ? 4 : 1) + (int64_t)tiles * 16 + (int64_t)B_ * 32;
  const int64_t entries = numTasks + numLeader + interTotal + intraTotal;
  const bool fits = numTasks <= taskCap && interTotal <= interCap && intraTotal <= intraCap && numLeader <= leaderCap;
  if (entries > 0 && fits) {
    if ((numTasks > 0 && !tasks) || (interTotal > 0 && (!interEntries || !brokerOrder)) ||
        (intraTotal > 0 && !intraEntries) || (numLeader > 0 && !leaderTasks))
      throw std::logic_error("executionPlan: no room for the lists");
    // the gathers finish a list with whole 16-byte stores: a DevBuf's capacity is whole 256-byte runs
    SortEntry* buf[2];  // both buffers in one block: a merge pass may come with any call
    carve(epEntries_, [&](Carver& c) {
      c.take(buf[0], (size_t)entries);
      c.take(buf[1], (size_t)entries);
    });
    ccmi_plan_task* dTasks = (ccmi_plan_task*)epTasks_.ensure((size_t)numTasks * sizeof(ccmi_plan_task));
    int32_t* dInter = (int32_t*)epInter_.ensure((size_t)interTotal * sizeof(int32_t));
    int32_t* dIntra = (int32_t*)epIntra_.ensure((size_t)intraTotal * sizeof(int32_t));
    int32_t* dLeader = (int32_t*)epLeader_.ensure((size_t)numLeader * sizeof(int32_t));
    int fill = 0;
    timedLaunch([&] {
      hipCheck(launchExecutionPlanFill(T, q, tiles, ep_.rows, tileInter, tileLeader, ep_.cursors, ep_.state, numTasks,
                                       numLeader, interTotal, interMax, intraTotal, intraMax, buf[0], buf[1],
                                       ep_.idOf, dTasks, dInter, ep_.order, dIntra, dLeader, &fill,
                                       st),
               "execution_plan fill");
    });
    auto back = [&](void* h, const void* d, size_t bytes, const char* what) {
      if (bytes) hipCheck(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, st), what);
    };
    back(tasks, dTasks, (size_t)numTasks * sizeof(ccmi_plan_task), "D2H plan tasks");
    back(interEntries, dInter, (size_t)interTotal * sizeof(int32_t), "D2H plan inter entries");
    if (interTotal > 0) back(brokerOrder, ep_.order, (size_t)B_ * sizeof(int32_t), "D2H broker order");
    back(intraEntries, dIntra, (size_t)intraTotal * sizeof(int32_t), "D2H plan intra entries");
    back(leaderTasks, dLeader, (size_t)numLeader * sizeof(int32_t), "D2H plan leader tasks");
    streamWait("execution_plan fill", kAcceptWaitSeconds);
    perf.syncs++;
    addKernelMs(perf.statsKernelMs);
    launches += fill;
    // per partition a row in (number, scatter); per task partition the proposal's tables again; per entry a write, the
    // sorts' and merge passes' reads and writes, the gather's read and a word out
    perf.statsBytes += (int64_t)P_ * 2 * (int64_t)sizeof(EpRow) +
                       (numTasks + intraTotal) * (int64_t)(sizeof(PartitionRec) + 64) +
                       entries * (int64_t)(sizeof(SortEntry) * (4 + 2 * std::max(0, fill - 8)) + 4) +
                       numTasks * (int64_t)sizeof(ccmi_plan_task);
  }
  if (interTotal == 0 && fits && brokerOrder)  // no broker has tasks: the whole order is "none"
    std::fill(brokerOrder, brokerOrder + B_, -1);
  perf.statsLaunches += launches;
}

}  // namespace ccmi
