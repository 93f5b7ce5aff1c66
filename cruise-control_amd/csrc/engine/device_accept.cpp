// Device::acceptBatch, Device::maskBatch and Device::swapGridBatch (device.h): the launchers of K9 accept_actions
// (kernels/accept.hip), K10 accept_mask (kernels/accept_mask.hip) and K11 accept_swaps (kernels/accept_swap.hip); and
// Device::brokerStats, the launcher of K12 (kernels/broker_stats.hip), which shares their launch protocol. A translation
// unit of its own, linked into libccmi.so only: the test emulation of Device has none of these kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>

#include "ccmi.h"
#include "device.h"
#include "prof.h"

namespace ccmi {

hipError_t launchAcceptActions(const DevTables& T, const DevProgram& prog, const AcceptRow* rows, int64_t nRows,
                               int8_t* out, hipStream_t st);
hipError_t launchAcceptMask(const DevTables& T, const DevProgram& prog, const MaskRow* rows, int64_t nSources,
                            unsigned long long* out, hipStream_t st);
hipError_t launchAcceptSwaps(const DevTables& T, const DevProgram& prog, const SwapRow* rows, int64_t nSources,
                             const int32_t* cands, int64_t m, int8_t* out, hipStream_t st);
hipError_t launchBrokerStatsRows(const BrokerRec* brokers, const BrokerStatic* meta, int B, ccmi_basic_stats* out, int D,
                                 const double* dUtil, const double* dCap, const int32_t* dBroker,
                                 ccmi_disk_stats* diskOut, hipStream_t st);
hipError_t launchBrokerStatsHosts(const ccmi_basic_stats* rows, const int32_t* hOff, const int32_t* hBrk,
                                  const int32_t* hIdx, int H, int B, ccmi_basic_stats* out, hipStream_t st);
hipError_t launchBrokerStatsDisks(const DiskMember* members, int64_t E, const ReplicaRec* replicas, int R, int D,
                                  ccmi_disk_stats* diskOut, hipStream_t st);

namespace {
void hipCheck(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string("HIP error in ") + what + ": " + hipGetErrorString(e));
}
// the session's device current for the call (HIP's current device is per host thread), the caller's afterwards
struct CurrentDevice {
  int prev = -1;
  explicit CurrentDevice(int ordinal) {
    hipCheck(hipGetDevice(&prev), "hipGetDevice");
    if (prev != ordinal) hipCheck(hipSetDevice(ordinal), "hipSetDevice");
    else prev = -1;
  }
  ~CurrentDevice() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};
constexpr double kAcceptWaitSeconds = 120.0;
}  // namespace

// the output buffer of one chunk, grown to the largest chunk so far
void Device::ensureAccept(size_t bytes) {
  if (bytes <= acceptCap_) return;
  if (dAccept_) hipCheck(hipFree(dAccept_), "hipFree");
  dAccept_ = nullptr;
  acceptCap_ = 0;
  hipCheck(hipMalloc((void**)&dAccept_, bytes), "hipMalloc acceptance");
  acceptCap_ = bytes;
}

void Device::acceptBatch(const DevProgram& prog, const AcceptRow* rows, int64_t nRows, int64_t nMoveRows, int8_t* out) {
  CurrentDevice cur(ordinal_);
  PhaseScope ps(PH_DEV_SCAN);
  stopServer();  // a plain launch on the session stream (no server is resident between API calls anyway)
  if (nRows % 64 != 0 || nMoveRows % 64 != 0 || nMoveRows < 0 || nMoveRows > nRows)
    throw std::logic_error("acceptBatch takes whole wavefronts of each row kind");
  if (prog.nGoals < 1 || prog.nGoals > kMaxGoals) throw std::logic_error("acceptBatch: goal count");
  if (nRows == 0) {
    flushPending();
    return;
  }
  const size_t G = (size_t)prog.nGoals;
  const int64_t chunk = acceptChunkRows_;  // a multiple of 64, so a chunk boundary never splits a wavefront
  const hipStream_t st = (hipStream_t)st_;
  for (int64_t r0 = 0; r0 < nRows; r0 += chunk) {
    const int64_t n = std::min(chunk, nRows - r0);
    // the chunk's rows go into HBM with the pending row updates (prep; the first chunk carries them all)
    const size_t req = (size_t)n * sizeof(AcceptRow);
    const Staged g = packUpdates(req);
    std::memcpy(hStage_ + g.end, rows + r0, req);
    launchPrepFor(g, req, false);
    ensureAccept((size_t)n * G);
    if (timing) (void)hipEventRecord((hipEvent_t)ev0_, st);
    hipCheck(launchAcceptActions(tables(), prog, (const AcceptRow*)dReq_, n, dAccept_, st), "accept_actions");
    if (timing) (void)hipEventRecord((hipEvent_t)ev1_, st);
    hipCheck(hipMemcpyAsync(out + (size_t)r0 * G, dAccept_, (size_t)n * G, hipMemcpyDeviceToHost, st), "D2H acceptance");
    streamWait("accept_actions", kAcceptWaitSeconds);
    perf.syncs++;
    perf.acceptLaunches++;  // acceptCells is the caller's count: it knows which rows are padding
    if (timing) {
      float ms = 0.f;
      hipCheck(hipEventElapsedTime(&ms, (hipEvent_t)ev0_, (hipEvent_t)ev1_), "hipEventElapsedTime");
      perf.acceptKernelMs += ms;
    }
  }
}

void Device::maskBatch(const DevProgram& prog, const MaskRow* rows, int64_t nSources, uint64_t* out) {
  CurrentDevice cur(ordinal_);
  PhaseScope ps(PH_DEV_SCAN);
  stopServer();  // a plain launch on the session stream, as acceptBatch
  if (nSources < 0 || prog.nGoals < 0 || prog.nGoals > kMaxGoals) throw std::logic_error("maskBatch: counts");
  if (nSources == 0) {
    flushPending();
    return;
  }
  const size_t W = (size_t)maskWords();
  const int64_t chunk = maskChunkSources_;
  const hipStream_t st = (hipStream_t)st_;
  for (int64_t s0 = 0; s0 < nSources; s0 += chunk) {
    const int64_t n = std::min(chunk, nSources - s0);
    // the chunk's sources go into HBM with the pending row updates (prep; the first chunk carries them all)
    const size_t req = (size_t)n * sizeof(MaskRow);
    const Staged g = packUpdates(req);
    std::memcpy(hStage_ + g.end, rows + s0, req);
    launchPrepFor(g, req, false);
    const size_t bytes = (size_t)n * W * sizeof(uint64_t);
    ensureAccept(bytes);
    if (timing) (void)hipEventRecord((hipEvent_t)ev0_, st);
    hipCheck(launchAcceptMask(tables(), prog, (const MaskRow*)dReq_, n, (unsigned long long*)dAccept_, st), "accept_mask");
    if (timing) (void)hipEventRecord((hipEvent_t)ev1_, st);
    hipCheck(hipMemcpyAsync(out + (size_t)s0 * W, dAccept_, bytes, hipMemcpyDeviceToHost, st), "D2H masks");
    streamWait("accept_mask", kAcceptWaitSeconds);
    perf.syncs++;
    perf.acceptLaunches++;  // acceptCells is the caller's count
    if (timing) {
      float ms = 0.f;
      hipCheck(hipEventElapsedTime(&ms, (hipEvent_t)ev0_, (hipEvent_t)ev1_), "hipEventElapsedTime");
      perf.acceptKernelMs += ms;
    }
  }
}

void Device::swapGridBatch(const DevProgram& prog, const SwapRow* rows, int64_t nSources, const int32_t* cands, int64_t m,
                           int8_t* out) {
  CurrentDevice cur(ordinal_);
  PhaseScope ps(PH_DEV_SCAN);
  stopServer();  // a plain launch on the session stream, as acceptBatch
  if (nSources < 0 || m < 0 || prog.nGoals < 0 || prog.nGoals > kMaxGoals) throw std::logic_error("swapGridBatch: counts");
  if (m > kMaxSwapCandidates)
    throw std::invalid_argument("a swap grid takes at most " + std::to_string(kMaxSwapCandidates) + " candidates");
  if (nSources == 0 || m == 0) {
    flushPending();
    return;
  }
  // a row of the device buffer is whole wavefronts: a wave's 64 codes are one aligned 64-byte run
  const size_t pitch = (size_t)((m + 63) / 64 * 64);
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(65535, swapChunkCells_ / (int64_t)pitch));
  const size_t oCand = (size_t)std::min(chunk, nSources) * sizeof(SwapRow);  // 16-byte rows: the ids stay aligned
  const hipStream_t st = (hipStream_t)st_;
  for (int64_t s0 = 0; s0 < nSources; s0 += chunk) {
    const int64_t n = std::min(chunk, nSources - s0);
    // the chunk's sources and the candidate ids go into HBM with the pending row updates (prep; the first chunk
    // carries them all)
    const size_t req = oCand + (size_t)m * sizeof(int32_t);
    const Staged g = packUpdates(req);
    std::memcpy(hStage_ + g.end, rows + s0, (size_t)n * sizeof(SwapRow));
    std::memcpy(hStage_ + g.end + oCand, cands, (size_t)m * sizeof(int32_t));
    launchPrepFor(g, req, false);
    ensureAccept((size_t)n * pitch);
    if (timing) (void)hipEventRecord((hipEvent_t)ev0_, st);
    hipCheck(launchAcceptSwaps(tables(), prog, (const SwapRow*)dReq_, n, (const int32_t*)(dReq_ + oCand), m, dAccept_, st),
             "accept_swaps");
    if (timing) (void)hipEventRecord((hipEvent_t)ev1_, st);
    // back without the pitch: one contiguous copy of the chunk, then a host compaction of its rows (a 2-D copy of the
    // same 64 x 825 codes took 0.6 ms against 0.08 ms for the whole call this way)
    int8_t* dst = out + (size_t)s0 * (size_t)m;
    const bool compact = pitch != (size_t)m;
    if (compact) swapHost_.resize((size_t)n * pitch);
    hipCheck(hipMemcpyAsync(compact ? swapHost_.data() : dst, dAccept_, (size_t)n * pitch, hipMemcpyDeviceToHost, st),
             "D2H swap codes");
    streamWait("accept_swaps", kAcceptWaitSeconds);
    if (compact)
      for (int64_t i = 0; i < n; ++i) std::memcpy(dst + (size_t)i * (size_t)m, swapHost_.data() + (size_t)i * pitch, (size_t)m);
    perf.syncs++;
    perf.acceptLaunches++;  // acceptCells is the caller's count
    if (timing) {
      float ms = 0.f;
      hipCheck(hipEventElapsedTime(&ms, (hipEvent_t)ev0_, (hipEvent_t)ev1_), "hipEventElapsedTime");
      perf.acceptKernelMs += ms;
    }
  }
}

void Device::uploadStatsStatic(const BrokerStatic* meta, int H, const int32_t* hOff, const int32_t* hBrk,
                               const int32_t* hIdx, const int32_t* dBroker) {
  CurrentDevice cur(ordinal_);
  stopServer();
  if (dStatMeta_) throw std::logic_error("uploadStatsStatic: once per session");
  if (H < 1 || H > B_) throw std::logic_error("uploadStatsStatic: host count");
  auto put = [&](auto** d, const auto* h, size_t n, const char* what) {
    hipCheck(hipMalloc((void**)d, std::max<size_t>(1, n) * sizeof(**d)), what);
    statsRowAllocs_.push_back(*d);
    if (h && n) hipCheck(hipMemcpy(*d, h, n * sizeof(**d), hipMemcpyHostToDevice), what);
  };
  put(&dStatHOff_, hOff, (size_t)H + 1, "upload stats host offsets");
  put(&dStatHBrk_, hBrk, (size_t)B_, "upload stats host brokers");
  put(&dStatHIdx_, hIdx, (size_t)H, "upload stats host indices");
  put(&dStatRows_, (const ccmi_basic_stats*)nullptr, (size_t)B_ + (size_t)H, "hipMalloc stats rows");
  if (D_ > 0) {
    put(&dStatDBroker_, dBroker, (size_t)D_, "upload stats disk brokers");
    put(&dStatDisks_, (const ccmi_disk_stats*)nullptr, (size_t)D_, "hipMalloc disk stats rows");
  }
  statH_ = H;
  put(&dStatMeta_, meta, (size_t)B_, "upload stats broker columns");  // last: statsStaticUploaded()
}

void Device::brokerStats(ccmi_basic_stats* brokers, ccmi_basic_stats* hosts, ccmi_disk_stats* disks,
                         const DiskMember* members, int64_t nMembers, uint64_t memberVer) {
  CurrentDevice cur(ordinal_);
  PhaseScope ps(PH_DEV_SCAN);
  stopServer();  // plain launches on the session stream, as maskBatch
  if (!dStatMeta_) throw std::logic_error("brokerStats before uploadStatsStatic");
  if (!brokers || nMembers < 0) throw std::logic_error("brokerStats: arguments");
  const bool withDisks = disks && D_ > 0;
  const hipStream_t st = (hipStream_t)st_;
  // the rows the host changed since the last launch reach the tables first (prep, on the same stream)
  if (!brows.empty() || !rrows.empty() || !prows.empty() || !tdeltas.empty()) {
    const Staged g = packUpdates(0);
    launchPrepFor(g, 0, false);
  }
  if (withDisks && memberVer != statMemberVer_) {
    if ((size_t)nMembers > statMembersCap_) {
      if (dStatMembers_) hipCheck(hipFree(dStatMembers_), "hipFree");
      dStatMembers_ = nullptr;
      statMembersCap_ = 0;
      hipCheck(hipMalloc((void**)&dStatMembers_, (size_t)nMembers * sizeof(DiskMember)), "hipMalloc disk members");
      statMembersCap_ = (size_t)nMembers;
    }
    if (nMembers)
      hipCheck(hipMemcpyAsync(dStatMembers_, members, (size_t)nMembers * sizeof(DiskMember), hipMemcpyHostToDevice, st),
               "upload disk members");
    statMembers_ = nMembers;
    statMemberVer_ = memberVer;
  }
  ccmi_basic_stats* dHosts = dStatRows_ + B_;
  if (timing) (void)hipEventRecord((hipEvent_t)ev0_, st);
  hipCheck(launchBrokerStatsRows(brokers_, dStatMeta_, B_, dStatRows_, withDisks ? D_ : 0, dDUtilIn_, dDCap_, dStatDBroker_,
                                 dStatDisks_, st),
           "broker_stats_rows");
  int launches = 1;
  if (hosts) {
    hipCheck(launchBrokerStatsHosts(dStatRows_, dStatHOff_, dStatHBrk_, dStatHIdx_, statH_, B_, dHosts, st),
             "broker_stats_hosts");
    launches++;
  }
  if (withDisks && statMembers_ > 0) {
    hipCheck(launchBrokerStatsDisks(dStatMembers_, statMembers_, replicas_, R_, D_, dStatDisks_, st), "broker_stats_disks");
    launches++;
  }
  if (timing) (void)hipEventRecord((hipEvent_t)ev1_, st);
  hipCheck(hipMemcpyAsync(brokers, dStatRows_, (size_t)B_ * sizeof(ccmi_basic_stats), hipMemcpyDeviceToHost, st),
           "D2H broker stats");
  if (hosts)
    hipCheck(hipMemcpyAsync(hosts, dHosts, (size_t)statH_ * sizeof(ccmi_basic_stats), hipMemcpyDeviceToHost, st),
             "D2H host stats");
  if (withDisks)
    hipCheck(hipMemcpyAsync(disks, dStatDisks_, (size_t)D_ * sizeof(ccmi_disk_stats), hipMemcpyDeviceToHost, st),
             "D2H disk stats");
  streamWait("broker_stats", kAcceptWaitSeconds);
  perf.syncs++;
  // ClusterModelStats' counters take it (a statistics read-back), not the acceptance ones: BrokerRec in, one row out per
  // broker; a row in and out per host; two doubles in and a row out per disk, and a member entry plus the flags word
  perf.statsLaunches += launches;
  perf.statsBytes += (int64_t)B_ * (int64_t)(sizeof(BrokerRec) + sizeof(BrokerStatic) + sizeof(ccmi_basic_stats)) +
                     (hosts ? (int64_t)B_ * (int64_t)sizeof(ccmi_basic_stats) + (int64_t)statH_ * 136 : 0) +
                     (withDisks ? (int64_t)D_ * (16 + 4 + (int64_t)sizeof(ccmi_disk_stats)) + statMembers_ * 12 : 0);
  if (timing) {
    float ms = 0.f;
    hipCheck(hipEventElapsedTime(&ms, (hipEvent_t)ev0_, (hipEvent_t)ev1_), "hipEventElapsedTime");
    perf.statsKernelMs += ms;
  }
}

}  // namespace ccmi
