// Device::acceptBatch, Device::maskBatch and Device::swapGridBatch (device.h): the launchers of K9 accept_actions
// (kernels/accept.hip), K10 accept_mask (kernels/accept_mask.hip) and K11 accept_swaps (kernels/accept_swap.hip). A
// translation unit of its own, linked into libccmi.so only: the test emulation of Device has no acceptance kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>

#include "device.h"
#include "prof.h"

namespace ccmi {

hipError_t launchAcceptActions(const DevTables& T, const DevProgram& prog, const AcceptRow* rows, int64_t nRows,
                               int8_t* out, hipStream_t st);
hipError_t launchAcceptMask(const DevTables& T, const DevProgram& prog, const MaskRow* rows, int64_t nSources,
                            unsigned long long* out, hipStream_t st);
hipError_t launchAcceptSwaps(const DevTables& T, const DevProgram& prog, const SwapRow* rows, int64_t nSources,
                             const int32_t* cands, int64_t m, int8_t* out, hipStream_t st);

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

}  // namespace ccmi
