// The launchers of K17 (kernels/aggregator.hip) as the host side of ccmi_aggregator (ccmi_aggregator.cpp) calls them.
// Every function only enqueues on `st`; the caller synchronises and reads back. Product only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "devtypes.h"

namespace ccmi {

// The options of one completeness walk as the kernels take them.
struct AggWalkOptions {
  double minEntityRatio, minGroupRatio;
  int32_t maxExtrapolations, groupGranularity;
};

// add_samples: group the accepted samples by entity (runOff[E + 1] and cursor[E] are scratch, order[n] receives the
// batch positions grouped by entity), then replay the batch per entity.
void aggLaunchAddSamples(const AggTables& T, const int32_t* entity, const int64_t* timeMs, const double* values,
                         const uint8_t* accepted, int64_t n, const AggRollEvent* events, int numEvents,
                         long long startOldest, long long windowMs, uint32_t* runOff, uint32_t* cursor, uint32_t* order,
                         hipStream_t st);
// The walk over the windows first, first - 1, .., first - numWindows + 1 (window indices); mask may be null.
void aggLaunchWalk(const AggTables& T, const AggWalk& W, const uint8_t* mask, long long firstWindow, int numWindows,
                   const AggWalkOptions& o, hipStream_t st);
// cover[e] = W.inter[e] (source 0), W.validE[e] (1) or T.present[e] (2); counts the covered entities into
// W.ctr[kAcCovered] and, per tile, into tileOff[tiles + 1] (scanned in place).
void aggLaunchCover(const AggTables& T, const AggWalk& W, int source, uint32_t* tileOff, hipStream_t st);
// The rows of the covered entities whose rank is below capacity: windows[numWindows] are window indices, newest first.
void aggLaunchRows(const AggTables& T, const AggWalk& W, int source, const uint32_t* tileOff, const long long* windows,
                   int numWindows, long long oldest, int maxExtrapolations, int64_t capacity, int32_t* entities,
                   float* values, uint8_t* extrapolations, uint8_t* invalid, hipStream_t st);
// sums[0] = samples in the kept windows, sums[1] = present entities (sums is cleared here)
void aggLaunchStateSums(const AggTables& T, unsigned long long* sums, hipStream_t st);
// clears the state of ids[n] that are present; *removed becomes nonzero if any was (removed is cleared here)
void aggLaunchRemove(const AggTables& T, const int32_t* ids, int64_t n, uint32_t* removed, hipStream_t st);

}  // namespace ccmi
