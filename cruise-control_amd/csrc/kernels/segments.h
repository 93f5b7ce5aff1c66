// The segment toolkit of the list kernels (K13..K16), each piece written once: the inline device functions, and the
// segmented sort of K15 and K16 as kernels templated on the feature's comparator. A "segment" is a consecutive run of
// SortEntry in a buffer, bounded by offsets[i] .. offsets[i + 1]; a segment block {total, longest, offsets[n + 1]} is
// what the host reads back.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../engine/devtypes.h"

namespace ccmi {

// the 64-lane sum of a 64-bit value, in every lane
__device__ __forceinline__ unsigned long long waveSum(unsigned long long v) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v += (unsigned long long)__shfl_xor((long long)v, s, 64);
  return v;
}

// The lanes of a wave with `active` set add one each to counters[seg]: one atomic per distinct segment in the wave.
// Returns the lane's slot among the counter's arrivals. EVERY lane of the wave must make the call (it ballots and
// shuffles): the caller's loop is wave-uniform and an idle lane passes active = false.
__device__ __forceinline__ uint32_t waveSegAdd(uint32_t* __restrict__ counters, int seg, bool active) {
  const int lane = (int)(threadIdx.x & 63);
  const unsigned long long below = (1ull << lane) - 1ull;
  unsigned long long todo = __ballot(active);
  uint32_t slot = 0;
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int s = __shfl(seg, leader, 64);
    const bool mine = active && seg == s;
    const unsigned long long m = __ballot(mine);
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(&counters[s], (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, leader, 64);
    if (mine) slot = base + (uint32_t)__popcll(m & below);
    todo &= ~m;
  }
  return slot;
}

// the segment of entry k: the last i with offsets[i] <= k (empty segments repeat an offset and are skipped)
__device__ __forceinline__ int segmentOf(const unsigned long long* __restrict__ offsets, int n, long long k) {
  int lo = 0, hi = n;  // invariant: offsets[lo] <= k < offsets[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((long long)offsets[mid] <= k)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// the merge passes a segment of length len takes: the number of widths kSegSortTile << i below len. The sorted segment
// ends in buffer (segSortPasses(len) & 1): 0 = the buffer it was scattered into, 1 = the other one.
__host__ __device__ __forceinline__ int segSortPasses(long long len) {
  int p = 0;
  for (long long w = kSegSortTile; w < len; w <<= 1) p++;
  return p;
}

// Exclusive scan over the kBlock threads of a workgroup (Hillis-Steele, ping-pong in LDS). `sum` is the thread's own
// value, usually the sum of a contiguous chunk it read; returns the sum of the threads before it, and *total gets the
// workgroup's sum in every thread. Every thread calls it, once per kernel: the first barrier comes after the thread's
// store, the last one before the reads, and a second call would need a barrier of its own before it reuses the LDS.
template <typename T, int kBlock>
__device__ __forceinline__ T blockExclusiveScan(T sum, T* total) {
  __shared__ T s[2][kBlock];
  int cur = 0;
  s[0][threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < kBlock; d <<= 1) {
    const T v = s[cur][threadIdx.x] + ((int)threadIdx.x >= d ? s[cur][threadIdx.x - d] : (T)0);
    s[cur ^ 1][threadIdx.x] = v;
    cur ^= 1;
    __syncthreads();
  }
  *total = s[cur][kBlock - 1];
  return s[cur][threadIdx.x] - sum;
}

// Exclusive scan of counts[0, n) in place by one workgroup of kBlock, summed as T; returns the total in every thread. A
// thread sums a contiguous chunk (so n may exceed the block), the chunk sums are scanned, the thread writes its chunk's
// prefixes.
template <typename T, int kBlock>
__device__ __forceinline__ T scanCountsInPlace(uint32_t* __restrict__ counts, int n) {
  const int chunk = (n + kBlock - 1) / kBlock;
  const int i0 = min(n, (int)threadIdx.x * chunk), i1 = min(n, i0 + chunk);
  T sum = 0, total;
  for (int i = i0; i < i1; ++i) sum += counts[i];
  T run = blockExclusiveScan<T, kBlock>(sum, &total);
  for (int i = i0; i < i1; ++i) {
    const uint32_t c = counts[i];
    counts[i] = (uint32_t)run;
    run += c;
  }
  return total;
}

// One workgroup of kBlock turns the n per-segment counts into a segment block: state[0] = the total, state[1] = the
// longest segment, state[2 + i] = offsets[i] for i <= n; cursor[0, n) is cleared for the scatter that follows. A thread
// takes a contiguous chunk, so n may exceed the block. With `zero` every count reads as 0 (an emptied list).
// mx is cleared before the first barrier and every atomicMax comes before the scan's barriers, so thread 0 reads the
// finished maximum after them.
template <int kBlock>
__device__ __forceinline__ void segmentOffsets(const uint32_t* __restrict__ counts, int n, bool zero,
                                               unsigned long long* __restrict__ state,
                                               uint32_t* __restrict__ cursor) {
  __shared__ uint32_t mx;
  if (threadIdx.x == 0) mx = 0;
  const int chunk = (n + kBlock - 1) / kBlock;
  const int i0 = min(n, (int)threadIdx.x * chunk), i1 = min(n, i0 + chunk);
  unsigned long long sum = 0, total;
  uint32_t longest = 0;
  for (int i = i0; i < i1; ++i) {
    const uint32_t c = zero ? 0u : counts[i];
    sum += c;
    longest = c > longest ? c : longest;
    cursor[i] = 0;
  }
  __syncthreads();
  if (longest) atomicMax(&mx, longest);
  unsigned long long run = blockExclusiveScan<unsigned long long, kBlock>(sum, &total);
  for (int i = i0; i < i1; ++i) {
    state[2 + i] = run;
    run += zero ? 0u : counts[i];
  }
  if (threadIdx.x == 0) {
    state[0] = total;
    state[1] = mx;
    state[2 + n] = total;
  }
}

// The segmented sort: n segments of SortEntry, bounded by offsets[n + 1], each sorted ascending where it lies. Less is
// the feature's comparator, a type with `static __device__ bool less(const uint4& a, const uint4& b)` on entries as the
// sort moves them (x, y = lo; z, w = hi): a strict order in which the all-ones entry comes last and no two entries of a
// segment compare equal, so a rank needs no tie-break. A comparator that leaves a word unread spares the LDS that read.
//     segsort_tiles : one workgroup per segment. A segment of up to kSegSortTile entries is loaded into LDS with
//                     16-byte accesses, padded to its next power of two with all-ones entries (not written back),
//                     sorted by a bitonic network of that width (a 100-entry segment runs the 128-wide network, not
//                     the tile's) and written back. When the call's longest segment is at most kSegSmallTile entries
//                     the launcher takes the instance with a 4 KB image and kSegSmallBlock lanes, so the common case
//                     does not reserve the tile's 64 KB per workgroup. A longer segment is sorted tile by tile here
//                     and finished by
//     segsort_merge : global-memory merge passes over the sorted tiles, run width doubling per launch, ping-pong
//                     between two entry buffers. One lane per entry finds its rank in the sibling run by binary search.
//                     Chosen over radix passes because the tiles come sorted out of the LDS network anyway, segment
//                     boundaries stay where they are (a radix pass over the whole array would need per-segment
//                     histograms), and the host launches it only when the longest segment it read back asks for it:
//                     the common case pays nothing. Pass i reads buffer (i & 1) and writes the other; a segment no
//                     longer than the pass's run width is skipped, so a segment of length len ends in buffer
//                     (segSortPasses(len) & 1).
// Every launch is a kernel boundary on the caller's stream; no workgroup reads another's writes inside a launch.
constexpr int kSegBlock = 256;
constexpr int kSegMaxBlocks = 1024;
constexpr int kSegSmallTile = 256;   // the LDS image of a call whose longest segment fits it: 4 KB
constexpr int kSegSmallBlock = 128;  // and its workgroup: one compare-exchange per lane at the full width
static_assert((kSegSortTile & (kSegSortTile - 1)) == 0 && kSegSortTile * sizeof(SortEntry) <= 64 * 1024, "tile shape");
static_assert((kSegSmallTile & (kSegSmallTile - 1)) == 0 && kSegSmallTile <= kSegSortTile, "small tile shape");

// kLds: the entries of the workgroup's LDS image. The launcher picks kSegSmallTile when the longest segment of the
// call fits it (more workgroups per CU), else the whole tile; a longer segment's tile stride is kSegSortTile either way.
template <class Less, int kLds>
__global__ __launch_bounds__(kSegBlock) void segsort_tiles(const unsigned long long* __restrict__ offsets,
                                                           SortEntry* __restrict__ entries) {
  __shared__ uint4 tile[kLds];
  const unsigned long long off0 = offsets[blockIdx.x];
  const long long len = (long long)(offsets[blockIdx.x + 1] - off0);
  if (len < 2) return;
  for (long long t0 = 0; t0 < len; t0 += kSegSortTile) {  // one tile unless the segment is longer than a tile
    const int m = (int)min((long long)kSegSortTile, len - t0);
    if (m > kLds) return;  // not reachable: the launcher chose kLds from the longest segment
    uint4* seg = reinterpret_cast<uint4*>(entries + off0 + t0);
    int width = 2;
    while (width < m) width <<= 1;
    for (int i = (int)threadIdx.x; i < width; i += (int)blockDim.x)
      tile[i] = i < m ? seg[i] : make_uint4(~0u, ~0u, ~0u, ~0u);
    __syncthreads();
    const int half = width >> 1;
    for (int k = 2; k <= width; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int t = (int)threadIdx.x; t < half; t += (int)blockDim.x) {
          const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
          const int p = i | j;
          const uint4 a = tile[i], b = tile[p];
          const bool up = (i & k) == 0;
          if (Less::less(b, a) == up) {
            tile[i] = b;
            tile[p] = a;
          }
        }
        __syncthreads();
      }
    for (int i = (int)threadIdx.x; i < m; i += (int)blockDim.x) seg[i] = tile[i];
    __syncthreads();
  }
}

// pass `pass` merges runs of width kSegSortTile << pass; it reads buffer (pass & 1) and writes the other
template <class Less>
__global__ __launch_bounds__(kSegBlock) void segsort_merge(const unsigned long long* __restrict__ offsets, int n,
                                                           long long total, int pass, SortEntry* __restrict__ bufA,
                                                           SortEntry* __restrict__ bufB) {
  const long long w = (long long)kSegSortTile << pass;
  const uint4* src = reinterpret_cast<const uint4*>((pass & 1) ? bufB : bufA);
  uint4* dst = reinterpret_cast<uint4*>((pass & 1) ? bufA : bufB);
  const long long stride = (long long)gridDim.x * kSegBlock;
  for (long long k = (long long)blockIdx.x * kSegBlock + threadIdx.x; k < total; k += stride) {
    const int sg = segmentOf(offsets, n, k);
    const long long off = (long long)offsets[sg], len = (long long)offsets[sg + 1] - off;
    if (len <= w) continue;  // sorted already; stays in the buffer of its last pass
    const long long j = k - off;
    const long long L = j / (2 * w) * (2 * w);
    const long long mid = min(L + w, len), end = min(L + 2 * w, len);
    const uint4 e = src[k];
    long long rank;
    if (j < mid) {  // left run: the entries before it, plus the right run's entries below it
      long long lo = mid, hi = end;
      while (lo < hi) {
        const long long c = (lo + hi) >> 1;
        if (Less::less(src[off + c], e))
          lo = c + 1;
        else
          hi = c;
      }
      rank = (j - L) + (lo - mid);
    } else {  // right run (keys are unique: no tie to break)
      long long lo = L, hi = mid;
      while (lo < hi) {
        const long long c = (lo + hi) >> 1;
        if (Less::less(src[off + c], e))
          lo = c + 1;
        else
          hi = c;
      }
      rank = (j - mid) + (lo - L);
    }
    dst[off + L + rank] = e;  // L + rank < end <= len
  }
}

// Sorts the n segments of `offsets` (total entries, the longest maxLen) that lie in bufA; a segment longer than
// kSegSortTile takes merge passes through bufB and ends in buffer (segSortPasses(len) & 1), every other one stays in
// bufA. bufB may be null when maxLen <= kSegSortTile. Returns the number of kernels launched on `stream`.
template <class Less>
int launchSegSort(const unsigned long long* offsets, int n, long long total, long long maxLen, SortEntry* bufA,
                  SortEntry* bufB, hipStream_t stream) {
  if (maxLen <= kSegSmallTile)
    hipLaunchKernelGGL((segsort_tiles<Less, kSegSmallTile>), dim3((unsigned)n), dim3(kSegSmallBlock), 0, stream, offsets,
                       bufA);
  else
    hipLaunchKernelGGL((segsort_tiles<Less, kSegSortTile>), dim3((unsigned)n), dim3(kSegBlock), 0, stream, offsets,
                       bufA);
  int nl = 1;
  const int eblocks = (int)std::min<long long>(kSegMaxBlocks, (total + kSegBlock - 1) / kSegBlock);
  int pass = 0;
  for (long long w = kSegSortTile; w < maxLen; w <<= 1, ++pass) {
    hipLaunchKernelGGL(segsort_merge<Less>, dim3((unsigned)eblocks), dim3(kSegBlock), 0, stream, offsets, n, total, pass,
                       bufA, bufB);
    nl++;
  }
  return nl;
}

}  // namespace ccmi
