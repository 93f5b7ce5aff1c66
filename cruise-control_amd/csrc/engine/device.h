// Device side of a session: HBM tables, a host-coherent mapped staging area for row updates and scan
// requests, and the launch/readback protocol of one scan (no DMA copies, no stream synchronisation):
//   host  packs [row updates | request arrays] into the mapped staging area
//   K1/2  scan_cross / scan_pairs: when the update list fits the LDS overlay and the request is small, the
//         scan applies the rows itself and reads the request from the staging area (one launch);
//         otherwise K4 prep applies the rows and copies the request into HBM first
//   K5    scan_swap (+ visited sum) always after prep
//   the last workgroup writes one {seq, key} word into a host-mapped mailbox; the host spins on it
// Everything runs on one HIP stream per session, so HIP events on that stream time the kernels.
#pragma once
#include <functional>
#include <cstdint>
#include <cstring>
#include <string>
#include <unordered_map>
#include <memory>
#include <vector>

#include "devbuf.h"
#include "devtypes.h"
#include "intra.h"
#include "keyed_table.h"
#include "shard_group.h"
#include "snapseg.h"

struct ccmi_basic_stats;  // include/ccmi.h
struct ccmi_disk_stats;
struct ccmi_partition_load_record;
struct ccmi_swap_replica;
struct ccmi_proposal_record;
struct ccmi_proposal_summary;
struct ccmi_plan_task;
struct ccmi_plan_summary;

namespace ccmi {


// Algorithmic bytes per evaluated candidate: destination-broker record 4x f64 util, 4x f64 capacity,
// f64 potential NW_OUT, f64 leader NW_IN, i32 replica/leader/rack/topic-replica counts = 96 B.
constexpr int64_t kBytesPerCandidate = 96;
// K6 algorithmic bytes: per disk capacity + utilization + alive (17 B); per replica entry the replica id, disk,
// DISK utilization, score, Replica.compareTo rank, original disk and selection flag (29 B).
constexpr int64_t kIntraBytesPerDisk = 17;
constexpr int64_t kIntraBytesPerEntry = 29;

struct DevicePerf {
  int64_t scanLaunches = 0;
  int64_t scanPairs = 0;   // device-evaluated candidates (speculation included), pair-space size per launch
  double scanKernelMs = 0;
  int64_t scanBytes = 0;   // algorithmic bytes (96 B per evaluated candidate)
  int64_t statsLaunches = 0;
  double statsKernelMs = 0;
  int64_t statsBytes = 0;
  int64_t syncs = 0;
  int64_t singleLaunch = 0;  // scans that applied their rows in-kernel and read the request from host memory
  int64_t chainLaunches = 0; // K7 chains (several decisions per launch)
  int64_t scanRequired = 0;  // candidates the launches had to evaluate: each first-fit list up to its winner
  int64_t intraLaunches = 0;  // K6 intra-broker launches
  double intraKernelMs = 0;  // intra_brokers launches (HIP events, kernel timing on)
  double intraSortMs = 0;    // intra_sort launches (one per K6 call)
  int64_t intraSorts = 0;
  int64_t intraBytes = 0;     // algorithmic bytes of K6 (per broker record + per replica entry)
  int64_t combines = 0;       // shard-combiner calls (MIN allreduce of a scan's first-fit key)
  int64_t crossLaunches = 0;  // the scan_cross share of the scan counters
  int64_t crossRequired = 0;
  double crossKernelMs = 0;
  int64_t serverLaunches = 0;  // K8 scan_server launches (each serves many scans)
  int64_t serverIdleExits = 0;  // commands the server watchdog ended before it saw them (then launched)
  int64_t serverScans = 0;     // scans served by a running scan_server (no launch each)
  double serverBusyMs = 0;     // their device busy time (s_memrealtime, command seen -> result published)
  int64_t serverPayloadBytes = 0;  // command payload written through the BAR (program, rows, request arrays)
  int64_t serverRequired = 0;  // candidates those scans had to evaluate
  int64_t serverChains = 0;    // K7 chains the running server took as commands (no launch, no server restart)
  int64_t serverApplies = 0;   // apply-only server commands (topic-count deltas before a served scan that reads them)
  double serverResidentMs = 0;  // HIP-event time from each server launch to its exit (kernel timing on)
  int64_t acceptLaunches = 0;   // K9 accept_actions launches (acceptBatch)
  int64_t acceptCells = 0;      // (action, goal) cells they answered
  double acceptKernelMs = 0;    // their HIP-event time (kernel timing on)
  int64_t hostScans = 0;        // pair scans decided by the engine's host prefix (Engine::pairScan): nothing posted
  int64_t hostCandidates = 0;   // candidates the host prefix evaluated, misses included
  int64_t hostCrossScans = 0;       // cross scans decided by the host prefix (Engine::crossScan / crossScanSegs)
  int64_t hostCrossCandidates = 0;  // candidates the cross host prefix evaluated, misses included
};

// K6 (kernels/intra.hip, intra.h): one intra-broker goal over every broker in one launch.
struct IntraRequest {
  int32_t goal;               // IntraGoal
  double capThr, margin;
  int32_t nPrior = 0;
  int32_t priorKind[4] = {0, 0, 0, 0};
  int32_t priorSlot[4] = {0, 0, 0, 0};  // threshold slots of prior IG_USAGE goals
  int32_t slot = 0;               // this goal's threshold slot (IG_USAGE)
  const int32_t* brokers = nullptr;  // ascending broker ids to rebalance
  int32_t nBrokers = 0;
  const int32_t* eOff = nullptr;  // [B+1] CSR of the replicas on each broker's disks
  const int32_t* eRep = nullptr;
  const int32_t* eDisk = nullptr;
  const uint8_t* rSel = nullptr;  // [R] tracked-sorted-replica selection
};
struct IntraResult {
  std::vector<int32_t> count, status;  // [B] records / IntraStatus per broker
  std::vector<int64_t> cand;           // [B]
  std::vector<int64_t> off;            // [B+1] compact record offsets (broker-id order)
  std::vector<int32_t> rep, src, dst;  // records
  std::vector<double> upper, lower;    // [B] this goal's thresholds (IG_USAGE)
};
struct DiskStatsOut {  // ClusterModelStats.populateStatsForDisks partials
  double varSum;
  int32_t unbalanced, numAlive;
};
constexpr int kDiskStatsBlocks = 256;  // stats_disks workgroups (partials folded by one wave)

class Device {
 public:
  Device(int ordinal, int B, int R, int P, int T, int maxGoalSlots);
  static int countGfx950();  // visible gfx950 devices
  ~Device();
  Device(const Device&) = delete;
  Device& operator=(const Device&) = delete;

  // Host work the engine hands over for the time a scan is in flight: called between polls of the result until it
  // returns false (each call a few microseconds of host-only work that touches no device state). Set around one
  // scan by its caller.
  std::function<bool()> idleWork;
  // Adds the last server command's busy time to perf (the kernel publishes it just after the result word); called
  // before every command and before perf is read.
  void collectServerBusy();
  struct IdleScope {  // clears idleWork when the scan returns or throws
    Device* d;
    ~IdleScope() { d->idleWork = nullptr; }
  };

  // initial upload (host arrays in device layout)
  void uploadStatic(const double* bCapRM, const int32_t* rPart, const int32_t* rOrig, const int32_t* pOff,
                    const int32_t* topicNrep, const int32_t* bRack, const int32_t* pTopic);
  // Partition._ineligibleBrokers as CSR (n = list length; nothing is uploaded for n == 0)
  void uploadIneligible(const int32_t* off, const int32_t* brokers, int n);
  void uploadDynamic(const double* bUtilRM, const int32_t* bNrep, const int32_t* bNlead, const double* bPot,
                     const double* bLeadNwIn, const uint8_t* bAlive, const double* rUtilRM, const int32_t* rBroker,
                     const uint8_t* rFlags, const int32_t* pBrokers, const double* pLeadNwOut,
                     const int32_t* topicCountDense /* [T][ldB] */);
  void setAllowed(int slot, const uint8_t* allowedB);
  // Brokers sharing hosts (Model::sharedHosts): every broker's host utilization [B][3] (CPU, NW_IN, NW_OUT) and its
  // host's capacity [B][3] (Host.capacityFor); from then on the predicates and stats read host values for those
  void uploadHosts(const double* hutil, const double* hcap);
  // The host model's replica -> broker, replica -> partition and partition -> topic arrays (stable for the session):
  // cross / pair scans send each row with its broker, partition and topic (RowRef).
  void setRowSource(const int32_t* rBroker, const int32_t* rPart, const int32_t* pTopic) {
    rowBroker_ = rBroker;
    rowPart_ = rPart;
    partTopic_ = pTopic;
  }
  // OptimizationOptions.excludedBrokersFor{Leadership,ReplicaMove} as bits kExclLeadBit / kExclMoveBit of every
  // broker's allowedBits
  void setExclusions(const uint8_t* exclLead, const uint8_t* exclMove, const uint8_t* isNew);
  // TopicReplicaDistributionGoal balance limits per topic (frozen at its initGoalState)
  void setTopicLimits(const int32_t* upper, const int32_t* lower);
  // BrokerSetAwareGoal: BrokerRec.bset [B] (broker set of every broker) and ReplicaRec.bset [R] (the set the mapping
  // policy gives every replica), strided writes that leave the rest of the records alone
  void setBrokerSets(const int32_t* brokerSet, const int32_t* replicaSet);
  // Broker.numLeadersFor counts [T][ldB] (the host model's dense table), kept on the device from now on (deltas of
  // kind 1 and the chain kernels update them); MinTopicLeadersPerBrokerGoal's minimum per topic [T] (-1 = not its topic)
  void enableTopicLeaders(const int32_t* topicLeadDense);
  void setMinLeaders(const int32_t* tMin);
  // TopicLeaderReplicaDistributionGoal's (upper, lower) leader limits per topic [T][2] (frozen at its initGoalState)
  void setTopicLeadLimits(const int32_t* lim);

  // pending row updates (flushed with the next launch)
  std::vector<BrokerRow> brows;
  std::vector<ReplicaRow> rrows;
  std::vector<PartitionRow> prows;
  std::vector<TopicCountDelta> tdeltas;

  // returns the winning key or -1. Cross: rows reps[0,K) x columns [c0,c1) of cands[0,N), key = k*N + j.
  // Pairs: pairs [p0,p1) of (pr, pb), key = pair index. Keys are global, so shards MIN-combine them.
  int64_t scanCross(const DevProgram& prog, const int32_t* reps, int K, const int32_t* cands, int N, int c0, int c1);
  int64_t scanSwap(const DevProgram& prog, const int32_t* srcs, int S, const int32_t* cbOff, int M,
                   const int32_t* cbRep, int nCand, const SwapLimit& lim, int64_t* visited);
  int64_t scanPairs(const DevProgram& prog, const int32_t* pr, const int32_t* pb, int p0, int p1);
  // A cross scan whose rows are snapshot segments: segment i contributes (*v)[skip, end) (replicas on broker cb, the
  // snapshot current for cb). Each snapshot is uploaded once into a device-resident pool and the scan sends only
  // the segment table; keys are those of scanCross over the concatenated rows. Falls back to scanCross.
  using SegIn = SnapSeg;
  int64_t scanSegs(const DevProgram& prog, const std::vector<SegIn>& segs, const int32_t* cands, int N, int c0,
                   int c1);
  bool segsUsable() const { return serverUsable_ && serverAllowed_; }

  // Queue scans (SOP_QUEUE, devtypes.h): the rows of a whole broker queue in one command. Each broker's rows are its
  // snapshot under ONE Spec, uploaded once per broker version into the snapshot pool and found through the snapshot
  // directory (QueueDirEntry[B] in fine-grained VRAM, written by the host only when a broker's snapshot changes). The
  // engine keeps the directory current (qdirSet after every version bump it has not yet seen); the device only reads.
  bool queueUsable() const;
  // entries belong to `key` (the engine's Spec + selection identity); another key drops every entry
  void qdirBind(uint64_t key);
  uint64_t qdirKey() const { return qdirKey_; }
  // bumped when the pool wraps: every directory entry then refers to overwritten rows and must be set again
  uint32_t poolEpoch() const { return poolEpoch_; }
  // upload broker b's snapshot and point its directory entry at it (false: larger than the pool)
  bool qdirSet(int b, std::shared_ptr<const std::vector<int32_t>> v);
  // qdirSet(bs[i], snaps[i]) for many brokers at once: the pool offsets are assigned here, the rows are written
  // through the BAR on the host pool (each row's RowRef gathers its partition and topic: random reads of the model,
  // most of a directory sync's time). false: a snapshot does not fit the pool.
  bool qdirSetMany(const std::vector<int32_t>& bs, const std::vector<std::shared_ptr<const std::vector<int32_t>>>& snaps);
  const std::vector<int32_t>& qdirRows(int b) const { return *qdirSnap_[b]; }
  int qdirLen(int b) const { return qdirSnap_[b] ? (int)qdirSnap_[b]->size() : 0; }
  // first accepted (row, column) over the queue entries [head (if >= 0)] ++ tail[0, nTail) (entry 0 from row skip0) x
  // cands[0, N); key = (i * span + row) * N + column with span = queueSpan(); -1 when none. Every entry must be set for
  // the bound key.
  int64_t scanQueue(const DevProgram& prog, int head, int skip0, const int32_t* tail, int nTail, const int32_t* cands,
                    int N);
  int queueSpan() const { return qdirSpan_; }
  // The keyed membership table (devtypes.h KeyedRow; the engine's KeyedMirror is its host mirror): the queue scans'
  // rows without a sorted snapshot. kqBind: a table of B blocks of `stride` slots for `key`, every length 0 (false:
  // too large to allocate). kqWriteRow / kqSetLen: one row / one length word through the BAR; the command that reads
  // them is published behind a store fence.
  // The table's entry points are installed by the Device that has one (device.cpp, at construction). A Device build
  // without them has no table (hasKeyedTable() false): the engine then keeps only the mirror, and a keyed queue scan
  // is scanQueueKeyedFlat.
  struct KeyedOps {
    bool (*bind)(Device&, uint64_t key, int stride) = nullptr;
    void (*writeRow)(Device&, int b, int slot, int r, uint64_t key) = nullptr;
    void (*setLen)(Device&, int b, int len) = nullptr;
    int64_t (*scan)(Device&, const DevProgram& prog, const KeyedMirror& mir, int head, bool hasSkip, uint64_t skipKey,
                    const int32_t* tail, int nTail, const int32_t* cands, int N) = nullptr;
  };
  bool hasKeyedTable() const { return keyedOps_.bind != nullptr; }
  bool kqBind(uint64_t key, int stride) { return keyedOps_.bind(*this, key, stride); }
  void kqUnbind() { kqKey_ = 0; }
  uint64_t kqKey() const { return kqKey_; }
  void kqWriteRow(int b, int slot, int r, uint64_t key) { keyedOps_.writeRow(*this, b, slot, r, key); }
  void kqSetLen(int b, int len) { keyedOps_.setLen(*this, b, len); }
  // Diagnostics (ccmi_queue_probe.cpp): the table read back through the host mapping the rows were written through,
  // and the workgroups the last served queue command was sent to (0: none was served yet)
  int kqStride() const { return kqStride_; }
  int32_t kqLenAt(int b) const { return *reinterpret_cast<const volatile int32_t*>(&kqLens_[b]); }
  void kqReadBlock(int b, int len, KeyedRow* out) const {  // one copy per block: wide loads through the BAR
    std::memcpy(out, &kqRows_[(size_t)b * (size_t)kqStride_], (size_t)len * sizeof(KeyedRow));
  }
  int queueLastActive = 0;
  // scanQueue over the keyed table: an entry's rows in key order (entry 0: only keys above skipKey when hasSkip), so
  // the key's row is the winner's slot and span = the table's stride. `mir` is the table's host mirror (accounting,
  // and the rows of the flattened fallback).
  int64_t scanQueueKeyed(const DevProgram& prog, const KeyedMirror& mir, int head, bool hasSkip, uint64_t skipKey,
                         const int32_t* tail, int nTail, const int32_t* cands, int N) {
    return keyedOps_.scan(*this, prog, mir, head, hasSkip, skipKey, tail, nTail, cands, N);
  }
  // The same scan without a device table: the mirror's blocks sorted by key and flattened into one cross scan
  // (scanCross), its key mapped back to (entry, slot, column). Also what scanQueueKeyed falls back to without a server.
  int64_t scanQueueKeyedFlat(const DevProgram& prog, const KeyedMirror& mir, int head, bool hasSkip, uint64_t skipKey,
                             const int32_t* tail, int nTail, const int32_t* cands, int N) {
    const int hasHead = head >= 0 ? 1 : 0, n = hasHead + nTail, span = mir.stride();
    std::vector<int32_t> flat, entryOf, slotOf, v;
    for (int i = 0; i < n; ++i) {
      const int b = i < hasHead ? head : tail[i - hasHead];
      mir.sorted(b, v);
      for (size_t r = i == 0 && hasSkip ? (size_t)mir.atOrBelow(b, skipKey) : 0; r < v.size(); ++r) {
        flat.push_back(v[r]);
        entryOf.push_back(i);
        slotOf.push_back(mir.slotOf(v[r]));
      }
    }
    if (flat.empty() || N <= 0) return -1;
    const int64_t k = scanCross(prog, flat.data(), (int)flat.size(), cands, N, 0, N);
    if (k < 0) return -1;
    const int64_t fr = k / N;
    return ((int64_t)entryOf[fr] * span + slotOf[fr]) * N + k % N;
  }
  // Shard groups (shard_group.h): the block every rank of the group maps, and the group's rank count. A served cross /
  // segment / pair scan is then combined by the server (takeDeviceCombined() reports it once); any other combine goes
  // through groupCombineHost on the same slot sequence.
  void attachGroup(CombineBlock* blk, int count, int rank);
  // armGroupCombine before the scan call Engine::combine wraps: the first served cross / segment / pair command after it
  // combines on the device (a scan the engine does not combine — a queue scan's flattened fallback — is never tagged)
  void armGroupCombine() { combineArmed_ = grpHost_ != nullptr; }
  bool takeDeviceCombined() {
    const bool x = devCombined_;
    devCombined_ = false;
    combineArmed_ = false;
    return x;
  }
  int64_t groupCombineHost(int64_t key);  // -1 = none, both ways
  static CombineBlock* allocCombineBlock();
  static void freeCombineBlock(CombineBlock* b);
  // the session's scans may (not) use the resident scan server (sessions whose scans wait on other ranks may not)
  // at most `blocks` server workgroups from the next server launch on (a multiple of 8, at least 8)
  void limitServerBlocks(int blocks);
  // an API call that may scan on this device begins / ends (the device's server budget is shared among its active
  // calls, ensureServer)
  void callBegin();
  void callEnd();
  void setServerAllowed(bool on) {
    if (!on) stopServer();
    serverAllowed_ = on;
  }
  void stats(const StatsParams& P, const uint8_t* allowedAliveHost, StatsOut* out);

  // Chains (K7, kernels/scan.hip): decisions applied on the device inside one launch. uploadLoads gives the device
  // the Java loads and partition slot order (once per session); lrows / srows carry the entities the host changed
  // without the device since the last chain and are sent first.
  void uploadLoads(int W, const LoadVec* rLoad, const LoadVec* bLoad, const LoadVec* bLnw, const LoadVec* bPot,
                   const int32_t* pSlots, const int32_t* pLeader);
  // brokers sharing hosts: Host._load per host, each broker's host and the hosts' brokers (CSR), once per session
  void uploadHostLoads(int H, const LoadVec* hLoad, const int32_t* bHost, const int32_t* hOff, const int32_t* hBrk);
  std::vector<LoadRow> lrows;
  std::vector<SlotRow> srows;
  struct ChainResult {
    int64_t accepts = 0, visited = 0, failRow = 0;
  };
  // PAIRS chain; log receives the accepted pair indices in order
  ChainResult chainPairs(const DevProgram& prog, const int32_t* pr, const int32_t* pb, const int32_t* next, int n,
                         int maxAccepts, std::vector<int32_t>& log);
  // RACK_ROWS chain; log receives (row, candidate index) per accepted row
  ChainResult chainRackRows(const DevProgram& prog, const int32_t* rows, int n, const int32_t* cands, int N,
                            std::vector<int32_t>& log);
  // RackAwareGoal's rows decided per partition group with no optimized goals (rackrows.h): rows[0, n) in loop order,
  // order[gOff[g], gOff[g + 1]) the row indices of group g in row order; res[k] receives the accepted candidate
  // index, kRackKeep or kRackFail. Nothing is applied on the device. Returns the candidates evaluated.
  int64_t rackRowsGroups(const DevProgram& prog, const int32_t* rows, int n, const int32_t* order, const int32_t* gOff,
                         int G, const int32_t* cands, int N, int32_t* res);
  void flushOnly();
  void flushPending();

  // K9 (kernels/accept.hip, device_accept.cpp): Goal.actionAcceptance of every goal of `prog` (goals[0, nGoals), each
  // an actionAcceptance column: no slot is an optimizing goal) for nRows resolved actions. rows[0, nMoveRows) are moves
  // and leadership moves, rows[nMoveRows, nRows) swaps; both counts are whole wavefronts (the caller pads a segment
  // with copies of one of its rows). out[row * nGoals + g] receives the ccmi_acceptance value. The pending row updates go
  // to the tables first; one launch and one stream sync per acceptChunkRows() rows. Not in the test emulation.
  void acceptBatch(const DevProgram& prog, const AcceptRow* rows, int64_t nRows, int64_t nMoveRows, int8_t* out);
  int acceptChunkRows() const { return acceptChunkRows_; }
  // K10 (kernels/accept_mask.hip, device_accept.cpp): for each of nSources resolved move / leadership sources the mask
  // of destination brokers that are legit and that every goal of `prog` (goals[0, nGoals), nGoals >= 0, each an
  // actionAcceptance column) ACCEPTs: out[source * W + (b >> 6)] bit (b & 63), W = maskWords(); bits of brokers >= B are
  // 0. The pending row updates go to the tables first; one launch and one stream sync per CCMI_MASK_CHUNK_SOURCES sources.
  // Not in the test emulation.
  void maskBatch(const DevProgram& prog, const SourceRow* rows, int64_t nSources, uint64_t* out);
  int maskWords() const { return (B_ + 63) / 64; }
  // K11 (kernels/accept_swap.hip, device_accept.cpp): the swap code of every (source, candidate replica) pair of
  // nSources resolved sources and m candidate replica ids (1 <= m <= kMaxSwapCandidates) under `prog` (goals[0, nGoals),
  // nGoals >= 0, each an actionAcceptance column): out[source * m + candidate] = 3 / 4 when the first / second
  // legitMove fails, else the first non-ACCEPT verdict in goal order, else 0. The pending row updates go to the tables
  // first; one launch and one stream sync per max(1, min(65535, CCMI_SWAP_CHUNK_CELLS / pitch)) sources, pitch = m
  // rounded up to 64. Not in the test emulation.
  void swapGridBatch(const DevProgram& prog, const SourceRow* rows, int64_t nSources, const int32_t* cands, int64_t m,
                     int8_t* out);
  // K12 (kernels/broker_stats.hip, device_accept.cpp): ClusterModel.brokerStats from the resident tables.
  // uploadStatsStatic once per session: every broker's {desc host index, state}, the hosts' brokers as CSR (H hosts in
  // ascending host index hIdx, a host's brokers ascending) and every disk's broker. brokerStats: the pending row
  // updates go to the tables first; brokers[B]; hosts[H] unless null; disks[D] unless null or D == 0, its member counts
  // from members[0, nMembers) ({replica, disk} of every Disk._replicas entry), uploaded only when memberVer differs from
  // the last call's (setDiskUtil brings the disks' utilization current beforehand). One stream sync, one D2H copy per
  // output array. Counts into perf.statsLaunches / statsKernelMs / statsBytes. Not in the test emulation.
  bool statsStaticUploaded() const { return bool(statStatic_); }
  void uploadStatsStatic(const BrokerStatic* meta, int H, const int32_t* hOff, const int32_t* hBrk, const int32_t* hIdx,
                         const int32_t* dBroker);
  int statsHosts() const { return statH_; }
  uint64_t statsMemberVer() const { return statMemberVer_; }
  void brokerStats(ccmi_basic_stats* brokers, ccmi_basic_stats* hosts, ccmi_disk_stats* disks, const DiskMember* members,
                   int64_t nMembers, uint64_t memberVer);

  // K13 (kernels/partition_load.hip, device_accept.cpp): the partition load response from the resident tables: every
  // selected partition ordered by (utilization of q.resource on its current leader descending, tieRank ascending,
  // partition ascending), the first min(q.entries, selected) as records. uploadPartitionNumbers once per session
  // (TopicPartition.partition() of every partition). partitionLoad: the pending row updates and the pending chain
  // loads (lrows / srows, syncChainLoads) reach the tables first; topicSel[T], brokerSel[B], tieRank[P] may each be
  // null; records has room for min(q.entries, P) rows. A hand-written LSD radix sort on the device; the workspace is
  // one block allocated on first use. Two stream syncs (the counts, then the rows) and one D2H copy of the returned rows. Counts
  // into perf.statsLaunches / statsKernelMs / statsBytes. Not in the test emulation.
  bool partitionNumbersUploaded() const { return bool(plStatic_); }
  void uploadPartitionNumbers(const int32_t* pNumber);
  void partitionLoad(const PlQuery& q, const uint8_t* topicSel, const uint8_t* brokerSel, const int32_t* tieRank,
                     ccmi_partition_load_record* records, int64_t* numRecords, int64_t* numSelected);

  // K14 (kernels/proposal_diff.hip, device_accept.cpp): AnalyzerUtils.getDiff of the resident model against the
  // session's initial placement, and OptimizerResult.getMovementStats over the result. uploadInitialPlacement once per
  // session: the initial broker of every slot [R], the initial leader's broker [P] and, on a model with disks, the
  // initial disk of every slot [R] and of the leader [P]. proposalDiff: the pending row updates and the pending chain
  // loads (syncChainLoads) reach the tables first; curDisks[R] is the current disk of every slot (null exactly when the
  // model has no disks: disks are not resident); records has room for min(capacity, P) rows, the first
  // min(capacity, proposals) are written in ascending partition order; summary may be null. Two stream syncs at most
  // (the summary, then the rows when there are any). Counts into perf.statsLaunches / statsKernelMs / statsBytes. Not
  // in the test emulation.
  bool initialPlacementUploaded() const { return bool(pdStatic_); }
  void uploadInitialPlacement(const int32_t* initDist, const int32_t* initLeaders, const int32_t* initDisks,
                              const int32_t* initLeaderDisks);
  void proposalDiff(const int32_t* curDisks, ccmi_proposal_record* records, int64_t capacity, int64_t* numRecords,
                    ccmi_proposal_summary* summary);

  // K15 (kernels/sorted_replicas.hip, device_accept.cpp): per asked broker the list a freshly initialised
  // SortedReplicas of the Spec q would iterate. uploadSortedStatic once per session: Model::rStatic [R] (the rank of
  // Replica.compareTo's tail), and the call's scratch with it. sortedReplicas: the pending row updates and the pending
  // chain loads (syncChainLoads) reach the tables first; seg[B] maps a broker to its segment in [0, n) or -1;
  // topicExcluded[T] and topicIncluded[T] may each be null; offsets[n + 1] and *numRecords = offsets[n] are always
  // written; records (and scores, when not null) only when offsets[n] <= capacity. One stream sync for the offsets, one
  // more for the rows. Counts into perf.statsLaunches / statsKernelMs / statsBytes. Not in the test emulation.
  bool sortedStaticUploaded() const { return bool(srStatic_); }
  void uploadSortedStatic(const int32_t* rStatic);
  void sortedReplicas(const SrQuery& q, const int32_t* seg, int n, const uint8_t* topicExcluded,
                      const uint8_t* topicIncluded, int64_t* offsets, ccmi_swap_replica* records, double* scores,
                      int64_t capacity, int64_t* numRecords);

  // K16 (kernels/execution_plan.hip, device_accept.cpp): what ExecutionTaskPlanner.addExecutionProposals builds from
  // the proposals of K14; needs uploadInitialPlacement. The pending row updates and the pending chain loads
  // (syncChainLoads) reach the tables first; curDisks as proposalDiff's; rank[P] and state[P] may each be null. summary,
  // interOffsets[B + 1] and intraOffsets[B + 1] are always written; the other arrays only when every list fits its
  // capacity. One stream sync for the sums and offsets, one more for the lists. Counts into perf.statsLaunches /
  // statsKernelMs / statsBytes. Not in the test emulation.
  void executionPlan(const EpQuery& q, const int32_t* curDisks, const int32_t* rank, const uint8_t* state,
                     ccmi_plan_summary* summary, ccmi_plan_task* tasks, int64_t taskCap, int64_t* interOffsets,
                     int32_t* interEntries, int64_t interCap, int32_t* brokerOrder, int64_t* intraOffsets,
                     int32_t* intraEntries, int64_t intraCap, int32_t* leaderTasks, int64_t leaderCap);

  // Disks (JBOD): the static disk / replica tables once per session; setDiskUtil whenever the host changed a disk's
  // utilization; intraRun = one intra-broker goal (K6); statsDisks = the disk part of ClusterModelStats. uploadDisks
  // may be called again on a session (ccmi_session_mark_disks_for_removal re-sends the tables with the new capacities;
  // K6, stats_disks and broker_stats_disks read that one capacity table); setDiskUtil must follow it.
  void uploadDisks(int D, const int32_t* bDiskOff, const int32_t* bDisks, const double* dCap, const uint8_t* dAlive,
                   const uint8_t* bAlive, const int32_t* rOrigDisk, const double* rDu, const float* rScore,
                   const int32_t* rTie);
  void setDiskUtil(const double* dUtil);
  void intraRun(const IntraRequest& q, IntraResult& out);
  void statsDisks(double diskBalance, DiskStatsOut* out);

  DevicePerf perf;
  bool timing = false;  // record HIP events around kernels (bench/profiling)
  int ldB() const { return ldB_; }
  // K8 scan server (kernels/scan.hip scan_server): cross / pair scans are served by one persistent launch while it
  // runs; any other work on the session stream stops it first. CCMI_SERVER=0 turns it off (a launch per scan).
  void stopServer();

 private:
  int ordinal_, B_, R_, P_, T_, ldB_, G_;
  void* st_ = nullptr;  // hipStream_t
  // tables (records, devtypes.h) and the host copies used to assemble them
  BrokerRec* brokers_ = nullptr;
  ReplicaRec* replicas_ = nullptr;
  PartitionRec* parts_ = nullptr;
  int32_t *topicCount_ = nullptr, *topicNrep_ = nullptr, *tUpper_ = nullptr, *tLower_ = nullptr;
  int32_t *pIneligOff_ = nullptr, *pIneligB_ = nullptr;
  int32_t *topicLead_ = nullptr, *tMinLead_ = nullptr, *tLeadLim_ = nullptr;
  double* hostCap_ = nullptr;  // [B][3] Host.capacityFor of each broker's host (null: no shared hosts)
  uint8_t* allowedAlive_ = nullptr;
  std::vector<BrokerRec> hBrokers_;
  std::vector<PartitionRec> hParts_;
  std::vector<int32_t> hRPart_, hROrig_, hPOff_, bRackHost_;
  std::vector<uint32_t> allowedHost_;
  void *topicScratch_ = nullptr, *statsOut_ = nullptr, *statsPart_ = nullptr;
  // staging (host-coherent, mapped) and the request copy in HBM
  char* hStage_ = nullptr;
  char* hStageDev_ = nullptr;
  size_t stageCap_ = 0, stageUsed_ = 0;
  char* dReq_ = nullptr;
  size_t reqCap_ = 0;
  // result words in HBM, arrival counter, host mailbox {seq, value, extra}
  unsigned long long* dResult_ = nullptr;
  unsigned int* dDone_ = nullptr;
  unsigned long long* hResult_ = nullptr;
  unsigned long long* hResultDev_ = nullptr;
  unsigned long long seq_ = 0;
  alignas(16) unsigned char statsHost_[sizeof(StatsOut)];
  void *ev0_ = nullptr, *ev1_ = nullptr, *ev2_ = nullptr;  // hipEvent_t
  bool serverTimed_ = false;  // the running server launch has its start event recorded
  void *evS0_ = nullptr, *evS1_ = nullptr;  // hipEvent_t: a scan-server launch's residency (kernel timing on)
  struct Staged {
    int nb = 0, nr = 0, np = 0, nt = 0;
    size_t obr = 0, orr = 0, opr = 0, otd = 0, end = 0;
  };
  DevTables tables() const;
  size_t updatesBytes() const;
  Staged packUpdates(size_t extra);
  void unpackUpdates(const Staged& g);
  void ensureStage(size_t bytes);
  void ensureReq(size_t bytes);
  void launchPrepFor(const Staged& g, size_t reqBytes, bool scan);
  UpdateList stagedList(const Staged& g) const;
  UpdateList overlayFor(const Staged& g) const;
  MutTables mutTables() const;
  const char* stageScan(const Staged& g, size_t req, bool readsTopicCounts, UpdateList& u);
  bool waitMail(unsigned long long seq, bool serverCmd = false);
  int64_t finishScan();
  unsigned long long* stamps_ = nullptr;
  // scan server state: the fine-grained VRAM block [ServerCmd | payload] the host writes through the BAR
  char* fg_ = nullptr;
  size_t fgCap_ = 0;
  bool serverOn_ = false;
  bool serverUsable_ = false;  // set in the constructor (gfx950, CCMI_SERVER, fine-grained VRAM host-writable)
  bool serverAllowed_ = true;   // setServerAllowed
  CombineBlock* grpHost_ = nullptr;  // attachGroup: host pointer, this device's mapping, ranks, combines so far
  unsigned long long grpDev_ = 0;
  int grpCount_ = 0, grpRank_ = 0;
  uint64_t grpCalls_ = 0;
  uint32_t grpHostSeq_ = 0;  // host combines so far (their results arrive in mail[6] under this count)
  bool devCombined_ = false;
  bool combineArmed_ = false;
  std::vector<unsigned long long> groupMail_;  // the test emulation's shard-group mailbox (the product uses hResult_)
  int serverBlocks_ = 256;     // the running (or last) server launch's workgroups
  int serverBlocksCap_ = 256;  // at most this many (CU count, CCMI_SERVER_BLOCKS, limitServerBlocks)
  // goal-parallel server tiles (ServerCmd.goalParts): at most this many waves per candidate (CCMI_GOAL_SPLIT: 1, 2 or
  // 4) and only for scans whose split first sweep needs at most CCMI_GOAL_SPLIT_WGS workgroups
  int goalSplitMax_ = 4;
  bool applyViaServer_ = true;  // packForServer
  int goalSplitWgs_ = 256;
  // a server scan's first sweep sized from its site's last winner depth (serverRun; CCMI_SCAN_WIDTH=full: off)
  bool adaptiveWidth_ = true;
  // pair commands within one tile share their goals over several workgroups (serverRun; CCMI_WG_GOAL_SPLIT=0: off)
  bool wgGoalSplit_ = true;
  // Device::waitMail: polls of the result word before the first stream query (CCMI_QUERY_SPINS, default 16384)
  uint64_t spinsBeforeQuery_ = 16384;
  unsigned long long stuckTicks_ = 1000000000ull;  // 10 s of s_memrealtime: a command unpublished that long is stuck
  unsigned long long chainDelayTicks_ = 0;
  unsigned long long parkTicks_ = 100000ull;  // 1 ms: a shard-group scan waiting longer parks the server
  bool parkedPending_ = false;                // waitMail saw the server park with the awaited command
  size_t lrowsSent_ = 0, srowsSent_ = 0;      // CCMI_PROFILE: the last chain command's load / slot rows
  void retireParkedServer();
  bool claimServer();
  std::unordered_map<uint64_t, int64_t> lastDepth_;
  int progVer_ = 0;
  bool progSent_ = false;
  DevProgram lastProg_{};
  unsigned long long* dServerT0_ = nullptr;
  unsigned long long lastCmdSeq_ = 0;  // the sequence word the command block holds
  int32_t rowsEpoch_ = 0;              // server commands with rows so far (ServerCmd.rowsEpoch)
  double lastServerUse_ = 0;  // steady-clock seconds of the last served scan (the host restarts an idle server)
  bool serveScan(const DevProgram& prog, const Staged& g, bool readsTopicCounts);
  bool ensureServer();
  int serverProgram(const DevProgram& prog, char* pay);
  bool postCommand(ServerCmd& c, bool rowsSent);
  Staged packForServer(const DevProgram& prog, bool readsTc, bool& serve);
  bool busyPending_ = false;      // a completed command's busy time not yet collected
  unsigned long long busySeq_ = 0;
  // a K7 chain as a server command over the request arrays a0 | a1 | a2 (SOP_CHAIN); false = launch it instead
  bool serverChain(const DevProgram& prog, int mode, const int32_t* a0, int n0, const int32_t* a1, int n1,
                   const int32_t* a2, int n2, int n, int m, int maxAccepts);
  void streamWait(const char* what, double seconds);
  // one chunk's acceptBatch verdicts [rows][nGoals], maskBatch words [sources][W] or swapGridBatch codes [sources][pitch],
  // grown to the largest chunk so far
  DevBuf acceptOut_;
  int8_t* dAccept() const { return (int8_t*)acceptOut_.get(); }
  // device_accept.cpp, its only user. PlainLaunch: the scope of a call that launches on the session stream with no
  // server resident. acceptChunk: one chunk of acceptBatch / maskBatch / swapGridBatch — fill(p) writes the req-byte
  // request behind the staged row updates, prep takes both to HBM, launch(stream) starts the kernel and its outBytes of
  // acceptOut_ come back to dst; one stream sync, one accept launch counted. timedLaunch / addKernelMs: the HIP-event
  // pair around a call's kernels and, after the stream wait, their time (kernel timing on).
  struct PlainLaunch;
  template <class Fill, class Launch>
  void acceptChunk(size_t req, Fill fill, size_t outBytes, Launch launch, void* dst, const char* kernel,
                   const char* copy);
  template <class Launch>
  void timedLaunch(Launch launch);
  void addKernelMs(double& total);
  int acceptChunkRows_ = 1 << 17;  // action rows per launch (CCMI_ACCEPT_CHUNK_ROWS, read at session create)
  int maskChunkSources_ = 4096;    // sources per launch (CCMI_MASK_CHUNK_SOURCES, read at session create)
  std::vector<int8_t> swapHost_;      // one chunk's pitched codes on the host, before the pitch is removed
  int64_t swapChunkCells_ = 1 << 24;  // padded swap cells per launch (CCMI_SWAP_CHUNK_CELLS, read at session create)
  // K12-K16 (device_accept.cpp; devbuf.h, DESIGN.md "Query workspaces"): per query one DevBuf per lifetime (the static
  // tables of its upload, the workspace of its first use, the outputs that grow) and a struct of typed pointers that one
  // layout function fills. "Uploaded" and "first use done" are bool(buffer): a block is there whole or not at all.
  // brokerStats. Static: the broker columns [B], the hosts' CSR [H + 1], [B], [H], the output rows [B] broker rows |
  // [H] host rows and, on a model with disks, the disks' brokers and output rows [D]. The member list of the disks grows,
  // with the Model::diskMemberVer it was built at (0 = none).
  struct StatTables {
    BrokerStatic* meta = nullptr;
    int32_t *hOff = nullptr, *hBrk = nullptr, *hIdx = nullptr, *dBroker = nullptr;
    ccmi_basic_stats* rows = nullptr;
    ccmi_disk_stats* disks = nullptr;
  } stat_;
  void layoutStat(Carver& c);
  DevBuf statStatic_, statMembersBuf_;
  int64_t statMembers_ = 0;
  uint64_t statMemberVer_ = 0;
  int statH_ = 0;
  // partitionLoad. Static: the partition numbers [P]. First use: the query's arrays, the ping-pong sort buffers [P]
  // each, the [256 x tiles] digit counts, the query state. The output rows grow to the largest request so far.
  struct PlWork {
    int32_t* rank = nullptr;
    uint8_t *topicSel = nullptr, *brokerSel = nullptr;
    PlEntry* buf[2] = {nullptr, nullptr};
    uint32_t* counts = nullptr;
    PlState* state = nullptr;
  } pl_;
  void layoutPl(Carver& c);
  DevBuf plStatic_, plWork_, plOut_;
  // proposalDiff. Static: the initial placement (the disks only on a model with disks). First use: the [tiles + 1] tile
  // counts, the current disks of a call [R], the sums. The output rows grow to the largest capacity so far.
  struct PdStatic {
    int32_t *initDist = nullptr, *initLeaders = nullptr, *initDisks = nullptr, *initLeaderDisks = nullptr;
  } pdInit_;
  struct PdWork {
    uint32_t* counts = nullptr;
    int32_t* curDisks = nullptr;
    PdSums* sums = nullptr;
  } pd_;
  void layoutPdStatic(Carver& c);
  void layoutPd(Carver& c);
  DevBuf pdStatic_, pdWork_, pdOut_;
  // sortedReplicas. Static, the call's scratch with it: the tail ranks [R], the segment map, counts and cursors [B],
  // {total, longest, offsets} [B + 3], the topic masks [T], the keys and segments [R], the entry buffer [R]. The merge
  // passes' second entry buffer [R] comes once a segment is longer than a tile. The output records and scores grow
  // together to the largest total so far.
  struct SrWork {
    int32_t *rStatic = nullptr, *seg = nullptr, *segOf = nullptr;
    uint32_t *counts = nullptr, *cursor = nullptr;
    unsigned long long* state = nullptr;
    uint8_t *topicExcl = nullptr, *topicIncl = nullptr;
    uint64_t* keys = nullptr;
    SortEntry* buf = nullptr;
  } sr_;
  void layoutSr(Carver& c);
  DevBuf srStatic_, srMerge_, srOut_;
  std::vector<unsigned long long> srHost_;
  // executionPlan. First use: the rows and execution ids [P], the call's rank [P], state [P] and current disks [R], the
  // broker order [B], the tile counts [2][tiles + 1], the broker counts and cursors [2 B], {total, longest, offsets} of
  // both lists and the two one-segment offsets [2 (B + 3) + 4], the sums. The two entry buffers grow together (a merge
  // pass may come with any call); each output list grows on its own to the largest call so far.
  struct EpWork {
    EpRow* rows = nullptr;
    int32_t *idOf = nullptr, *rank = nullptr, *curDisks = nullptr, *order = nullptr;
    uint8_t* pstate = nullptr;
    uint32_t *tiles = nullptr, *counts = nullptr, *cursors = nullptr;
    unsigned long long* state = nullptr;
    EpSums* sums = nullptr;
  } ep_;
  void layoutEp(Carver& c);
  DevBuf epWork_, epEntries_, epTasks_, epInter_, epIntra_, epLeader_;
  std::vector<unsigned long long> epHost_;
  // the pending chain loads (lrows / srows) go to the device's Java loads and slot order outside a chain
  void syncChainLoads();
  int32_t* dRackRes_ = nullptr;  // rackRowsGroups results (+ the evaluated-candidate counter after them)
  size_t rackResCap_ = 0;
  int32_t* dChainReq_ = nullptr;  // SOP_CHAIN request copy in HBM (the chain rereads it per decision)
  size_t chainReqCap_ = 0;
  const int32_t *rowBroker_ = nullptr, *rowPart_ = nullptr, *partTopic_ = nullptr;
  void writeRowRefs(char* dst, const int32_t* reps, size_t n) const;
  // A: replica ids sent as RowRefs (nA entries), or for SOP_SEGS the segment table (nA entries of SegEntry)
  int64_t serverRun(const DevProgram& prog, const Staged& g, int op, const void* A, size_t nA, const int32_t* C,
                    size_t nC, const int32_t params[6]);
  // snapshot pool (fine-grained VRAM, ring of RowRefs; a wrap restarts the server so no cache holds a reused line)
  RowRef* segPool_ = nullptr;
  size_t segCap_ = 0, segHead_ = 0;
  std::unordered_map<const void*, std::pair<std::shared_ptr<const std::vector<int32_t>>, uint32_t>> segCache_;
  std::vector<int32_t> segFlat_;
  std::vector<SegEntry> segTab_;
  int64_t segUpload(const SegIn& s);  // pool index of the snapshot's first entry, or -1 (does not fit)
  uint32_t poolEpoch_ = 0;
  uint64_t qdirKey_ = 0;
  int qdirSpan_ = 1;  // >= every set entry's length since the last bind
  QueueDirEntry* qdir_ = nullptr;  // fine-grained VRAM [B] (host-written through the BAR)
  std::vector<std::shared_ptr<const std::vector<int32_t>>> qdirSnap_;  // [B] the snapshot each entry points at
  // keyed membership table: one fine-grained VRAM block, the length words [B] then the rows [B * kqStride_]
  uint64_t kqKey_ = 0;
  int kqStride_ = 0;
  size_t kqBytes_ = 0;
  char* kqMem_ = nullptr;
  int32_t* kqLens_ = nullptr;
  KeyedRow* kqRows_ = nullptr;
  KeyedOps keyedOps_;
  bool kqBindImpl(uint64_t key, int stride);
  void kqWriteRowImpl(int b, int slot, int r, uint64_t key);
  void kqSetLenImpl(int b, int len);
  // scanQueue (mir null; skip0 rows of entry 0 skipped) and scanQueueKeyed (skip0 != 0: skipKey applies) in one
  int64_t scanQueueImpl(const DevProgram& prog, const KeyedMirror* mir, int head, int skip0, uint64_t skipKey,
                        const int32_t* tail, int nTail, const int32_t* cands, int N);
  void ensureFg(size_t bytes);
  int32_t* rowVisited_ = nullptr;
  size_t rowVisitedCap_ = 0;
  // chain state
  int W_ = 1;
  LoadVec *dRLoad_ = nullptr, *dBLoad_ = nullptr, *dBLnw_ = nullptr, *dBPot_ = nullptr, *dHLoad_ = nullptr;
  int32_t *dBHost_ = nullptr, *dHOff_ = nullptr, *dHBrk_ = nullptr;
  int32_t *dPOff_ = nullptr, *dPSlots_ = nullptr, *dPLeader_ = nullptr;
  // chain results in host-coherent mapped memory: the kernels write them, the host reads them after the stream sync
  // (no device-to-host copies per chain)
  int32_t* hChainLog_ = nullptr;
  int32_t* hChainLogDev_ = nullptr;
  size_t chainLogCap_ = 0;
  ChainResultDev* hChainOut_ = nullptr;
  ChainResultDev* hChainOutDev_ = nullptr;
  void ensureChainLog(size_t n);
  ChainTables chainTables() const;
  template <class F>
  size_t stageChainCopy(size_t reqBytes, Staged& g, size_t& oReq, F fill, void* stream);
  // disk state (K6)
  int D_ = 0;
  int32_t *dBDiskOff_ = nullptr, *dBDisks_ = nullptr, *dROrigDisk_ = nullptr, *dRTie_ = nullptr;
  double *dDCap_ = nullptr, *dDUtilIn_ = nullptr, *dDUtil_ = nullptr, *dRDu_ = nullptr;
  uint8_t *dDAlive_ = nullptr, *dBAlive_ = nullptr, *dRSel_ = nullptr;
  float* dRScore_ = nullptr;
  double *dUpper_ = nullptr, *dLower_ = nullptr;  // [G][B] usage-goal thresholds
  int32_t *dEOff_ = nullptr, *dERep_ = nullptr, *dEDiskIn_ = nullptr, *dEDisk_ = nullptr, *dSnapA_ = nullptr,
          *dSnapB_ = nullptr, *dOrdRev_ = nullptr, *dOrdFwd_ = nullptr, *dNSel_ = nullptr, *dHist_ = nullptr, *dBrokers_ = nullptr, *dLogCap_ = nullptr, *dCount_ = nullptr,
          *dStatus_ = nullptr, *dLogRep_ = nullptr, *dLogSrc_ = nullptr, *dLogDst_ = nullptr, *dCRep_ = nullptr,
          *dCSrc_ = nullptr, *dCDst_ = nullptr;
  int64_t *dLogOff_ = nullptr, *dCand_ = nullptr, *dCOff_ = nullptr;
  IntraRep* dRStat_ = nullptr;  // K6 packed static replica fields
  double* dEDu_ = nullptr;  // K6 entry-indexed gathers (IntraArgs.eDu / eOrig / eKeyRev / eKeyFwd)
  int32_t* dEOrig_ = nullptr;
  uint64_t *dEKeyRev_ = nullptr, *dEKeyFwd_ = nullptr;
  size_t entCap_ = 0, logCap_ = 0, compactCap_ = 0;
  DiskStatsOut* dDiskStats_ = nullptr;
  std::vector<void*> intraAllocs_;
  std::vector<int32_t> hBDiskOff_;
};


}  // namespace ccmi
