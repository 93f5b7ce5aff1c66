// What the translation units behind the C ABI share (ccmi_api.cpp, ccmi_accept.cpp): the session object and the
// exception-to-status mapping. Private to the library; include/ccmi.h only names the structs.
#pragma once
#include <exception>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "ccmi.h"
#include "engine/device.h"
#include "engine/engine.h"
#include "engine/errors.h"
#include "engine/model.h"
#include "engine/shard_rccl.h"
#include "engine/shard_shm.h"

struct ccmi_session;
struct ccmi_shard_group {
  ccmi::CombineBlock* blk = nullptr;
  int32_t count = 0;
  // attached sessions by rank; a destroyed session clears its slot and a destroyed group its sessions' back pointers,
  // so neither side is ever read after it is freed
  std::vector<ccmi_session*> ranks;
};

struct ccmi_session {
  ~ccmi_session();  // ccmi_api.cpp: leaves its shard group, ends its combiners
  ccmi::Model model;
  std::unique_ptr<ccmi::Device> device;
  std::unique_ptr<ccmi::Engine> engine;
  ccmi::RcclShard* rccl = nullptr;
  ccmi::ShmShard* shm = nullptr;
  ccmi_shard_group* group = nullptr;  // the shard group this session is a rank of (ccmi_session_attach_group)
  int32_t groupRank = -1;
  int deviceOrdinal = 0;
  std::vector<int32_t> initDist, initLeaders;  // for ExecutionProposal diffs
  std::vector<int32_t> initDisks, initLeaderDisks;  // the logdir half of ReplicaPlacementInfo (JBOD)
  struct Prop {
    int32_t partition, size, oldLeader;
    std::vector<int32_t> oldR, newR, oldD, newD;
  };
  std::vector<Prop> proposals;
};

// ---- Queue-scan diagnostics (ccmi_queue_probe.cpp). Not part of the ABI: include/ccmi.h does not declare them and
// CCMI_ABI_VERSION does not count them. One queue scan (Engine::queueScan's device call) chosen by the caller on the
// session's current model, with the answer a plain host loop over the model gives for the same arguments.
struct ccmi_queue_probe_args {
  // the Spec of the entries' rows (the fields Engine's directory identity mixes that a queue scan's callers set)
  int32_t sel_leaders;      // 1: leader replicas only
  int32_t score_res;        // 0..3: rows ordered by this resource's score; -1: none
  int32_t score_reverse;
  int32_t prio_offline, prio_immigrants;
  int32_t sel_excl_topics;  // 1: leave out the replicas of the session's excluded topics (the last options')
  // the program: the goal being optimized (an optimized goal kind; goals[0], selfSatisfied) and the acceptance goals
  int32_t self_kind;
  int32_t num_accept;
  const int32_t* accept_kinds;
  // the queue: [head (or -1)] ++ tail[0, n_tail), distinct brokers; has_skip: the head's rows at or below skip_key
  // were walked before
  int32_t head, has_skip;
  uint64_t skip_key;
  const int32_t* tail;
  int32_t n_tail;
  const int32_t* cands;  // the columns
  int32_t n_cands;
  int32_t mode;  // 0: everything; 1: no table audit; 2: the host loop only (nothing is sent to the device)
};
struct ccmi_queue_probe_report {
  int32_t dev_entry, dev_replica, dev_column;  // the device's winner, -1 each: none
  int32_t ref_entry, ref_replica, ref_column;  // the host loop's
  int32_t served;    // 1: a scan-server queue command answered, 0: the flattened fall-back (or an emulated Device)
  int32_t keyed;     // 1: the keyed membership table was current, 0: the snapshot directory
  int32_t stride;    // keyed: the table's slots per broker
  int32_t n_active;  // served: the workgroups the command was sent to
  // keyed: brokers whose rows {(key, replica, partition, topic)} or length differ between the model, the mirror and
  // (audited & 2) the device table read back; audited: bit 0 the mirror was compared, bit 1 the device table
  int32_t audit, audited;
  // coverage facts, from the host loop (slots are the mirror's, -1 when not keyed): the winner's slot in its block,
  // the rows of the winner's entry with an accepted column (after the head's mask) and the lowest and highest slot
  // among them, the winner's entry's length (masked rows included) and the winner's index in its key order (win_len -
  // 1: the highest-key row), the head rows masked and the winner's row key
  int32_t win_slot, accepted_rows, lowest_accepted_slot, highest_accepted_slot, win_len, win_rank, head_masked;
  int32_t pad;
  uint64_t win_key;
};
extern "C" ccmi_status ccmi_queue_probe(ccmi_session* s, const ccmi_queue_probe_args* a, ccmi_queue_probe_report* out);
// Broker b's rows under the args' Spec (the queue and program fields are not read), in key order, from the model:
// up to `capacity` (key, replica) pairs; *count: how many there are. slots (may be null): the slot each replica has in
// the broker's block of the keyed mirror as the last queue sync left it (the caller knows for which Spec), -1: none
extern "C" ccmi_status ccmi_queue_probe_view(ccmi_session* s, const ccmi_queue_probe_args* a, int32_t broker,
                                             uint64_t* keys, int32_t* replicas, int32_t* slots, int32_t capacity,
                                             int32_t* count);

namespace ccmi {
void setLastError(const std::string& msg);  // the message ccmi_last_error() returns on this thread
}  // namespace ccmi

// Exceptions never cross the boundary: every entry point maps them to a ccmi_status and keeps the message.
template <class F>
ccmi_status guarded(F&& f) {
  auto fail = [](ccmi_status s, const std::string& msg) {
    ccmi::setLastError(msg);
    return s;
  };
  try {
    return f();
  } catch (ccmi::OptimizationFailure& e) {
    return fail(CCMI_E_OPT_FAILURE, e.what());
  } catch (ccmi::StateError& e) {
    return fail(CCMI_E_STATE, e.what());
  } catch (ccmi::Unsupported& e) {
    return fail(CCMI_E_UNSUPPORTED, e.what());
  } catch (std::invalid_argument& e) {
    return fail(CCMI_E_INVALID, e.what());
  } catch (std::exception& e) {
    const std::string w = e.what();
    return fail(w.rfind("HIP", 0) == 0 || w.find("gfx950") != std::string::npos || w.find("device") != std::string::npos
                    ? CCMI_E_DEVICE
                    : CCMI_E_INVALID,
                w);
  }
}
