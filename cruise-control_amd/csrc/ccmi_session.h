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
