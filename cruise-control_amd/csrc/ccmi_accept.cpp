// ccmi_actions_acceptance (ABI v13): Goal.actionAcceptance of several optimized goals for a batch of actions, answered
// on the device (Device::acceptBatch, kernels/accept.hip), and ccmi_moves_acceptance_mask: the destination brokers every
// optimized goal accepts for a batch of move / leadership sources (Device::maskBatch, kernels/accept_mask.hip), and
// ccmi_swaps_acceptance_grid: one code per (source replica, candidate replica) pair of a swap loop
// (Device::swapGridBatch, kernels/accept_swap.hip). A translation unit of its own: it holds the only callers of those
// three launchers, which the test emulation of Device does not have.
#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "ccmi.h"
#include "ccmi_session.h"
#include "engine/threadpin.h"

namespace {

using ccmi::AcceptRow;

// The batch in device order: moves and leadership moves first, swaps after them, each segment padded to whole
// wavefronts with copies of its last row (index -1: no caller row) so a wavefront runs one dispatch function.
struct Resolved {
  std::vector<AcceptRow> rows;
  std::vector<int64_t> index;  // caller's action index of every row, -1 = padding
  int64_t nMoveRows = 0;
};

void padToWave(Resolved& r) {
  while (r.rows.size() % 64 != 0) {
    r.rows.push_back(r.rows.back());
    r.index.push_back(-1);
  }
}

// The row of action i as Engine::acceptance resolves it; throws what the single call throws. Indices are checked
// against the model first (the kernel trusts its rows).
AcceptRow resolve(const ccmi::Model& m, const ccmi_action& a) {
  if (a.type != CCMI_INTER_BROKER_REPLICA_MOVEMENT && a.type != CCMI_LEADERSHIP_MOVEMENT &&
      a.type != CCMI_INTER_BROKER_REPLICA_SWAP)
    throw std::invalid_argument("Unsupported balancing action " + std::to_string(a.type) + " is provided.");
  auto partition = [&](int p) {
    if (p < 0 || p >= m.P) throw std::invalid_argument("partition out of range");
  };
  auto broker = [&](int b) {
    if (b < 0 || b >= m.B) throw std::invalid_argument("broker out of range");
  };
  partition(a.partition);
  broker(a.source_broker);
  broker(a.destination_broker);
  const int sr = m.replicaOn(a.partition, a.source_broker);
  if (sr < 0) throw std::invalid_argument("no replica of the partition on the source broker");
  if (a.type == CCMI_INTER_BROKER_REPLICA_SWAP) {
    partition(a.destination_partition);
    const int dr = m.replicaOn(a.destination_partition, a.destination_broker);
    if (dr < 0) throw std::invalid_argument("no replica of the destination partition on the destination broker");
    return AcceptRow{sr, dr, a.destination_broker, ccmi::DA_SWAP};
  }
  return AcceptRow{sr, -1, a.destination_broker,
                   a.type == CCMI_LEADERSHIP_MOVEMENT ? ccmi::DA_LEADERSHIP : ccmi::DA_MOVE};
}

}  // namespace

extern "C" ccmi_status ccmi_actions_acceptance(ccmi_session* s, const int32_t* goal_kinds, int32_t num_goals,
                                               const ccmi_action* actions, int64_t n, int8_t* acceptance,
                                               int64_t* first_invalid) {
  if (first_invalid) *first_invalid = -1;
  return guarded([&] {
    if (!s) throw std::invalid_argument("null session");
    if (num_goals < 0 || n < 0) throw std::invalid_argument("negative count");
    if ((num_goals > 0 && !goal_kinds) || (n > 0 && !actions) || (n > 0 && num_goals > 0 && !acceptance))
      throw std::invalid_argument("null argument");
    ccmi::Engine& e = *s->engine;
    // each kind is the session's latest optimization of it (ccmi_action_acceptance_by_kind)
    std::vector<const ccmi::GoalImpl*> goals(num_goals);
    for (int g = 0; g < num_goals; ++g) {
      goals[g] = e.optimizedOfKind(goal_kinds[g]);
      if (!goals[g])
        throw std::invalid_argument("the session has not optimized goal kind " + std::to_string(goal_kinds[g]));
    }
    if (n == 0 || num_goals == 0) return CCMI_OK;
    const ccmi::ThreadPin pin(s->deviceOrdinal);  // restored when the call returns
    // columns of intra-broker goals are the host's (they read the disk tables the scan kernels do not hold)
    std::vector<int> devCols;
    const ccmi::GoalImpl* terminal = nullptr;
    for (int g = 0; g < num_goals; ++g)
      if (!ccmi::isIntraGoalKind(goals[g]->kind)) {
        devCols.push_back(g);
        if (!terminal && goals[g]->terminal) terminal = goals[g];
      }
    // every error of the single calls, before anything runs on the device
    Resolved moves, swaps;
    for (int64_t i = 0; i < n; ++i) {
      const ccmi_action& a = actions[i];
      try {
        for (int g = 0; g < num_goals; ++g)
          if (ccmi::isIntraGoalKind(goals[g]->kind))
            acceptance[i * num_goals + g] = (int8_t)ccmi::intraAcceptance(*goals[g], e, a);
        if (devCols.empty()) continue;
        if (a.type == CCMI_INTRA_BROKER_REPLICA_MOVEMENT || a.type == CCMI_INTRA_BROKER_REPLICA_SWAP)
          throw std::invalid_argument("Unsupported balancing action " + std::to_string(a.type) + " is provided.");
        if (terminal) throw ccmi::StateError("No goal should be executed after " + terminal->name);
        const AcceptRow row = resolve(s->model, a);
        Resolved& seg = row.action == ccmi::DA_SWAP ? swaps : moves;
        seg.rows.push_back(row);
        seg.index.push_back(i);
      } catch (std::invalid_argument&) {
        if (first_invalid) *first_invalid = i;
        throw;
      }
    }
    if (devCols.empty()) return CCMI_OK;
    padToWave(moves);
    padToWave(swaps);
    Resolved all = std::move(moves);
    all.nMoveRows = (int64_t)all.rows.size();
    all.rows.insert(all.rows.end(), swaps.rows.begin(), swaps.rows.end());
    all.index.insert(all.index.end(), swaps.index.begin(), swaps.index.end());
    const int64_t nRows = (int64_t)all.rows.size();

    s->model.flushToDevice();  // the rows the host changed since the last launch (ccmi_session_apply, a goal's moves)
    std::vector<int8_t> cells;
    for (size_t c0 = 0; c0 < devCols.size(); c0 += ccmi::kMaxGoals) {
      const int G = (int)std::min<size_t>(ccmi::kMaxGoals, devCols.size() - c0);
      // every slot is an actionAcceptance column: no slot is the goal being optimized. The kernel gathers whole
      // records, so the scan programs' operand mask and candidate filters stay clear.
      ccmi::DevProgram prog;
      std::memset(&prog, 0, sizeof(prog));
      prog.nGoals = G;
      prog.action = ccmi::DA_MOVE;
      for (int g = 0; g < G; ++g) prog.goals[g] = goals[devCols[c0 + g]]->dg;
      cells.resize((size_t)nRows * G);
      s->device->acceptBatch(prog, all.rows.data(), nRows, all.nMoveRows, cells.data());
      s->device->perf.acceptCells += n * G;
      for (int64_t r = 0; r < nRows; ++r) {  // back to the caller's order
        const int64_t i = all.index[r];
        if (i < 0) continue;
        for (int g = 0; g < G; ++g) acceptance[i * num_goals + devCols[c0 + g]] = cells[(size_t)r * G + g];
      }
    }
    return CCMI_OK;
  });
}

extern "C" ccmi_status ccmi_moves_acceptance_mask(ccmi_session* s, const int32_t* goal_kinds, int32_t num_goals,
                                                  const ccmi_move_source* sources, int64_t n, uint64_t* mask,
                                                  int64_t* first_invalid) {
  if (first_invalid) *first_invalid = -1;
  return guarded([&] {
    if (!s) throw std::invalid_argument("null session");
    if (num_goals < 0 || n < 0) throw std::invalid_argument("negative count");
    if ((num_goals > 0 && !goal_kinds) || (n > 0 && (!sources || !mask))) throw std::invalid_argument("null argument");
    ccmi::Engine& e = *s->engine;
    // each kind is the session's latest optimization of it; a kind named twice is evaluated twice (a conjunction)
    std::vector<const ccmi::GoalImpl*> goals;
    const ccmi::GoalImpl* terminal = nullptr;
    for (int g = 0; g < num_goals; ++g) {
      if (ccmi::isIntraGoalKind(goal_kinds[g]))
        throw ccmi::Unsupported("goal kind " + std::to_string(goal_kinds[g]) +
                                " is an intra-broker goal: it shares no chain with inter-broker goals and has no "
                                "destination-broker mask; ccmi_actions_acceptance answers its cells on the host");
      const ccmi::GoalImpl* goal = e.optimizedOfKind(goal_kinds[g]);
      if (!goal) throw std::invalid_argument("the session has not optimized goal kind " + std::to_string(goal_kinds[g]));
      if (!terminal && goal->terminal) terminal = goal;
      goals.push_back(goal);
    }
    if (n == 0) return CCMI_OK;
    if (terminal) throw ccmi::StateError("No goal should be executed after " + terminal->name);
    // every source against the model before anything runs on the device (the kernel trusts its rows)
    const ccmi::Model& m = s->model;
    std::vector<ccmi::MaskRow> rows((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
      const ccmi_move_source& a = sources[i];
      try {
        if (a.type != CCMI_INTER_BROKER_REPLICA_MOVEMENT && a.type != CCMI_LEADERSHIP_MOVEMENT)
          throw std::invalid_argument("a move source is a replica movement or a leadership movement, not action type " +
                                      std::to_string(a.type));
        if (a.partition < 0 || a.partition >= m.P) throw std::invalid_argument("partition out of range");
        if (a.source_broker < 0 || a.source_broker >= m.B) throw std::invalid_argument("broker out of range");
        const int sr = m.replicaOn(a.partition, a.source_broker);
        if (sr < 0) throw std::invalid_argument("no replica of the partition on the source broker");
        rows[(size_t)i] = ccmi::MaskRow{sr, a.partition, a.source_broker,
                                        a.type == CCMI_LEADERSHIP_MOVEMENT ? ccmi::DA_LEADERSHIP : ccmi::DA_MOVE};
      } catch (std::invalid_argument&) {
        if (first_invalid) *first_invalid = i;
        throw;
      }
    }
    const ccmi::ThreadPin pin(s->deviceOrdinal);  // restored when the call returns
    s->model.flushToDevice();  // the rows the host changed since the last launch (ccmi_session_apply, a goal's moves)
    const size_t words = (size_t)n * (size_t)s->device->maskWords();
    std::vector<uint64_t> part;
    // one device program per kMaxGoals goals (at least one: without goals, the legit mask); the masks are ANDed
    for (size_t c0 = 0; c0 == 0 || c0 < goals.size(); c0 += ccmi::kMaxGoals) {
      const int G = (int)std::min<size_t>(ccmi::kMaxGoals, goals.size() - c0);
      // every slot is an actionAcceptance column, as in ccmi_actions_acceptance
      ccmi::DevProgram prog;
      std::memset(&prog, 0, sizeof(prog));
      prog.nGoals = G;
      prog.action = ccmi::DA_MOVE;
      for (int g = 0; g < G; ++g) prog.goals[g] = goals[c0 + g]->dg;
      if (c0 == 0) {
        s->device->maskBatch(prog, rows.data(), n, mask);
      } else {
        part.resize(words);
        s->device->maskBatch(prog, rows.data(), n, part.data());
        for (size_t w = 0; w < words; ++w) mask[w] &= part[w];
      }
    }
    // the cells the masks stand for, early exits included
    s->device->perf.acceptCells += n * (int64_t)m.B * num_goals;
    return CCMI_OK;
  });
}

extern "C" ccmi_status ccmi_swaps_acceptance_grid(ccmi_session* s, const int32_t* goal_kinds, int32_t num_goals,
                                                  const ccmi_swap_replica* sources, int64_t n,
                                                  const ccmi_swap_replica* candidates, int64_t m, int8_t* codes,
                                                  int64_t* first_invalid) {
  if (first_invalid) *first_invalid = -1;
  return guarded([&] {
    if (!s) throw std::invalid_argument("null session");
    if (num_goals < 0 || n < 0 || m < 0) throw std::invalid_argument("negative count");
    if ((num_goals > 0 && !goal_kinds) || (n > 0 && !sources) || (m > 0 && !candidates) || (n > 0 && m > 0 && !codes))
      throw std::invalid_argument("null argument");
    ccmi::Engine& e = *s->engine;
    // each kind is the session's latest optimization of it, in the caller's order: the code is the first verdict that
    // is not ACCEPT
    std::vector<const ccmi::GoalImpl*> goals;
    const ccmi::GoalImpl* terminal = nullptr;
    for (int g = 0; g < num_goals; ++g) {
      if (ccmi::isIntraGoalKind(goal_kinds[g]))
        throw ccmi::Unsupported("goal kind " + std::to_string(goal_kinds[g]) +
                                " is an intra-broker goal: it shares no chain with inter-broker goals and has no "
                                "swap grid; ccmi_actions_acceptance answers its cells on the host");
      const ccmi::GoalImpl* goal = e.optimizedOfKind(goal_kinds[g]);
      if (!goal) throw std::invalid_argument("the session has not optimized goal kind " + std::to_string(goal_kinds[g]));
      if (!terminal && goal->terminal) terminal = goal;
      goals.push_back(goal);
    }
    if (n == 0 || m == 0) return CCMI_OK;
    if (terminal) throw ccmi::StateError("No goal should be executed after " + terminal->name);
    // every replica against the model before anything runs on the device (the kernel trusts its rows): n + m
    // resolutions, sources first
    const ccmi::Model& md = s->model;
    auto resolve = [&](const ccmi_swap_replica& a, int64_t index) {
      try {
        if (a.partition < 0 || a.partition >= md.P) throw std::invalid_argument("partition out of range");
        if (a.broker < 0 || a.broker >= md.B) throw std::invalid_argument("broker out of range");
        const int r = md.replicaOn(a.partition, a.broker);
        if (r < 0) throw std::invalid_argument("no replica of the partition on the broker");
        return r;
      } catch (std::invalid_argument&) {
        if (first_invalid) *first_invalid = index;
        throw;
      }
    };
    std::vector<ccmi::SwapRow> rows((size_t)n);
    for (int64_t i = 0; i < n; ++i)
      rows[(size_t)i] = ccmi::SwapRow{resolve(sources[i], i), sources[i].partition, sources[i].broker, ccmi::DA_SWAP};
    std::vector<int32_t> cands((size_t)m);
    for (int64_t j = 0; j < m; ++j) cands[(size_t)j] = resolve(candidates[j], n + j);
    const ccmi::ThreadPin pin(s->deviceOrdinal);  // restored when the call returns
    s->model.flushToDevice();  // the rows the host changed since the last launch (ccmi_session_apply, a goal's moves)
    const size_t cells = (size_t)n * (size_t)m;
    std::vector<int8_t> part;
    // one device program per kMaxGoals goals (at least one: without goals, the legitimacy grid). Codes 3 and 4 are the
    // same in every program; a cell still at 0 takes the next program's code
    for (size_t c0 = 0; c0 == 0 || c0 < goals.size(); c0 += ccmi::kMaxGoals) {
      const int G = (int)std::min<size_t>(ccmi::kMaxGoals, goals.size() - c0);
      // every slot is an actionAcceptance column, as in ccmi_actions_acceptance
      ccmi::DevProgram prog;
      std::memset(&prog, 0, sizeof(prog));
      prog.nGoals = G;
      prog.action = ccmi::DA_SWAP;
      for (int g = 0; g < G; ++g) prog.goals[g] = goals[c0 + g]->dg;
      if (c0 == 0) {
        s->device->swapGridBatch(prog, rows.data(), n, cands.data(), m, codes);
      } else {
        part.resize(cells);
        s->device->swapGridBatch(prog, rows.data(), n, cands.data(), m, part.data());
        for (size_t c = 0; c < cells; ++c)
          if (codes[c] == 0) codes[c] = part[c];
      }
    }
    // the cells the codes stand for, early exits included
    s->device->perf.acceptCells += n * m * num_goals;
    return CCMI_OK;
  });
}
