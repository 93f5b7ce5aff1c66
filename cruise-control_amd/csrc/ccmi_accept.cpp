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
using ccmi::SourceRow;

// ---- the arguments of a call, in the order every entry point refuses them
void checkArguments(const ccmi_session* s, bool negativeCount, bool nullArgument) {
  if (!s) throw std::invalid_argument("null session");
  if (negativeCount) throw std::invalid_argument("negative count");
  if (nullArgument) throw std::invalid_argument("null argument");
}

// ---- the goals of a call
struct GoalList {
  std::vector<const ccmi::GoalImpl*> goals;    // one per kind, in the caller's order
  std::vector<int> devCols;                    // the indices of those the device answers (every one but intra-broker goals)
  const ccmi::GoalImpl* terminal = nullptr;    // the first of the device's goals after which no goal may run
};

// Each kind is the session's latest optimization of it (ccmi_action_acceptance_by_kind); a kind named twice is
// evaluated twice. Intra-broker goals read the disk tables, which the scan kernels do not hold: with `noIntra` null
// they stay in the list for the host to answer, else they are refused as having no `noIntra`.
GoalList resolveGoals(const ccmi::Engine& e, const int32_t* kinds, int32_t n, const char* noIntra) {
  GoalList gl;
  for (int g = 0; g < n; ++g) {
    const bool intra = ccmi::isIntraGoalKind(kinds[g]);
    if (intra && noIntra)
      throw ccmi::Unsupported("goal kind " + std::to_string(kinds[g]) +
                              " is an intra-broker goal: it shares no chain with inter-broker goals and has no " +
                              noIntra + "; ccmi_actions_acceptance answers its cells on the host");
    const ccmi::GoalImpl* goal = e.optimizedOfKind(kinds[g]);
    if (!goal) throw std::invalid_argument("the session has not optimized goal kind " + std::to_string(kinds[g]));
    gl.goals.push_back(goal);
    if (intra) continue;
    gl.devCols.push_back(g);
    if (!gl.terminal && goal->terminal) gl.terminal = goal;
  }
  return gl;
}

[[noreturn]] void throwTerminal(const GoalList& gl) {
  throw ccmi::StateError("No goal should be executed after " + gl.terminal->name);
}

// ---- the rows of a call: indices are checked against the model first (the kernels trust their rows)
// (the throw stays out of line so that the checks, which run once or twice per row, are inlined into the row loops)
[[noreturn]] __attribute__((noinline)) void invalid(const char* what) { throw std::invalid_argument(what); }
inline void checkPartition(const ccmi::Model& m, int p) {
  if (p < 0 || p >= m.P) invalid("partition out of range");
}
inline void checkBroker(const ccmi::Model& m, int b) {
  if (b < 0 || b >= m.B) invalid("broker out of range");
}
// the replica of partition p on broker b; `none` is the caller's word for a broker that holds none
inline int replicaOf(const ccmi::Model& m, int p, int b, const char* none) {
  checkPartition(m, p);
  checkBroker(m, b);
  const int r = m.replicaOn(p, b);
  if (r < 0) invalid(none);
  return r;
}
// f() for the caller's row `index`: an invalid_argument on its way out, and nothing else, makes it *first_invalid
template <class F>
auto atIndex(int64_t* first_invalid, int64_t index, F f) {
  try {
    return f();
  } catch (std::invalid_argument&) {
    if (first_invalid) *first_invalid = index;
    throw;
  }
}

// ---- the device programs of a call
// The device goals [c0, c0 + G) of the list. Every slot is an actionAcceptance column: no slot is the goal being
// optimized. The kernels gather whole records, so the scan programs' operand mask and candidate filters stay clear.
ccmi::DevProgram programOf(const GoalList& gl, size_t c0, int G, int action) {
  ccmi::DevProgram prog;
  std::memset(&prog, 0, sizeof(prog));
  prog.nGoals = G;
  prog.action = action;
  for (int g = 0; g < G; ++g) prog.goals[g] = gl.goals[gl.devCols[c0 + g]]->dg;
  return prog;
}
// run(program, c0, G) for one device program per kMaxGoals device goals; `atLeastOne`: one even without goals
template <class Run>
void forEachProgram(const GoalList& gl, int action, bool atLeastOne, Run run) {
  for (size_t c0 = 0; (atLeastOne && c0 == 0) || c0 < gl.devCols.size(); c0 += ccmi::kMaxGoals) {
    const int G = (int)std::min<size_t>(ccmi::kMaxGoals, gl.devCols.size() - c0);
    run(programOf(gl, c0, G, action), c0, G);
  }
}

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

// The row of action i as Engine::acceptance resolves it; throws what the single call throws.
AcceptRow resolve(const ccmi::Model& m, const ccmi_action& a) {
  if (a.type != CCMI_INTER_BROKER_REPLICA_MOVEMENT && a.type != CCMI_LEADERSHIP_MOVEMENT &&
      a.type != CCMI_INTER_BROKER_REPLICA_SWAP)
    throw std::invalid_argument("Unsupported balancing action " + std::to_string(a.type) + " is provided.");
  checkPartition(m, a.partition);
  checkBroker(m, a.source_broker);
  checkBroker(m, a.destination_broker);  // before the source's replica is looked up
  const int sr = replicaOf(m, a.partition, a.source_broker, "no replica of the partition on the source broker");
  if (a.type == CCMI_INTER_BROKER_REPLICA_SWAP) {
    const int dr = replicaOf(m, a.destination_partition, a.destination_broker,
                             "no replica of the destination partition on the destination broker");
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
    checkArguments(s, num_goals < 0 || n < 0,
                   (num_goals > 0 && !goal_kinds) || (n > 0 && !actions) || (n > 0 && num_goals > 0 && !acceptance));
    ccmi::Engine& e = *s->engine;
    // columns of intra-broker goals are the host's
    const GoalList gl = resolveGoals(e, goal_kinds, num_goals, nullptr);
    if (n == 0 || num_goals == 0) return CCMI_OK;
    const ccmi::ThreadPin pin(s->deviceOrdinal);  // restored when the call returns
    // every error of the single calls, before anything runs on the device
    Resolved moves, swaps;
    for (int64_t i = 0; i < n; ++i) {
      const ccmi_action& a = actions[i];
      atIndex(first_invalid, i, [&] {
        for (int g = 0; g < num_goals; ++g)
          if (ccmi::isIntraGoalKind(gl.goals[g]->kind))
            acceptance[i * num_goals + g] = (int8_t)ccmi::intraAcceptance(*gl.goals[g], e, a);
        if (gl.devCols.empty()) return;
        if (a.type == CCMI_INTRA_BROKER_REPLICA_MOVEMENT || a.type == CCMI_INTRA_BROKER_REPLICA_SWAP)
          throw std::invalid_argument("Unsupported balancing action " + std::to_string(a.type) + " is provided.");
        if (gl.terminal) throwTerminal(gl);
        const AcceptRow row = resolve(s->model, a);
        Resolved& seg = row.action == ccmi::DA_SWAP ? swaps : moves;
        seg.rows.push_back(row);
        seg.index.push_back(i);
      });
    }
    if (gl.devCols.empty()) return CCMI_OK;
    padToWave(moves);
    padToWave(swaps);
    Resolved all = std::move(moves);
    all.nMoveRows = (int64_t)all.rows.size();
    all.rows.insert(all.rows.end(), swaps.rows.begin(), swaps.rows.end());
    all.index.insert(all.index.end(), swaps.index.begin(), swaps.index.end());
    const int64_t nRows = (int64_t)all.rows.size();

    s->model.flushToDevice();  // the rows the host changed since the last launch (ccmi_session_apply, a goal's moves)
    std::vector<int8_t> cells;
    forEachProgram(gl, ccmi::DA_MOVE, false, [&](const ccmi::DevProgram& prog, size_t c0, int G) {
      cells.resize((size_t)nRows * G);
      s->device->acceptBatch(prog, all.rows.data(), nRows, all.nMoveRows, cells.data());
      s->device->perf.acceptCells += n * G;
      for (int64_t r = 0; r < nRows; ++r) {  // back to the caller's order
        const int64_t i = all.index[r];
        if (i < 0) continue;
        for (int g = 0; g < G; ++g) acceptance[i * num_goals + gl.devCols[c0 + g]] = cells[(size_t)r * G + g];
      }
    });
    return CCMI_OK;
  });
}

extern "C" ccmi_status ccmi_moves_acceptance_mask(ccmi_session* s, const int32_t* goal_kinds, int32_t num_goals,
                                                  const ccmi_move_source* sources, int64_t n, uint64_t* mask,
                                                  int64_t* first_invalid) {
  if (first_invalid) *first_invalid = -1;
  return guarded([&] {
    checkArguments(s, num_goals < 0 || n < 0, (num_goals > 0 && !goal_kinds) || (n > 0 && (!sources || !mask)));
    const GoalList gl = resolveGoals(*s->engine, goal_kinds, num_goals, "destination-broker mask");  // a conjunction
    if (n == 0) return CCMI_OK;
    if (gl.terminal) throwTerminal(gl);
    // every source against the model before anything runs on the device
    const ccmi::Model& m = s->model;
    std::vector<SourceRow> rows((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
      const ccmi_move_source& a = sources[i];
      rows[(size_t)i] = atIndex(first_invalid, i, [&] {
        if (a.type != CCMI_INTER_BROKER_REPLICA_MOVEMENT && a.type != CCMI_LEADERSHIP_MOVEMENT)
          throw std::invalid_argument("a move source is a replica movement or a leadership movement, not action type " +
                                      std::to_string(a.type));
        const int sr = replicaOf(m, a.partition, a.source_broker, "no replica of the partition on the source broker");
        return SourceRow{sr, a.partition, a.source_broker,
                         a.type == CCMI_LEADERSHIP_MOVEMENT ? ccmi::DA_LEADERSHIP : ccmi::DA_MOVE};
      });
    }
    const ccmi::ThreadPin pin(s->deviceOrdinal);  // restored when the call returns
    s->model.flushToDevice();  // the rows the host changed since the last launch (ccmi_session_apply, a goal's moves)
    const size_t words = (size_t)n * (size_t)s->device->maskWords();
    std::vector<uint64_t> part;
    // without goals, the legit mask; the programs' masks are ANDed
    forEachProgram(gl, ccmi::DA_MOVE, true, [&](const ccmi::DevProgram& prog, size_t c0, int) {
      if (c0 == 0) {
        s->device->maskBatch(prog, rows.data(), n, mask);
      } else {
        part.resize(words);
        s->device->maskBatch(prog, rows.data(), n, part.data());
        for (size_t w = 0; w < words; ++w) mask[w] &= part[w];
      }
    });
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
    checkArguments(s, num_goals < 0 || n < 0 || m < 0,
                   (num_goals > 0 && !goal_kinds) || (n > 0 && !sources) || (m > 0 && !candidates) ||
                       (n > 0 && m > 0 && !codes));
    // in the caller's order: the code is the first verdict that is not ACCEPT
    const GoalList gl = resolveGoals(*s->engine, goal_kinds, num_goals, "swap grid");
    if (n == 0 || m == 0) return CCMI_OK;
    if (gl.terminal) throwTerminal(gl);
    // every replica against the model before anything runs on the device: n + m resolutions, sources first
    const ccmi::Model& md = s->model;
    auto resolve = [&](const ccmi_swap_replica& a, int64_t index) {
      return atIndex(first_invalid, index,
                     [&] { return replicaOf(md, a.partition, a.broker, "no replica of the partition on the broker"); });
    };
    std::vector<SourceRow> rows((size_t)n);
    for (int64_t i = 0; i < n; ++i)
      rows[(size_t)i] = SourceRow{resolve(sources[i], i), sources[i].partition, sources[i].broker, ccmi::DA_SWAP};
    std::vector<int32_t> cands((size_t)m);
    for (int64_t j = 0; j < m; ++j) cands[(size_t)j] = resolve(candidates[j], n + j);
    const ccmi::ThreadPin pin(s->deviceOrdinal);  // restored when the call returns
    s->model.flushToDevice();  // the rows the host changed since the last launch (ccmi_session_apply, a goal's moves)
    const size_t cells = (size_t)n * (size_t)m;
    std::vector<int8_t> part;
    // without goals, the legitimacy grid. Codes 3 and 4 are the same in every program; a cell still at 0 takes the next
    // program's code
    forEachProgram(gl, ccmi::DA_SWAP, true, [&](const ccmi::DevProgram& prog, size_t c0, int) {
      if (c0 == 0) {
        s->device->swapGridBatch(prog, rows.data(), n, cands.data(), m, codes);
      } else {
        part.resize(cells);
        s->device->swapGridBatch(prog, rows.data(), n, cands.data(), m, part.data());
        for (size_t c = 0; c < cells; ++c)
          if (codes[c] == 0) codes[c] = part[c];
      }
    });
    // the cells the codes stand for, early exits included
    s->device->perf.acceptCells += n * m * num_goals;
    return CCMI_OK;
  });
}
