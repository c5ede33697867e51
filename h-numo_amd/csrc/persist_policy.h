// persist_policy.h -- when a suspended persistent sub-cycle path is tried again.
//
// Plain C++17, no HIP call and no engine type: engine.hip includes it for the engine,
// tests/persist_policy_main.cpp for a CPU program that runs under the host sanitizers (tests/test_persist_policy.py).
//
// A persistent launch that found its workgroups not co-resident suspends the path (abort); the engine then runs
// on per-stage launches.  Every run that starts while the path is suspended asks due_for_probe: it spends one run
// of the wait, or, the wait over, asks for a stage-less trial launch whose outcome goes to probed.  The wait
// doubles with every abort and every failed probe, up to 1024 runs, and starts again at 1 after a persistent run
// that completed.  The per-stage redo of an aborted run asks nothing: it spends no run of the wait.
#pragma once
#include <stdint.h>

#include <algorithm>

namespace hnumo {

struct PersistPolicy {
  bool suspended = false;
  int wait = 0, backoff = 1;
  int aborts = 0, reprobes = 0, recovered = 0;

  void back_off() {
    wait = backoff;
    backoff = std::min(2 * backoff, 1024);
  }
  void abort() {
    suspended = true;
    aborts++;
    back_off();
  }
  bool due_for_probe() {
    if (!suspended) return false;
    if (wait > 0) {
      wait--;
      return false;
    }
    reprobes++;
    return true;
  }
  void probed(bool resident) {
    if (!resident) return back_off();
    suspended = false;
    recovered++;
  }
  void completed_persistent() { backoff = 1; }
  // hnumo_persistent_stats: aborts, re-probes, recoveries, runs left before the next re-probe (-1: not suspended)
  void stats(int32_t out[4]) const {
    const int32_t v[4] = {aborts, reprobes, recovered, suspended ? wait : -1};
    std::copy(v, v + 4, out);
  }
};

}  // namespace hnumo
