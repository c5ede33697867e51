// persist_policy_main.cpp -- stand-alone driver of h-numo_amd/csrc/persist_policy.h for
// tests/test_persist_policy.py.
//
//   persist_policy_main EVENTS
//
// EVENTS is a string of one letter per event, applied in order to one PersistPolicy:
//   a abort()   d due_for_probe()   r probed(true)   f probed(false)   c completed_persistent()
//   x nothing: the per-stage redo of an aborted run, which asks the policy nothing
// After every event one line goes to stdout, eleven integers:
//   suspended wait backoff aborts reprobes recovered | due_for_probe's answer (-1: another event) |
//   the four numbers of stats()
// Exit status: 0, or 2 for a usage error or an unknown letter.
#include <cstdint>
#include <cstdio>

#include "../h-numo_amd/csrc/persist_policy.h"

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  hnumo::PersistPolicy p;
  for (const char *e = argv[1]; *e; e++) {
    int due = -1;
    switch (*e) {
      case 'a': p.abort(); break;
      case 'd': due = p.due_for_probe() ? 1 : 0; break;
      case 'r': p.probed(true); break;
      case 'f': p.probed(false); break;
      case 'c': p.completed_persistent(); break;
      case 'x': break;
      default: return 2;
    }
    int32_t s[4] = {-9, -9, -9, -9};  // (every slot must be written)
    p.stats(s);
    printf("%d %d %d %d %d %d %d %d %d %d %d\n", p.suspended ? 1 : 0, p.wait, p.backoff, p.aborts, p.reprobes,
           p.recovered, due, (int)s[0], (int)s[1], (int)s[2], (int)s[3]);
  }
  return 0;
}
