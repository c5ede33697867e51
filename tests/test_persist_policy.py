"""The suspend / back-off state of the persistent sub-cycle path (h-numo_amd/csrc/persist_policy.h), run on
the CPU.

tests/persist_policy_main.cpp includes the header; this module compiles it once per session with
AddressSanitizer and UBSan into a temporary directory and runs it as a child process on scripted event
sequences.  Nothing is loaded into Python.  After EVERY event every field of the struct, due_for_probe's answer
and the four numbers of hnumo_persistent_stats are compared with the model below, which is written from
include/hnumo_engine.h's words: a launch that gives up suspends the path; after a back-off of 1, 2, 4 ... 1024
runs a trial launch decides; a completed persistent run starts the back-off at 1 again.

Events, as the engine raises them (engine.hip run_with_redo, maybe_reprobe): every run that is not the redo of an
aborted one begins with d (due_for_probe) and, on a yes, the trial launch's r / f (resident or not); a launch that
gives up is a; its per-stage redo asks the policy nothing (x); a persistent run that completes is c."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GXX = shutil.which("g++")
pytestmark = pytest.mark.skipif(GXX is None, reason="no g++ to compile tests/persist_policy_main.cpp with")

CAP = 1024


@pytest.fixture(scope="session")
def policy_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("persist_policy") / "persist_policy_main")
    subprocess.run([GXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(HERE, "persist_policy_main.cpp"), "-o", exe], check=True)
    return exe


class Model:
    """The policy in Python; row() is one output line of persist_policy_main."""

    def __init__(self):
        self.suspended, self.wait, self.backoff = False, 0, 1
        self.aborts = self.reprobes = self.recovered = 0

    def _back_off(self):
        self.wait, self.backoff = self.backoff, min(2 * self.backoff, CAP)

    def event(self, ev):
        """applies one event; due_for_probe's answer, -1 for every other event"""
        if ev == "a":
            self.suspended, self.aborts = True, self.aborts + 1
            self._back_off()
        elif ev == "d":
            if not self.suspended:
                return 0
            if self.wait > 0:
                self.wait -= 1
                return 0
            self.reprobes += 1
            return 1
        elif ev == "r":
            self.suspended, self.recovered = False, self.recovered + 1
        elif ev == "f":
            self._back_off()
        elif ev == "c":
            self.backoff = 1
        else:
            assert ev == "x", ev
        return -1

    def stats(self):
        return {"aborts": self.aborts, "reprobes": self.reprobes, "recovered": self.recovered,
                "wait": self.wait if self.suspended else -1}

    def row(self, due):
        s = self.stats()
        return [int(self.suspended), self.wait, self.backoff, self.aborts, self.reprobes, self.recovered, due,
                s["aborts"], s["reprobes"], s["recovered"], s["wait"]]


def replay(exe, events):
    """Runs the events through the program and the model, compares after every event; the model at the end."""
    r = subprocess.run([exe, events], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])   # (a sanitizer report fails the test)
    rows = [[int(v) for v in ln.split()] for ln in r.stdout.splitlines()]
    assert len(rows) == len(events)
    m = Model()
    for k, (ev, got) in enumerate(zip(events, rows)):
        due = m.event(ev)
        assert got == m.row(due), (k, events[max(0, k - 8):k + 1], got, m.row(due))
    return m


def runs_until_probe(m):
    """the d events of the runs up to and including the one whose trial launch is due (on a copy of m's state)"""
    n, wait = 1, m.wait
    while wait > 0:
        n, wait = n + 1, wait - 1
    return "d" * n


def test_abort_runs_probe_resident(policy_exe):
    # a run starts (d: not suspended), its launch gives up, the redo; one run of the wait; the probe, resident
    m = replay(policy_exe, "dax" + "d" + "dr")
    assert m.stats() == {"aborts": 1, "reprobes": 1, "recovered": 1, "wait": -1}
    assert m.backoff == 2    # (no persistent run has completed yet)


def test_failed_probes_double_the_wait_up_to_the_cap_and_stay_there(policy_exe):
    m, events, waits = Model(), "a", []
    m.event("a")
    for _ in range(12):                       # backoff 2, 4 ... 1024, then 1024 again: one past the cap
        d = runs_until_probe(m)
        for ev in d + "f":
            m.event(ev)
        events += d + "f"
        waits.append(m.wait)
    assert waits == [2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 1024, 1024]
    end = replay(policy_exe, events)
    assert end.stats() == {"aborts": 1, "reprobes": 12, "recovered": 0, "wait": CAP} and end.backoff == CAP
    # the runs between two probes: as many as the wait said
    assert events.count("d") == 12 + 1 + sum(waits[:-1])


def test_backoff_restarts_at_one_after_a_completed_persistent_run(policy_exe):
    recover = "a" + "d" + "dr"
    m = replay(policy_exe, recover + "dc" + "da")
    assert (m.wait, m.backoff) == (1, 2) and m.stats()["aborts"] == 2
    # without a completed persistent run in between the second abort waits twice as long
    m = replay(policy_exe, recover + "da")
    assert (m.wait, m.backoff) == (2, 4)


def test_redo_right_after_an_abort_leaves_the_wait(policy_exe):
    m = replay(policy_exe, "dax")
    assert m.stats() == {"aborts": 1, "reprobes": 0, "recovered": 0, "wait": 1}
    # the next run spends it, the one after probes
    m = replay(policy_exe, "dax" + "d")
    assert m.stats()["wait"] == 0 and m.reprobes == 0
    m = replay(policy_exe, "dax" + "d" + "d")
    assert m.reprobes == 1


def test_sequence_of_the_corrector_abort_test(policy_exe):
    """tests/test_persistent_residency_gpu.py test_corrector_abort_is_redone_and_path_recovers: a step whose
    corrector launch gives up and is redone, a step on per-stage launches, a step that probes, finds the grid
    resident and completes on the persistent path, and one more persistent step."""
    m = replay(policy_exe, "dax")
    assert m.stats() == {"aborts": 1, "reprobes": 0, "recovered": 0, "wait": 1}
    m = replay(policy_exe, "dax" + "d" + "drc" + "dc")
    assert m.stats() == {"aborts": 1, "reprobes": 1, "recovered": 1, "wait": -1}
    assert m.backoff == 1


def test_unknown_event_is_refused(policy_exe):
    assert subprocess.run([policy_exe, "aq"], capture_output=True).returncode == 2
