"""Inputs of the marks-summary tests (tests/test_marks_summary_host.py, tests/test_gpu_marks_summary.py) and the host's two statements
of the three coverage numbers.  Nothing here comes from the device.

Statements.  `loops(marks, win)` is the reference's own: percent_recapitulated, percent_recapitulated_forgiving and n_captures of a bare
NavBySceneFamiliarity whose `_host_coverage` is `marks` and whose `_window` gives `win` -- as (covered, furthest, captures) with
furthest the i of the i / n the forgiving loop returns (0 for its 0.).  `restated` is navsim_amd.agent.marks_summary_host, which the CPU
test holds to the loops; the GPU tests use it for slots too long for the loops (> LOOP_LIMIT points).

Planted slots (SLOTS: one straight route (i, 0) of its own per slot, in this order, so slot j's marks begin at byte sum(LENGTHS[:j]) of
the device's array).  With C = marks per thread, T = marks per trip of the kernel, both read from the build's constants:
  0  n = 1          all set
  1  n = 2          mark 0 clear, then a run of win = 1: the capture at p = win; the slot begins at an odd byte
  2  n = C          all clear
  3  n = 64 C - 1   a run from index 0; a run across a thread's chunk edge; runs of 4, 5 and 6 marks (win = 5: one short, exact, one over);
                    a run of exactly 5 ending at n - 1 (the capture in the last admissible place)
  4  n = 64 C + 1   mark 0 clear then a run of 7; a run across the wave edge at 64 C that ends at n - 1
  5  n = T - 1      all set
  6  n = T          marks 0..2 clear, then one run of T - 3 to n - 1: exactly win = T - 3, ending with the trip
  7  n = T + 1      a run from 0 over several wave edges; a run across the trip edge that ends at n - 1
  8  n = 2 T + 3    all set but mark T + 5: two runs that cross trip edges
  9  n = 263 200    runs of W - 1, W and W + 1 marks for W = T + 10 (a window longer than a trip); a run over many trips; a run of
                    exactly W ending at n - 1
Every slot is asked under the windows 0, 1, n - 1, n, n + 5, int(0.05 n) and its planted ones: ENTRIES, so every slot occurs in several
entries of one call with different windows."""
import functools

import numpy as np

from navsim_amd import _native as N
from navsim_amd import NavBySceneFamiliarity
from navsim_amd.agent import marks_summary_host as restated  # noqa: F401

C, T = N.DV_MARKS_PER_THREAD, N.DV_MARKS_PER_TRIP
W = T + 10
LONG = 263200
LENGTHS = (1, 2, C, 64 * C - 1, 64 * C + 1, T - 1, T, T + 1, 2 * T + 3, LONG)
LOOP_LIMIT = 3000

# slot -> the stretches [a, b] (inclusive) planted in it
STRETCHES = {
    0: [(0, 0)],
    1: [(1, 1)],
    2: [],
    3: [(0, 2), (C - 3, C + 2), (40, 43), (50, 54), (60, 65), (64 * C - 6, 64 * C - 2)],
    4: [(1, 7), (64 * C - 5, 64 * C)],
    5: [(0, T - 2)],
    6: [(3, T - 1)],
    7: [(0, 2000), (T - 7, T)],
    8: [(0, T + 4), (T + 6, 2 * T + 2)],
    9: [(100, 100 + W - 2), (10000, 10000 + W - 1), (20000, 20000 + W), (40000, 200000), (LONG - W, LONG - 1)],
}
PLANTED_WINDOWS = {0: [], 1: [], 2: [3], 3: [3, 4, 5, 6, 7], 4: [6, 7, 8], 5: [T - 2, 64 * C], 6: [T - 4, T - 3, T - 2], 7: [8, 9, 2001, 2002],
                   8: [T - 3, T + 5, T + 6], 9: [5, W - 1, W, W + 1, 160001, 160002]}


def routes():
    """One straight route of unit spacing per slot: float64[n, 2] of (i, 0)."""
    return [np.stack([np.arange(n, dtype=np.float64), np.zeros(n)], axis=1) for n in LENGTHS]


def offsets():
    return np.cumsum((0,) + LENGTHS[:-1])


def plant_call():
    """(slots int32, xs, ys, reach): one path_routes_error entry per stretch -- at the stretch's middle with half its length as reach; on
    a straight route of unit spacing the distances are |i - x|, exact in doubles, so exactly the marks a..b are set."""
    slots, xs, reach = [], [], []
    for j in sorted(STRETCHES):
        for a, b in STRETCHES[j]:
            assert 0 <= a <= b < LENGTHS[j]
            slots.append(j)
            xs.append((a + b) / 2.0)
            reach.append((b - a) / 2.0)
    return np.array(slots, dtype=np.int32), np.array(xs), np.zeros(len(xs)), np.array(reach)


@functools.lru_cache(maxsize=None)
def planned_marks():
    """The marks the stretches make, slot by slot (bool arrays, read-only): what the device's marks must read back as."""
    out = []
    for j, n in enumerate(LENGTHS):
        m = np.zeros(n, dtype=bool)
        for a, b in STRETCHES[j]:
            m[a:b + 1] = True
        m.setflags(write=False)
        out.append(m)
    return tuple(out)


def windows_of(slot):
    n = LENGTHS[slot]
    return sorted(set([0, 1, n - 1, n, n + 5, int(0.05 * n)] + PLANTED_WINDOWS[slot]))


def entries():
    """(slots int32[k], windows int64[k]): every slot under each of its windows, the slots interleaved."""
    pairs = [(j, w) for j in range(len(LENGTHS)) for w in windows_of(j)]
    pairs.sort(key=lambda p: (p[1] % 7, p[0], p[1]))                # (neighbouring entries are of different slots)
    return np.array([p[0] for p in pairs], dtype=np.int32), np.array([p[1] for p in pairs], dtype=np.int64)


class _Bare(NavBySceneFamiliarity):
    """The agent's three methods over given marks and a given window: nothing else of the agent is made."""
    def __init__(self, marks, win):
        self._host_coverage, self.training_path, self._win = np.asarray(marks, dtype=bool), np.zeros((len(marks), 2)), win

    def _window(self, n_consecutive_scenes):
        return self._win


def loops(marks, win):
    """(covered, furthest, captures) by the reference's loops; also checks furthest / n against the value the loop returned."""
    a = _Bare(marks, win)
    n = len(marks)
    forgiving = a.percent_recapitulated_forgiving()
    furthest = int(round(forgiving * n))
    assert furthest / n == forgiving
    assert a.percent_recapitulated == np.count_nonzero(marks) / n
    return int(np.count_nonzero(marks)), furthest, int(a.n_captures())


def expected(marks_by_slot, slots, windows):
    """int64[k, 3] for the entries, over the marks given (those read back from the device): the loops for slots of up to LOOP_LIMIT
    points, the restatement beyond; each (slot, window) worked out once."""
    out = np.empty((len(slots), 3), dtype=np.int64)
    memo = {}
    for e, (j, w) in enumerate(zip(np.asarray(slots).tolist(), np.asarray(windows).tolist())):
        if (j, w) not in memo:
            m = marks_by_slot[j]
            memo[(j, w)] = loops(m, w) if len(m) <= LOOP_LIMIT else restated(m, w)
        out[e] = memo[(j, w)]
    return out
