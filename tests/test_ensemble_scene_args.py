"""CPU tests of per-member scene_familiarity in ensembles (no GPU): the C ABI declares, the built library exports and the binding
carries the batched calls that keep the per-view minimum per agent; NavEnsemble takes tracking members when its engine offers the
call, leaves its step as it was and works the rows out when they are read.

The ensemble logic runs here over a TEST-ONLY engine that senses with the host sensor model and scores with the oracle, so that the
rows can be compared with agents stepping alone on the oracle plug-in (the reference's own loop, NavBySceneFamiliarity.py:283-303)."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from navsim_amd import synth
from oracle import oracle
from tests.conftest import REPO

NEW = ("dv_sense_step_batch_scene", "dv_step_batch_scene")


def test_scene_batch_calls_are_declared_exported_and_bound():
    header = open(os.path.join(REPO, "include", "dejavu.h")).read()
    lib = ctypes.CDLL(N.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in N.PROTOTYPES, name
    # ..._weighted's arguments with scene_fam behind the records
    for name, old in zip(NEW, ("dv_sense_step_batch_weighted", "dv_step_batch_weighted")):
        assert N.PROTOTYPES[name][0] is ctypes.c_int
        assert N.PROTOTYPES[name][1] == N.PROTOTYPES[old][1] + [N._f64p], name
    # the earlier entry points are as they were
    assert len(N.PROTOTYPES["dv_sense_step_batch_weighted"][1]) == 9 and len(N.PROTOTYPES["dv_step_batch_weighted"][1]) == 7
    for name in ("sense_step_batch_scene", "step_batch_scene"):
        assert callable(getattr(navsim_amd.FamiliarityEngine, name)), name


def _member(eng, track):
    return SimpleNamespace(_engine=eng, track_scene_familiarity=track, familiarity_model=SimpleNamespace(chem_weight=0.25), chem_weight=None,
                           step_size=1.0, landscape=None, _sensor_r=1, angle_offsets=np.zeros(2), training_path=None)


def test_tracking_members_need_an_engine_with_the_call():
    without = SimpleNamespace(sense_step_batch=lambda *a, **k: None)
    with pytest.raises(ValueError, match="track_scene_familiarity=False: a batched pass keeps no per-view minimum"):
        navsim_amd.NavEnsemble([_member(without, True), _member(without, False)])
    navsim_amd.NavEnsemble([_member(without, False), _member(without, False)])           # as before
    with_call = SimpleNamespace(sense_step_batch=lambda *a, **k: None, sense_step_batch_scene=lambda *a, **k: None)
    ens = navsim_amd.NavEnsemble([_member(with_call, True), _member(with_call, True)])
    assert len(ens.agents) == 2
    mixed = navsim_amd.NavEnsemble([_member(with_call, True), _member(with_call, False)])
    with pytest.raises(ValueError, match="track_scene_familiarity=True"):
        mixed.scene_familiarity()                                                        # one array for ALL members needs all tracking


class HostEngine(object):
    """Senses with an agent's host sensor model and scores with the oracle; records every call made to it."""

    def __init__(self, sensor_agent, chem_weight, with_scene_call=True, sense_error_at=None):
        self.agent, self.cw, self.calls, self.sense_error_at = sensor_agent, chem_weight, [], sense_error_at
        if with_scene_call:
            self.sense_step_batch_scene = self._scene

    def sense(self, x, y, angle):                                      # (a member stepping on its own senses through its engine)
        return np.stack([self.agent.get_sensor_mat((x[i], y[i]), angle[i]) for i in range(len(x))])

    def _steps(self, x, y, angles, chem_weights, want_scene):
        lib = self.agent.familiar_scenes
        out = []
        for i in range(len(x)):
            if self.sense_error_at is not None and (float(x[i]), float(y[i])) == self.sense_error_at:
                out.append(None)
                continue
            patches = np.stack([self.agent.get_sensor_mat((x[i], y[i]), a) for a in angles[i]])
            out.append(oracle.step(lib, patches, self.cw if chem_weights is None else chem_weights[i], want_scene=want_scene))
        return out

    def sense_step_batch(self, x, y, angles, force_resolve=False, chem_weights=None):
        self.calls.append(("sense_step_batch", np.asarray(x).tolist(), np.asarray(y).tolist(), np.asarray(angles).tolist(),
                           None if chem_weights is None else np.asarray(chem_weights).tolist()))
        A = len(angles[0])
        return [dict(flags=16, best_idex=0, angle_familiarity=np.zeros(A)) if r is None else dict(r, flags=0)
                for r in self._steps(x, y, angles, chem_weights, False)]

    def _scene(self, x, y, angles, force_resolve=False, chem_weights=None):
        self.calls.append(("sense_step_batch_scene", np.asarray(x).tolist(), np.asarray(y).tolist(), np.asarray(angles).tolist(),
                           None if chem_weights is None else np.asarray(chem_weights).tolist()))
        res = self._steps(x, y, angles, chem_weights, True)
        return SimpleNamespace(scene_familiarity=np.stack([r["scene_familiarity"] for r in res]))


LAND = synth.synth_landscape(5, 200, 4)
PATH = np.stack([np.linspace(50, 150, 40), np.full(40, 100.0)], axis=1)
KW = dict(n_test_angles=4, n_sensor_levels=5, use_gpu_sensor=False)


def _trained(track=True):
    nsf = navsim_amd.NavBySceneFamiliarity(LAND, (8, 8), 2.0, familiarity_model=oracle.sads_familiarity(0.25), track_scene_familiarity=track, **KW)
    nsf.train_from_path(PATH)
    return nsf


def _ensemble(poses, track=True, **engine_kw):
    nsf = _trained(track)
    nsf._engine = HostEngine(_trained(), 0.25, **engine_kw)          # (the host agent's sensor model behind the engine's batched call)
    return navsim_amd.NavEnsemble.from_agent(nsf, poses)


POSES = [((60.0, 100.5), 0.1), ((80.0, 99.0), 6.1), ((100.0, 101.0), 0.3), ((3.0, 100.0), 0.0), ((120.0, 100.0), 0.2)]   # member 3: inside the bounds margin


def test_members_rows_equal_agents_stepping_alone_and_the_step_is_unchanged():
    ens = _ensemble(POSES)
    plain = _ensemble(POSES, track=False, with_scene_call=False)
    assert all(a.track_scene_familiarity for a in ens.agents)                            # from_agent / clone_for_ensemble carry it over
    assert not any(a.track_scene_familiarity for a in plain.agents)
    alone = []
    for pos, ang in POSES:
        a = _trained()
        a.position, a.angle = pos, ang
        alone.append(a)
    F = len(PATH)
    # before any step: zeros, as after train_from_path; no device work
    assert ens.scene_familiarity().shape == (len(POSES), F) and not ens.scene_familiarity().any()
    assert ens.engine.calls == []
    for t in range(6):
        ens.step_forward()
        plain.step_forward()
        for a in alone:
            if a.stopped_with_exception is None:
                try:
                    a.step_forward()
                except navsim_amd.StopNavigationException as e:
                    a.stopped_with_exception = e
        # the engine saw the calls of an ensemble that tracks nothing, and nothing else
        assert ens.engine.calls == plain.engine.calls and {c[0] for c in ens.engine.calls} == {"sense_step_batch"}
        if t in (0, 2, 5):
            n_calls = len(ens.engine.calls)
            rows = ens.scene_familiarity()
            assert rows.dtype == np.float64 and rows.shape == (len(POSES), F)
            assert [c[0] for c in ens.engine.calls[n_calls:]] == ["sense_step_batch_scene"]      # all members in ONE call
            assert len(ens.engine.calls[n_calls][1]) == 4                                        # ... the four that were scored
            for i, (m, a) in enumerate(zip(ens.agents, alone)):
                assert m.position == a.position and m.angle == a.angle, (t, i)
                assert m.scene_familiarity.tobytes() == a.scene_familiarity.tobytes(), (t, i)
                assert rows[i].tobytes() == a.scene_familiarity.tobytes(), (t, i)
            assert np.isinf(rows[3]).all() and ens.stop_status[3] == navsim_amd.OutOfLandscapeBoundsException().get_code()
            again = ens.scene_familiarity()                                                      # no device work until the next step
            assert again.tobytes() == rows.tobytes() and again is not rows and len(ens.engine.calls) == n_calls + 1
            del ens.engine.calls[n_calls:]
    assert [a.position for a in ens.agents] == [a.position for a in plain.agents]                # tracking changes nothing else


def test_one_member_reads_its_row_and_the_others_come_with_it():
    ens = _ensemble(POSES[:3])
    ens.step_forward()
    ens.step_forward()
    a = _trained()
    a.position, a.angle = POSES[1]
    a.step_forward()
    a.step_forward()
    assert ens.agents[1].scene_familiarity.tobytes() == a.scene_familiarity.tobytes()
    assert [c[0] for c in ens.engine.calls] == ["sense_step_batch", "sense_step_batch", "sense_step_batch_scene"]
    assert all(m._scene_stale is None for m in ens.agents)
    ens.agents[0].scene_familiarity, ens.agents[2].scene_familiarity, ens.scene_familiarity()
    assert len(ens.engine.calls) == 3
    # a member that steps on its own afterwards: the ensemble's array shows its row as it is now, and a caller's writes stay its own
    before = ens.scene_familiarity()
    before[2, :] = -1.0
    ens.agents[0].step_forward()
    a0 = _trained()
    a0.position, a0.angle = POSES[0]
    for _ in range(3):
        a0.step_forward()
    after = ens.scene_familiarity()
    assert after[0].tobytes() == a0.scene_familiarity.tobytes() and after[0].tobytes() != before[0].tobytes()
    assert after[1].tobytes() == before[1].tobytes() and (after[2] != -1.0).all()


def test_stopped_members_keep_their_rows_and_a_sense_error_leaves_inf():
    poses = [POSES[0], ((148.0, 100.0), 0.0), POSES[2]]                                  # member 1 reaches the end of the path at once
    ens = _ensemble(poses, sense_error_at=(100.0, 101.0))                                # member 2's footprint "leaves the landscape"
    assert ens.step_forward() == [0]
    assert ens.stop_status[1] == 1 and ens.stop_status[2] == navsim_amd.NavEnsemble.SENSE_ERROR_STATUS
    first = ens.scene_familiarity().copy()
    assert np.isfinite(first[:2]).all() and np.isinf(first[2]).all()
    a = _trained()
    a.position, a.angle = poses[1]
    with pytest.raises(navsim_amd.ReachedEndOfTrainingPathException):
        a.step_forward()
    assert first[1].tobytes() == a.scene_familiarity.tobytes()
    ens.step_forward()
    rows = ens.scene_familiarity()
    assert ens.engine.calls[-1][0] == "sense_step_batch_scene" and len(ens.engine.calls[-1][1]) == 1     # only the member that stepped
    assert rows[1].tobytes() == first[1].tobytes() and np.isinf(rows[2]).all() and rows[0].tobytes() != first[0].tobytes()


def test_members_weights_go_with_the_poses():
    nsf = _trained()
    nsf._engine = HostEngine(_trained(), 0.25)
    ens = navsim_amd.NavEnsemble.from_agent(nsf, POSES[:3])
    for a, w in zip(ens.agents, (0.25, 0.0, 1.0)):
        a.chem_weight = w
    ens = navsim_amd.NavEnsemble(ens.agents)
    ens.step_forward()
    rows = ens.scene_familiarity()
    step, read = ens.engine.calls
    assert step[4] == read[4] == [0.25, 0.0, 1.0] and step[1:4] == read[1:4]             # the poses, headings and weights of the step
    lib = nsf.familiar_scenes
    for i, w in enumerate((0.25, 0.0, 1.0)):
        patches = np.stack([ens.engine.agent.get_sensor_mat(POSES[i][0], a) for a in read[3][i]])
        assert rows[i].tobytes() == oracle.step(lib, patches, w)["scene_familiarity"].tobytes()
