"""CPU tests of the per-agent chem_weight surface (no GPU): the C ABI declares and the binding carries the weighted calls, and the
Python side refuses malformed weights before anything reaches a device."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import navsim_amd
from navsim_amd import _native as N
from navsim_amd import synth
from navsim_amd.engine import agent_weights
from oracle import oracle
from tests.conftest import REPO


def test_weighted_calls_are_declared_and_bound():
    header = open(os.path.join(REPO, "include", "dejavu.h")).read()
    for name in ("dv_set_weight_range", "dv_step_batch_weighted", "dv_sense_step_batch_weighted"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in N.PROTOTYPES, name
    # the weights ride between n_headings and flags, as a double pointer
    assert N.PROTOTYPES["dv_step_batch_weighted"][1][4] is N._f64p
    assert N.PROTOTYPES["dv_sense_step_batch_weighted"][1][6] is N._f64p
    # dv_lib_info reports the range the layout serves, behind the fields it had
    names = [f[0] for f in N.LibInfo._fields_]
    assert names[-2:] == ["weight_lo", "weight_hi"]
    assert N.LibInfo.weight_lo.offset == N.LibInfo.reserved0.offset + 4 and ctypes.sizeof(N.LibInfo) % 8 == 0


def test_agent_weights_argument():
    assert agent_weights(None, 3) is None
    w = agent_weights([0, 0.25, 1], 3)
    assert w.dtype == np.float64 and w.flags["C_CONTIGUOUS"] and w.tolist() == [0.0, 0.25, 1.0]
    with pytest.raises(ValueError, match="2 weights for 3 agents"):
        agent_weights([0.0, 0.5], 3)


def test_from_agent_refuses_malformed_weights():
    agent = SimpleNamespace(familiarity_model=SimpleNamespace(chem_weight=0.0), _engine=None, training_path=None)
    poses = [((1.0, 2.0), 0.0), ((3.0, 4.0), 0.5)]
    with pytest.raises(ValueError, match="2 poses"):
        navsim_amd.NavEnsemble.from_agent(agent, poses, chem_weights=[0.5])
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        navsim_amd.NavEnsemble.from_agent(agent, poses, chem_weights=[0.5, 1.5])
    with pytest.raises(ValueError, match="GPU"):
        navsim_amd.NavEnsemble.from_agent(agent, poses, chem_weights=[0.5, 0.0])


def test_ensemble_sends_each_members_weight():
    """Members' own weights (None: the library's) become the ensemble's per-member array, passed for the active members only."""
    eng = SimpleNamespace()
    model = SimpleNamespace(chem_weight=0.25)

    def member(w):
        return SimpleNamespace(_engine=eng, track_scene_familiarity=False, familiarity_model=model, chem_weight=w, step_size=1.0,
                               landscape=None, _sensor_r=1, angle_offsets=np.zeros(2), training_path=None)
    ens = navsim_amd.NavEnsemble([member(None), member(0.0), member(1.0)])
    assert ens._weights.tolist() == [0.25, 0.0, 1.0]
    assert navsim_amd.NavEnsemble([member(None), member(None)])._weights is None


def test_a_foreign_weight_member_refuses_to_step_alone():
    land = synth.synth_landscape(5, 200, 4)
    nsf = navsim_amd.NavBySceneFamiliarity(land, (8, 8), 2.0, n_test_angles=4, familiarity_model=oracle.sads_familiarity())
    path = np.stack([np.linspace(50, 150, 40), np.full(40, 100.0)], axis=1)
    nsf.train_from_path(path)
    nsf.position, nsf.angle = (60.0, 100.0), 0.0
    nsf.chem_weight = 0.5                                            # the plug-in's library carries no weight of its own
    with pytest.raises(ValueError, match="NavEnsemble"):
        nsf.step_forward()
    nsf.chem_weight = None
    nsf.step_forward()
    assert nsf.navigated_for_frames == 1
