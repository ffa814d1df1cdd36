"""Ensembles of agents on one GPU: the reference farms independent trials over MPI ranks
(scripts/run_experiment.py:326-347); here N agents that share a landscape and a trained library step in lockstep,
and the device work of 64/A of them shares each pass over the library (dv_sense_step_batch).

Every agent is a full navsim_amd.NavBySceneFamiliarity (own pose, error metrics, stop conditions); only the sensing
and scoring of a step are batched.  An agent that stops (end of path, out of bounds, too far) keeps its final state
and no longer takes part.

Members may score under chem_weights of their own (the experiment grid's chem_weight variable, scripts/run_experiment.py:61,218):
a trial's training views do not depend on the weight, so one library serves every weight its layout stores the sums for
(FamiliarityEngine.set_weight_range), and the members of all weights share the library passes (dv_sense_step_batch_weighted).

Members may track scene_familiarity (the constructor's default, the reference's agent).  The ensemble's step is the same either way:
it only remembers, per tracking member, the pose, candidate headings and weight of the step it last took.  When a member's
`scene_familiarity` -- or NavEnsemble.scene_familiarity() for all members -- is read, those poses are sensed once more and the
per-view minimum over each member's OWN headings comes back from shared library passes (dv_sense_step_batch_scene), as the
single agent works its minimum out when it is read.
"""
import numpy as np

from .agent import StopNavigationException, OutOfLandscapeBoundsException, coverage_row
from .util import reject_infomax, reject_mushroom, reject_ncc, reject_banked, route_ensemble_name


class NavEnsemble(object):
    _metrics_on_slots = True     # the members' error metrics run on the device's path slots (they hold ONE training path)

    def __init__(self, agents):
        if not agents:
            raise ValueError("no agents")
        for a in agents:
            self._check_member(a)
        eng = agents[0]._engine
        if eng is None or any(a._engine is not eng for a in agents):
            raise ValueError("the agents of an ensemble share one engine (NavEnsemble.from_agent)")
        if any(a.track_scene_familiarity for a in agents) and not hasattr(eng, "sense_step_batch_scene"):
            raise ValueError("construct the agents with track_scene_familiarity=False: a batched pass keeps no per-view minimum")
        self.agents = list(agents)
        self.engine = eng
        # per-member weights (a member's own `chem_weight`; None: the library's): sent with every batch when any member has one
        lib_w = getattr(agents[0].familiarity_model, "chem_weight", None)
        own = [getattr(a, "chem_weight", None) for a in agents]
        self._weights = None if all(w is None for w in own) else np.array([lib_w if w is None else w for w in own], dtype=np.float64)
        self.stop_status = [0] * len(agents)                      # the reference's codes: 0 running / 1 / -1 / -2
        # update_error (:252-276) of all members in ONE device call per ensemble step: every member gets a coverage array of its own on
        # the device (dv_path_slots) and hands its position in; 32 members x a NumPy pass over 50 000 training points each were
        # ~10 ms of host time beside a 0.85 ms device step
        # members made alike (from_agent: clones) have their candidate headings and the poses those lead to worked out as arrays for
        # all members at once (NumPy's elementwise loops give an element what they give the scalar)
        a0 = agents[0]
        self._uniform = all(a.step_size == a0.step_size and a.landscape is a0.landscape and a._sensor_r == a0._sensor_r and
                            np.array_equal(a.angle_offsets, a0.angle_offsets) for a in agents)
        self._stepping = False
        self._pending = []                                        # members whose position awaits its metrics
        self._too_far = {}
        if self._metrics_on_slots and agents[0].training_path is not None and hasattr(eng, "path_slots") and all(a.training_path is agents[0].training_path for a in agents):
            for a in self.agents:
                if getattr(a, "_metrics_on_device", False):
                    a._collect_errors()                           # (answers still outstanding from steps it took on its own)
            if not any(getattr(a, "_metrics_on_device", False) for a in self.agents):
                eng.set_training_path(agents[0].training_path)    # (the engine holds the path already where an agent's metrics ran on it)
            eng.path_slots(len(agents))
            for j, a in enumerate(self.agents):
                a._metric_slot, a._ens = j, self
                a._metrics_on_device = False

    @classmethod
    def _check_member(cls, agent):
        """Raises ValueError for an agent this kind of ensemble cannot step."""
        reject_banked(agent, cls.__name__)
        reject_infomax(agent, "NavEnsemble")

    def _device_step(self, idx, xs, ys, angs):
        """The one device call of an ensemble step: members `idx` at (xs, ys) looking along angs[k] -> engine.BatchResults."""
        return self.engine.sense_step_batch(xs, ys, angs, chem_weights=None if self._weights is None else self._weights[idx])

    def _want_error(self, agent):
        self._pending.append((agent, agent.position[0], agent.position[1]))

    def _drop_errors(self, agent):
        self._pending = [p for p in self._pending if p[0] is not agent]

    def _flush_errors(self, raise_for=None):
        """The metrics of every position handed in since the last flush; a member too far from the path is remembered (_too_far) for
        the ensemble's step to stop it as the reference's update_error would have (:264) -- or raised at once for `raise_for`, a
        member stepping on its own."""
        if not self._pending:
            return
        pend, self._pending = self._pending, []
        nearest = self._metrics_call(pend)
        for (a, _, _), d in zip(pend, nearest.tolist()):
            try:
                a._take_error(d)
            except StopNavigationException as e:
                if a is raise_for:
                    raise
                self._too_far[id(a)] = e

    # What a member's slot on the device is asked: the members' agents go through these, so that every kind of ensemble issues the
    # engine calls of ITS slots (here: the one training path's, dv_path_slots).
    def _metrics_call(self, pend):
        """update_error of the (member, x, y) of `pend` in one device call -> the distances to the nearest training point."""
        a0 = pend[0][0]
        return self.engine.path_error_batch([a._metric_slot for a, _, _ in pend], [x for _, x, _ in pend], [y for _, _, y in pend],
                                            a0.coverage_threshold_factor * a0.step_size)

    def _read_marks(self, agent):
        return self.engine.path_coverage_slot(agent._metric_slot, len(agent.training_path))

    def _reset_marks(self, agent):
        self.engine.path_reset_slot(agent._metric_slot)

    _summary_call = "marks_summary_slots"     # the engine call `_marks_summary` makes

    def _marks_summary(self, members, windows):
        """int64[n, 3]: (covered, furthest, captures) of every member's slot under its own window, in one device call."""
        return self.engine.marks_summary_slots([a._metric_slot for a in members], windows)

    def coverage_summary(self, n_consecutive_scenes=0.05):
        """One {"path_coverage", "percent_forgiving", "n_captures"} per member: what its percent_recapitulated,
        percent_recapitulated_forgiving(n_consecutive_scenes) and n_captures(n_consecutive_scenes) give.  The members whose marks lie in
        a slot on the device are all answered by ONE device call, each under the window of its own route's length; a member without a
        slot, and every member where the engine has no such call, by its own three methods."""
        if n_consecutive_scenes < 0:
            raise ValueError("n_consecutive_scenes must be >= 0, got %r" % (n_consecutive_scenes,))
        rows = [None] * len(self.agents)
        held = [i for i, a in enumerate(self.agents) if getattr(a, "_metric_slot", None) is not None and getattr(a, "_ens", None) is self
                and a.training_path is not None]
        if held and callable(getattr(self.engine, self._summary_call, None)):
            self._flush_errors()
            members = [self.agents[i] for i in held]
            got = self._marks_summary(members, [a._window(n_consecutive_scenes) for a in members])
            for i, a, (covered, furthest, captures) in zip(held, members, got.tolist()):
                rows[i] = coverage_row(covered, furthest, captures, len(a.training_path))
        for i, a in enumerate(self.agents):
            if rows[i] is None:
                rows[i] = {"path_coverage": a.percent_recapitulated,
                           "percent_forgiving": a.percent_recapitulated_forgiving(n_consecutive_scenes=n_consecutive_scenes),
                           "n_captures": a.n_captures(n_consecutive_scenes=n_consecutive_scenes)}
        return rows

    @classmethod
    def from_agent(cls, agent, poses, chem_weights=None):
        """`agent`: trained, with the GPU sensor model; poses: iterable of ((x, y), angle), one agent each
        (the first pose goes to `agent` itself, the others to clones on the same engine and library).
        chem_weights (optional, one per pose): member i scores under chem_weights[i], kept as its `chem_weight`.  When the resident
        library's layout does not store the sums those weights need, it is ingested once more from agent.familiar_scenes, laid out
        for the range of weights (the agent's own weight stays the library's: that of its unweighted steps)."""
        cls._check_member(agent)
        poses = list(poses)
        weights = None
        if chem_weights is not None:
            weights = [float(w) for w in chem_weights]
            if len(weights) != len(poses):
                raise ValueError("chem_weights holds %d weights for %d poses" % (len(weights), len(poses)))
            if not all(0.0 <= w <= 1.0 for w in weights):
                raise ValueError("chem_weights must lie in [0, 1], got %r" % (weights,))
            lib_w = float(agent.familiarity_model.chem_weight)
            eng = agent._engine
            if eng is None or agent.training_path is None:
                raise ValueError("clone a trained agent whose sensor model runs on the GPU")
            lo, hi = eng.library_info()["weight_range"]
            if not all(lo <= w <= hi for w in weights):
                eng.set_weight_range(min(weights + [lib_w]), max(weights + [lib_w]))
                try:
                    eng.set_library(agent.familiar_scenes, lib_w)
                finally:
                    eng.set_weight_range(1.0, 0.0)              # later ingests: their own weight alone, as before
        agents = [agent] + [agent.clone_for_ensemble() for _ in poses[1:]]
        for i, (a, (pos, ang)) in enumerate(zip(agents, poses)):
            a.position = (float(pos[0]), float(pos[1]))
            a.angle = float(ang)
            a.chem_weight = None if weights is None else weights[i]
        return cls(agents)

    # ---- scene_familiarity of tracking members: worked out when it is read -------------------------------------
    def _note_scene(self, agent, x, y, headings, weight):
        """`agent` has just been scored at (x, y) along `headings` under `weight`: what its scene_familiarity is made from when read."""
        agent._scene_stale = (x, y, headings, weight)
        agent._scene_owner = self
        agent._scene_is_inf = False

    def _scene_inf(self, agent):
        """`agent` stopped before it was scored: the reference had reset the array to +inf before it sensed (:287)."""
        if agent.track_scene_familiarity:
            agent._scene_stale = None                         # (whatever was left to work out belonged to the step before)
            agent._scene_owner = None
            agent._scene_fam[:] = np.inf
            agent._scene_is_inf = True

    def _read_scene(self):
        """The per-view minima every member's last step left to work out, all members in shared library passes."""
        todo = [a for a in self.agents if a._scene_stale is not None and a._scene_owner is self]
        if not todo:
            return
        st = [a._scene_stale for a in todo]
        weights = None if all(t[3] is None for t in st) else [t[3] for t in st]
        res = self.engine.sense_step_batch_scene([t[0] for t in st], [t[1] for t in st], np.stack([t[2] for t in st]), chem_weights=weights)
        for a, row in zip(todo, res.scene_familiarity):
            a._scene_stale = None
            a._scene_owner = None
            a._scene_fam[:] = row

    def scene_familiarity(self):
        """float64[n_members, F]: every member's scene_familiarity after its last step (members that never stepped: zeros, as after
        train_from_path; stopped before sensing: inf; stopped members keep the row of their last step).  The device work is done once
        per step (the members keep their rows); the array handed out is the caller's own copy, stacked from the members' rows as they
        are now -- also of a member that has stepped on its own since."""
        if any(not a.track_scene_familiarity for a in self.agents):
            raise ValueError("construct the agents with track_scene_familiarity=True (the default) to read scene_familiarity")
        self._read_scene()
        return np.stack([a.scene_familiarity for a in self.agents])

    SENSE_ERROR_STATUS = -3      # not one of the reference's codes: its trial would have died of an IndexError

    def _stop(self, i, exc):
        self.stop_status[i] = exc.get_code() if hasattr(exc, "get_code") else self.SENSE_ERROR_STATUS
        self.agents[i].stopped_with_exception = exc

    def step_forward(self, fake=False):
        """One step of every running agent; returns the indices that are still running afterwards."""
        self._stepping = True
        try:
            return self._step_forward(fake)
        finally:
            self._stepping = False

    def _step_forward(self, fake):
        idx, xs, ys, angs = [], [], [], []
        cands = None
        act = self.active
        if self._uniform and act:
            a0 = self.agents[act[0]]
            b = a0._bounds_tuple()
            px = np.array([self.agents[i].position[0] for i in act], dtype=np.float64)
            py = np.array([self.agents[i].position[1] for i in act], dtype=np.float64)
            ang = np.array([self.agents[i].angle for i in act], dtype=np.float64)
            out = (px <= b[0]) | (py <= b[0]) | (px >= b[1]) | (py >= b[2])        # the bounds test of :153-158, before anything is sensed
            for k in np.nonzero(out)[0].tolist():
                self.agents[act[k]].angle_familiarity[:] = np.nan
                self._scene_inf(self.agents[act[k]])
                self._stop(act[k], OutOfLandscapeBoundsException())
            keep = np.nonzero(~out)[0]
            idx = [act[k] for k in keep.tolist()]
            if idx:
                xs, ys = px[keep], py[keep]
                cand_angle = (ang[keep][:, None] + a0.angle_offsets[None, :]) % (2 * np.pi)
                angs = cand_angle
                cands = (cand_angle, xs[:, None] + a0.step_size * np.cos(cand_angle), ys[:, None] + a0.step_size * np.sin(cand_angle))
        else:
            for i in act:
                try:
                    x, y, a = self.agents[i].headings_to_test()
                except StopNavigationException as e:              # out of the landscape before anything is sensed
                    self._scene_inf(self.agents[i])
                    self._stop(i, e)
                    continue
                idx.append(i); xs.append(x); ys.append(y); angs.append(a)
            if idx:
                angs = np.stack(angs)
        if idx:
            stops = {}
            results = self._device_step(idx, xs, ys, angs)
            # the records as arrays when the engine offers them (engine.BatchResults): no dictionary per agent and step
            lean = hasattr(results, "angle_familiarity")
            flags = results.flags.tolist() if lean else [r["flags"] for r in results]
            best = results.best_idex.tolist() if lean else None
            for k, i in enumerate(idx):
                if flags[k] & 16:                                 # DV_RES_SENSE_ERROR: this agent's footprint left the
                    # landscape (a corner reaches r*sqrt(2) > r past the bounds test); the reference's trial ends in an
                    # IndexError, the other trials go on
                    if cands is not None:
                        self.agents[i].angle_familiarity[:] = np.nan      # (headings_to_test's reset, :285)
                    self._scene_inf(self.agents[i])
                    self._stop(i, IndexError("sensor footprint reaches past the end of the landscape (index out of bounds)"))
                    continue
                if self.agents[i].track_scene_familiarity:
                    self._note_scene(self.agents[i], xs[k], ys[k], angs[k], None if self._weights is None else self._weights[i])
                try:
                    if lean:
                        self.agents[i].apply_step_arrays(results.angle_familiarity[k], best[k], fake,
                                                         None if cands is None else (cands[0][k], cands[1][k], cands[2][k]))
                    else:
                        self.agents[i].apply_step_result(results[k], fake)
                except StopNavigationException as e:
                    stops[i] = e
            # the members' error metrics, all in one device call; the reference takes them BEFORE its end-of-path test (:324-328), so
            # "too far from the path" wins where both would stop a member
            self._flush_errors()
            for i in idx:
                e = self._too_far.pop(id(self.agents[i]), None) or stops.get(i)
                if e is not None and self.stop_status[i] == 0:
                    self._stop(i, e)
        return self.active

    _frames_left = None          # run() with a count per member: the steps each member may still take

    @property
    def active(self):
        left = self._frames_left
        return [i for i, s in enumerate(self.stop_status) if s == 0 and self.agents[i].stopped_with_exception is None and
                (left is None or left[i] > 0)]

    def run(self, frames):
        """Up to `frames` steps -- an int, or one count per member; returns the per-agent number of completed steps.  A member that has
        taken its count steps no more and keeps stop_status 0."""
        if isinstance(frames, (int, np.integer)):
            frames = [int(frames)] * len(self.agents)
        else:
            frames = [int(f) for f in frames]
            if len(frames) != len(self.agents):
                raise ValueError("frames holds %d counts for %d members" % (len(frames), len(self.agents)))
        done = [0] * len(self.agents)
        self._frames_left = list(frames)
        try:
            for _ in range(max(frames + [0])):
                before = self.active
                if not before:
                    break
                self.step_forward()
                for i in before:
                    self._frames_left[i] -= 1
                    if self.stop_status[i] == 0:
                        done[i] += 1
        finally:
            self._frames_left = None
        return done


class _OneValueEnsemble(NavEnsemble):
    """What InfomaxEnsemble and MushroomEnsemble share: one model without per-view memory serves every member, and a step is ONE device
    call on the members' engine (`_batch_call`).  The model keeps no per-view score: a tracking member's scene_familiarity is its least
    familiarity over the headings at every view, filled after each step (as the lone agent's _step_one_value fills it); +inf for a
    member stopped before it sensed.  Members' error metrics run on the device as NavEnsemble's do.  Members with weights of their own
    are not offered: there is no chem_weights argument."""
    _metric = None               # familiarity_model.metric of the agents taken
    _takes = None                # "agents of the ... model (familiarity_model=...(...))", for the refusal
    _batch_call = None           # the engine's batched sense step

    @classmethod
    def _reject_others(cls, agent):
        """The refusals of util.py for the other model without a library."""

    @classmethod
    def _reject_ncc(cls, agent):
        """The NCC model's views lie in the route view store: only NccRouteEnsemble (which overrides this) steps it."""
        reject_ncc(agent, cls.__name__)

    @classmethod
    def _reject_banked(cls, agent):
        reject_banked(agent, cls.__name__)

    @classmethod
    def _check_member(cls, agent):
        func = getattr(agent, "_familiarity_func", None)
        cls._reject_banked(agent)
        cls._reject_ncc(agent)
        cls._reject_others(agent)
        if getattr(getattr(agent, "familiarity_model", None), "metric", None) != cls._metric:
            raise ValueError("%s takes %s; NavEnsemble steps the library-based models" % (cls.__name__, cls._takes))
        if getattr(agent, "_engine", None) is None:
            raise ValueError("%s needs agents whose sensor model runs on the GPU (use_gpu_sensor=True)" % cls.__name__)
        if agent.training_path is None or func is None or getattr(func, "engine", None) is not agent._engine:
            raise ValueError("%s needs trained agents (train_from_path first)" % cls.__name__)

    @classmethod
    def from_agent(cls, agent, poses):
        """`agent`: a trained agent of the ensemble's model with the GPU sensor model; poses: iterable of ((x, y), angle), one member
        each (the first goes to `agent` itself, the others to clones on the same engine and model)."""
        return super(_OneValueEnsemble, cls).from_agent(agent, poses)

    def _device_step(self, idx, xs, ys, angs):
        results = getattr(self.engine, self._batch_call)(xs, ys, angs)
        self._rows = {id(self.agents[i]): results.angle_familiarity[k] for k, i in enumerate(idx)}
        return results

    def _note_scene(self, agent, x, y, headings, weight):
        agent._scene_stale = None
        agent._scene_owner = None
        agent._scene_fam[:] = np.min(self._rows[id(agent)])
        agent._scene_is_inf = False


class InfomaxEnsemble(_OneValueEnsemble):
    """NavEnsemble for agents of the Infomax model (util.infomax_familiarity): the trials of the reference's grid that share one trained
    route and differ in start_offset.  One W serves every member; a step senses every running member's headings, scores them as columns
    of one H = W X and takes each member's first maximum in ONE device call (dv_batch_infomax_sense_step), with the bits a lone agent's
    step_forward gives at the same pose."""
    _metric = "infomax"
    _takes = "agents of the Infomax model (familiarity_model=infomax_familiarity(...))"
    _batch_call = "infomax_sense_step_batch"

    @classmethod
    def _reject_others(cls, agent):
        reject_mushroom(agent, "InfomaxEnsemble")


class MushroomEnsemble(_OneValueEnsemble):
    """NavEnsemble for agents of the mushroom-body model (util.mushroom_familiarity), the twin of InfomaxEnsemble.  One connectivity and
    one byte of weight per Kenyon cell serve every member; a step scores every running member's headings, one workgroup each, straight
    from the landscape, and takes each member's first maximum in ONE device call (dv_batch_mb_sense_step), with the bits a lone agent's
    step_forward gives at the same pose."""
    _metric = "mushroom"
    _takes = "agents of the mushroom-body model (familiarity_model=mushroom_familiarity(...))"
    _batch_call = "mb_sense_step_batch"

    @classmethod
    def _reject_others(cls, agent):
        for obj in (agent, getattr(agent, "familiarity_model", None), getattr(agent, "_familiarity_func", None)):
            if getattr(obj, "metric", None) == "infomax":
                raise ValueError("MushroomEnsemble does not take an Infomax model: navsim_amd.InfomaxEnsemble steps that one")


class _RouteEnsemble(_OneValueEnsemble):
    """What MushroomRouteEnsemble and InfomaxRouteEnsemble share: trials that differ in their TRAINING ROUTE as well as in their start.
    The engine's one model holds a bank per route; from_routes trains all routes in one device call (`_train_banks`), and a step scores
    every running member under its own route's bank in ONE device call (`_batch_call`, which takes the members' banks).  A member steps
    with its ensemble only.

    Members' error metrics (update_error, :252-276): metrics="host", the default, leaves them to every member's own NumPy pass over its
    route.  metrics="device" sets the members' routes on the engine once (path_routes_set), gives every member a slot of coverage marks
    as long as its own route (path_routes_slots, in member order), and takes the metrics of all members that stepped in ONE
    path_routes_error call per ensemble step -- every member with its own coverage_threshold_factor * step_size; the numbers are the
    host's, bit for bit, and "too far from the path" stops a member in the same step, before it marks anything (a member whose
    max_distance_to_training_path is below its coverage reach has its marks taken in a second call: _metrics_call).

    from_landscapes makes trials that differ in their LANDSCAPE as well: the engine holds the landscapes as a set
    (FamiliarityEngine.lands_set), every route is sensed on its own landscape, and a step hands the device the members' landscapes
    beside their banks.  Members on landscapes of one shape keep the vectorised host path of a step; members on landscapes of
    different shapes work out their headings one by one (headings_to_test), each against its own bounds.

    from_landscapes(sensors=[...]) makes trials that differ in their SENSOR too: entry l of the list is the sensor landscape l is sensed
    with -- its sensor_pixel_dimensions, n_sensor_levels and mask_middle_n; w x h stays the engine's one -- kept on the engine as the
    set's sensor table (FamiliarityEngine.sensors_set).  A trial that uses two sensors on one landscape enters that landscape twice.
    The members of a route on landscape l carry that entry's configuration, so their bounds are their own footprint's.

    from_landscapes(noise=dict(...)) puts NOISE IN THE SENSOR: every sensing adds to S and V of every sensor pixel an integer drawn
    uniformly from [-amp, +amp] (FamiliarityEngine.noise_rows has the statement), independent at every sensing and reproducible from
    (seed, key): training view v of route r draws under key (0x80000000 | r) << 32 | v, a member's step under stream << 32 | count,
    count being the device steps the member has taken part in so far (fake or not).  Members carry `noise_stream`, `noise_amp`
    (amp_s, amp_v) and `noise_count`; a member's rows are those of a one-member ensemble built with its stream, whoever else is in
    the ensemble.  The ensemble sets the rows of exactly the members of each device call before it."""
    NOISE_KEYS = ("seed", "amp_s", "amp_v", "train_amp_s", "train_amp_v", "streams")
    _noise_seed = None           # from_landscapes(noise=...): the seed of the members' draws (None: no rows are ever set)
    _metrics_on_slots = False    # (NavEnsemble's slots hold ONE training path: the routed slots are made below)
    _one_route = None            # the name of the ensemble whose members share one trained route
    _info_call = None            # the engine's per-bank info
    METRICS = ("host", "device")

    def __init__(self, agents, metrics="host"):
        name = type(self).__name__
        if metrics not in self.METRICS:
            raise ValueError("metrics must be one of %r, got %r" % (self.METRICS, metrics))
        for a in agents:
            if getattr(a, "memory_bank", None) is None:
                raise ValueError("%s takes the members %s.from_routes makes (agents with a memory_bank); %s steps agents that share one "
                                 "trained route" % (name, name, self._one_route))
        super(_RouteEnsemble, self).__init__(agents)
        self._banks = np.array([a.memory_bank for a in agents], dtype=np.int32)
        on_set = [a.landscape_index is not None for a in agents]
        if any(on_set) and not all(on_set):
            raise ValueError("%s: members on a landscape set (from_landscapes) and members on the engine's one landscape do not mix" % name)
        self._lands = np.array([a.landscape_index for a in agents], dtype=np.int32) if all(on_set) else None
        if self._lands is not None:
            # NavEnsemble asks for ONE landscape object; what the vectorised path needs is one set of bounds: landscapes of one shape
            a0 = agents[0]
            self._uniform = all(a.step_size == a0.step_size and a.landscape.shape == a0.landscape.shape and a._sensor_r == a0._sensor_r and
                                np.array_equal(a.angle_offsets, a0.angle_offsets) for a in agents)
        self.metrics = metrics
        if metrics == "device":
            routes, route_of = [], []                              # the members' routes, each once, in the order the members bring them
            for a in self.agents:
                at = [k for k, r in enumerate(routes) if r is a.training_path]
                if not at:
                    routes.append(a.training_path)
                route_of.append(at[0] if at else len(routes) - 1)
            self.engine.path_routes_set(routes)
            self.engine.path_routes_slots(route_of)
            for j, a in enumerate(self.agents):
                a._metric_slot, a._ens = j, self

    def _metrics_call(self, pend):
        slots = np.array([a._metric_slot for a, _, _ in pend], dtype=np.int32)
        xs = np.array([x for _, x, _ in pend], dtype=np.float64)
        ys = np.array([y for _, _, y in pend], dtype=np.float64)
        reach = np.array([a.coverage_threshold_factor * a.step_size for a, _, _ in pend], dtype=np.float64)
        # The reference stops a member that is too far BEFORE it marks anything (:264-271).  Where max_distance_to_training_path is at
        # least the reach that needs no care: too far is then out of reach of every point.  A member whose limit is below its reach
        # sends a reach that marks nothing, and its marks follow in a second call once its distance is known to be within the limit.
        limit = np.array([a.max_distance_to_training_path for a, _, _ in pend], dtype=np.float64)
        late = limit < reach
        if not late.any():
            return self.engine.path_routes_error(slots, xs, ys, reach)
        nearest = self.engine.path_routes_error(slots, xs, ys, np.where(late, -1.0, reach))
        mark = late & (nearest <= limit)
        if mark.any():
            self.engine.path_routes_error(slots[mark], xs[mark], ys[mark], reach[mark])
        return nearest

    def _read_marks(self, agent):
        return self.engine.path_routes_coverage(agent._metric_slot, len(agent.training_path))

    def _reset_marks(self, agent):
        self.engine.path_routes_reset(agent._metric_slot)

    _summary_call = "marks_summary_routes"

    def _marks_summary(self, members, windows):
        return self.engine.marks_summary_routes([a._metric_slot for a in members], windows)

    @classmethod
    def _reject_banked(cls, agent):
        """(its own members are the banked ones; an SsdRouteEnsemble's or NccRouteEnsemble's carry a route of the view store, not a bank
        of this model)"""
        name = route_ensemble_name(agent)
        if getattr(agent, "memory_bank", None) is not None and name in ("SsdRouteEnsemble", "NccRouteEnsemble") and cls.__name__ != name:
            reject_banked(agent, cls.__name__)

    @classmethod
    def from_agent(cls, agent, poses):
        raise ValueError("%s is made from routes (from_routes); %s.from_agent clones a trained agent" % (cls.__name__, cls._one_route))

    @classmethod
    def _check_model(cls, model):
        """Raises ValueError for an agent's familiarity_model that is not the ensemble's."""
        if getattr(model, "metric", None) != cls._metric:
            raise ValueError("%s takes %s; NavEnsemble steps the library-based models" % (cls.__name__, cls._takes))

    @staticmethod
    def _begin_model(model, eng, agent):
        """A fresh model of the agent's views on the engine, before the routes are trained."""
        model.begin(eng, agent.sensor_dimensions[1], agent.sensor_dimensions[0])

    @staticmethod
    def _train_banks(eng, n_routes, x, y, headings, bank_of_view, land_of_view=None):
        """One bank per route on the engine's fresh model, every view trained into its route's bank in one call -> the views.
        land_of_view: the landscape of the engine's set every view is sensed on (None: the engine's one landscape)."""
        raise NotImplementedError

    @classmethod
    def from_routes(cls, agent, routes, starts):
        """`agent`: an UNTRAINED agent of the ensemble's model with the GPU sensor model; routes: R arrays float64[n_r, 2];
        starts: iterable of (route_index, (x, y), angle), one member each (the first is `agent` itself, the others copies of it on the
        same engine).  Every route is trained into its own bank, all in one call; member i gets the training_path, training_path_length
        and familiar_scenes of routes[route_index_i], and that route's bank as its `memory_bank`.  The members' error metrics run on
        the host; from_routes_with chooses.  Sensor noise needs a landscape set: from_landscapes([landscape], ..., noise=...)."""
        return cls.from_routes_with(agent, routes, starts)

    @classmethod
    def from_routes_with(cls, agent, routes, starts, metrics="host", populations=None):
        """from_routes with the members' error metrics on the host ("host": every member's own NumPy pass, as from_routes) or on the
        device ("device": all members' in one call per ensemble step, each against its own route; see the class).
        populations (MushroomRouteEnsemble): None, or a list with one entry per route, the route's own model parameters -- see
        MushroomRouteEnsemble.  There is no `noise` here: sensor noise rides the landscape table, so use
        from_landscapes([landscape], ..., noise=...)."""
        return cls._from_routes(agent, routes, starts, metrics, None, None, populations=populations)

    @classmethod
    def _population_entries(cls, agent, model, n_routes, populations):
        """`populations` as (the distinct populations, population_of_route), or ValueError naming the entry."""
        raise ValueError("%s has no populations: MushroomRouteEnsemble gives every route's bank cells and wiring of its own" % cls.__name__)

    @classmethod
    def _from_routes(cls, agent, routes, starts, metrics, lands, land_of_route, sensors=None, populations=None, table=None, noise=None,
                     opponent=None):
        """from_routes_with (lands None: every route on the agent's own landscape, the engine's one), or from_landscapes (route r on
        lands[land_of_route[r]] of the engine's landscape set; sensors: None, or _sensor_entries' entry per landscape; noise: None, or
        _noise_arg's dict).  opponent: None, or MushroomRouteEnsemble._opponent_arg's dict: route r gets a second, repulsive bank R + r,
        trained in the same call on the same points sensed at the route's headings plus its turn, behind the attractive views.
        populations: None, or from_routes_with's list (an entry per route).  table: None, or a subclass's own extra argument of
        _train_banks, by name (InfomaxRouteEnsemble's networks)."""
        import copy
        if metrics not in cls.METRICS:
            raise ValueError("metrics must be one of %r, got %r" % (cls.METRICS, metrics))
        cls._reject_ncc(agent)
        cls._reject_others(agent)
        model = getattr(agent, "familiarity_model", None)
        cls._check_model(model)
        eng = getattr(agent, "_engine", None)
        if eng is None:
            raise ValueError("%s needs agents whose sensor model runs on the GPU (use_gpu_sensor=True)" % cls.__name__)
        if agent.training_path is not None or getattr(agent, "memory_bank", None) is not None:
            raise ValueError("%s.from_routes takes an UNTRAINED agent: it trains every route into a bank of its own" % cls.__name__)
        routes = [np.asarray(r, dtype=np.float64) for r in routes]
        if not routes or any(r.ndim != 2 or r.shape[1] != 2 or len(r) < 2 for r in routes):
            raise ValueError("routes must be one or more arrays float64[n_r, 2] of at least two points each")
        starts = [(r, (float(pos[0]), float(pos[1])), float(ang)) for r, pos, ang in starts]
        if not starts:
            raise ValueError("no starts: one (route_index, (x, y), angle) per member")
        for i, (r, _, _) in enumerate(starts):
            if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not 0 <= r < len(routes):
                raise ValueError("starts[%d]: route_index %r outside [0, %d)" % (i, r, len(routes)))
        pops = None if populations is None else cls._population_entries(agent, model, len(routes), populations)
        table = dict(table or {}) if pops is None else dict(populations=pops)    # (_train_banks' extra argument, only where there is a table)
        for k, route in enumerate(routes):                        # (the agent's own bounds test, on the route's own landscape)
            probe = agent if lands is None else cls._on_landscape(copy.copy(agent), lands[land_of_route[k]],
                                                                  None if sensors is None else sensors[land_of_route[k]])
            for pt in route:
                probe._check_bounds(pt)
        # the views of a route look along ITS steps (train_from_path: towards the next point, the last heading once more)
        headings = []
        for route in routes:
            steps = route[1:] - route[:-1]
            h = np.arctan2(steps[:, 1], steps[:, 0])
            headings.append(h[np.minimum(np.arange(len(route)), len(route) - 2)])
        first = np.cumsum([0] + [len(r) for r in routes])
        per_route = [len(r) for r in routes]
        points = np.concatenate(routes)
        all_headings = np.concatenate(headings)
        bank_of_view = np.repeat(np.arange(len(routes), dtype=np.int32), per_route)
        n_banks, sides = len(routes), 1
        if opponent is not None:                                  # the attractive views first, in the order they have without an opponent
            points = np.concatenate([points, points])
            all_headings = np.concatenate([all_headings] + [h + t for h, t in zip(headings, opponent["turn"])])
            bank_of_view = np.concatenate([bank_of_view, bank_of_view + np.int32(len(routes))])
            n_banks, sides = 2 * len(routes), 2
        cls._begin_model(model, eng, agent)
        if lands is None:
            views = cls._train_banks(eng, n_banks, points[:, 0], points[:, 1], all_headings, bank_of_view, **table)
        else:
            eng.lands_set(lands)
            if sensors is not None:
                eng.sensors_set([e["sensor_pixel_dimensions"] for e in sensors], np.stack([e["lut"] for e in sensors]),
                                [e["mask_middle_n"] for e in sensors])
            land_of_view = np.tile(np.repeat(np.array(land_of_route, dtype=np.int32), per_route), sides)
            if noise is not None:                                 # the routes' views draw under their own keys, then no rows until a step
                keys = [cls._train_keys(r, n) for r, n in enumerate(per_route)]
                if opponent is not None:
                    keys += [cls._repulsive_keys(r, n) for r, n in enumerate(per_route)]
                eng.noise_rows(noise["seed"], np.concatenate(keys), np.tile(np.repeat(noise["train_amp_s"], per_route), sides),
                               np.tile(np.repeat(noise["train_amp_v"], per_route), sides))
            try:
                views = cls._train_banks(eng, n_banks, points[:, 0], points[:, 1], all_headings, bank_of_view, land_of_view, **table)
            finally:
                if noise is not None:
                    eng.noise_clear()
        func = model.from_engine(eng, views[:first[-1]])
        members = []
        for k, (r, pos, ang) in enumerate(starts):
            a = agent if k == 0 else copy.copy(agent)
            route = routes[r]
            a.training_path = route
            a.training_path_length = np.sum(np.linalg.norm(route[1:] - route[:-1], axis=1))
            a.familiar_scenes = views[first[r]:first[r + 1]]
            a._familiarity_func = func
            a.memory_bank = int(r)
            a.population_index = None if pops is None else int(pops[1][r])
            a.population = None if pops is None else {k: v for k, v in pops[0][a.population_index].items() if k != "conn"}
            if lands is not None:
                a.landscape_index = land_of_route[r]
                cls._on_landscape(a, lands[a.landscape_index], None if sensors is None else sensors[a.landscape_index])
            a.angle_familiarity = np.full(agent.n_test_angles, np.nan)
            a.scene_familiarity = np.zeros(len(route), dtype=np.float64)
            a._scene_is_inf = False
            a._metrics_on_device = False                         # (update_error's NumPy branch, until the ensemble gives it a slot)
            a._metric_slot, a._ens, a._spec = None, None, None
            a.step_familiarity = np.inf
            a.position, a.angle = pos, ang
            a.reset_error()
            a.noise_stream = None if noise is None else noise["streams"][k]
            a.noise_amp = None if noise is None else (noise["amp_s"][k], noise["amp_v"][k])
            a.noise_count, a._noise_key = 0, None
            if opponent is not None:
                a.repulsive_bank = len(routes) + int(r)
                a.opponent_gain = opponent["gain"][k]
                a.repulsive_scenes = views[first[-1] + first[r]:first[-1] + first[r + 1]]
                a.bank_novelty = None
            members.append(a)
        ens = cls(members, metrics=metrics)
        if noise is not None:
            ens._noise_seed = noise["seed"]
        return ens

    # ---- sensor noise (from_landscapes(noise=...)) --------------------------------------------------------------------------------
    @staticmethod
    def _train_keys(route, n_views):
        """uint64[n_views]: the noise keys of the views of route `route`, (0x80000000 | route) << 32 | view."""
        return (np.uint64((0x80000000 | route) << 32) | np.arange(n_views, dtype=np.uint64)).astype(np.uint64)

    @staticmethod
    def _repulsive_keys(route, n_views):
        """... and of the views of its repulsive bank (MushroomRouteEnsemble's opponent): (0xC0000000 | route) << 32 | view."""
        return (np.uint64((0xC0000000 | route) << 32) | np.arange(n_views, dtype=np.uint64)).astype(np.uint64)

    @staticmethod
    def _step_key(stream, count):
        """The noise key of a member's device step: stream << 32 | count (count wraps at 2**32)."""
        return (int(stream) << 32) | (int(count) & 0xFFFFFFFF)

    @classmethod
    def _noise_arg(cls, noise, n_starts, n_routes):
        """from_landscapes' `noise` as dict(seed, amp_s / amp_v: a list per start, train_amp_s / train_amp_v: a list per route,
        streams: a list per start), or None.  ValueError names the entry."""
        if noise is None:
            return None
        if not isinstance(noise, dict):
            raise ValueError("noise must be None or a dict with any of %r, got %r" % (cls.NOISE_KEYS, noise))
        extra = sorted(set(noise) - set(cls.NOISE_KEYS))
        if extra:
            raise ValueError("noise: unknown keys %r (it holds any of %r)" % (extra, cls.NOISE_KEYS))

        def whole(v):
            return isinstance(v, (int, np.integer)) and not isinstance(v, bool)
        seed = noise.get("seed", 0)
        if not whole(seed) or not 0 <= seed < 2 ** 64:
            raise ValueError("noise['seed'] must be an integer in [0, 2**64), got %r" % (seed,))

        def amps(key, n, per):
            v = noise.get(key, 0)
            if isinstance(v, (list, tuple, np.ndarray)):
                if len(v) != n:
                    raise ValueError("noise[%r] holds %d values for %d %s" % (key, len(v), n, per))
                items = [("noise[%r][%d]" % (key, i), x) for i, x in enumerate(v)]
            else:
                items = [("noise[%r]" % key, v)] * n
            for what, x in items:
                if not whole(x) or not 0 <= x <= 255:
                    raise ValueError("%s = %r: an amplitude is an integer in [0, 255]" % (what, x))
            return [int(x) for _, x in items]
        out = dict(seed=int(seed), amp_s=amps("amp_s", n_starts, "starts"), amp_v=amps("amp_v", n_starts, "starts"),
                   train_amp_s=amps("train_amp_s", n_routes, "routes"), train_amp_v=amps("train_amp_v", n_routes, "routes"))
        streams = noise.get("streams")
        if streams is None:
            streams = list(range(n_starts))
        else:
            if isinstance(streams, (str, dict)) or not hasattr(streams, "__len__") or len(streams) != n_starts:
                raise ValueError("noise['streams'] must be None or a list with one stream per start (%d), got %r" % (n_starts, streams))
            streams = list(streams)
            for i, x in enumerate(streams):
                if not whole(x) or not 0 <= x < 2 ** 31:
                    raise ValueError("noise['streams'][%d] = %r: a stream is an integer in [0, 2**31)" % (i, x))
                if x in streams[:i]:
                    raise ValueError("noise['streams'][%d] = %d duplicates noise['streams'][%d]: members of one stream would draw the same "
                                     "noise" % (i, x, streams.index(x)))
        out["streams"] = [int(x) for x in streams]
        return out

    def _noise_begin_step(self, idx):
        """The members `idx` are about to take part in a device step: each gets that step's key (kept for its scene_familiarity) and
        its count goes up.  Nothing without noise."""
        if self._noise_seed is None:
            return
        for i in idx:
            a = self.agents[i]
            a._noise_key = self._step_key(a.noise_stream, a.noise_count)
            a.noise_count += 1

    def _noise_set_rows(self, agents):
        """The engine's noise rows become those of `agents`, the members of the device call that follows, under their last keys."""
        if self._noise_seed is None:
            return
        self.engine.noise_rows(self._noise_seed, np.array([a._noise_key for a in agents], dtype=np.uint64),
                               [a.noise_amp[0] for a in agents], [a.noise_amp[1] for a in agents])

    @staticmethod
    def _on_landscape(agent, landscape, sensor=None):
        """`agent` on `landscape`: its bounds are worked out again from that landscape's shape -> the agent.  sensor: that landscape's
        entry of the sensor table (_sensor_entries), which the agent then carries: its bounds are its own footprint's."""
        agent.landscape = landscape
        if sensor is not None:
            agent.sensor_index = sensor["index"]
            agent.sensor_pixel_dimensions = sensor["sensor_pixel_dimensions"].copy()
            agent.n_sensor_levels = sensor["n_sensor_levels"]
            agent.mask_middle_n = sensor["mask_middle_n"]
            extent = agent.sensor_dimensions * agent.sensor_pixel_dimensions
            agent._sensor_r = np.max(extent / 2)
            agent._landscape_glimpse_buf = np.empty((extent[1], extent[0], 3), dtype=np.uint8)
        agent._bounds = agent._bounds_arr = None
        return agent

    SENSOR_KEYS = ("sensor_pixel_dimensions", "n_sensor_levels", "mask_middle_n")

    @classmethod
    def _sensor_entries(cls, agent, n_lands, sensors):
        """from_landscapes' `sensors` as a list of dict(index, sensor_pixel_dimensions int[2], n_sensor_levels (3-tuple), mask_middle_n,
        lut uint8[3, 256]), an entry per landscape; a key an entry leaves out takes the agent's value.  ValueError names the entry."""
        import copy
        sensors = list(sensors)
        if len(sensors) != n_lands:
            raise ValueError("sensors holds %d entries for %d landscapes: one per landscape (None: the agent's own configuration)"
                             % (len(sensors), n_lands))
        w = int(agent.sensor_dimensions[0])
        out = []
        for l, s in enumerate(sensors):
            if s is not None and not isinstance(s, dict):
                raise ValueError("sensors[%d] must be None or a dict with any of %r" % (l, cls.SENSOR_KEYS))
            s = dict(s or {})
            if "sensor_dimensions" in s:
                raise ValueError("sensors[%d]: sensor_dimensions cannot differ between entries: w × h is the engine's one" % l)
            extra = sorted(set(s) - set(cls.SENSOR_KEYS))
            if extra:
                raise ValueError("sensors[%d]: unknown keys %r (an entry holds any of %r)" % (l, extra, cls.SENSOR_KEYS))
            px = np.asarray(s.get("sensor_pixel_dimensions", agent.sensor_pixel_dimensions))
            if px.dtype.kind not in "iu" or px.shape != (2,) or px.min() < 1 or int(px[0]) * int(px[1]) > 4096:
                raise ValueError("sensors[%d]: sensor_pixel_dimensions must be two integers (pw, ph) >= 1 with pw * ph <= 4096, got %r"
                                 % (l, s.get("sensor_pixel_dimensions")))
            if np.any((agent.sensor_dimensions * px) % 2 != 0):
                raise ValueError("sensors[%d]: the sensor's extent %r in landscape pixels must be even" % (l, (agent.sensor_dimensions * px).tolist()))
            levels = s.get("n_sensor_levels", agent.n_sensor_levels)
            if not isinstance(levels, tuple):
                levels = (256, 256, levels)
            if len(levels) != 3 or not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) and 2 <= v <= 256 for v in levels):
                raise ValueError("sensors[%d]: n_sensor_levels must be in [2, 256] (one value, or a tuple of three), got %r" % (l, levels))
            mask = s.get("mask_middle_n", agent.mask_middle_n)
            if isinstance(mask, bool) or not isinstance(mask, (int, np.integer)) or not 0 <= mask <= w // 2:
                raise ValueError("sensors[%d]: mask_middle_n %r outside [0, w / 2 = %d]" % (l, mask, w // 2))
            probe = copy.copy(agent)                              # the agent's own level arithmetic, on the entry's levels
            probe.n_sensor_levels = tuple(int(v) for v in levels)
            out.append(dict(index=l, sensor_pixel_dimensions=px.astype(np.asarray(agent.sensor_pixel_dimensions).dtype),
                            n_sensor_levels=probe.n_sensor_levels, mask_middle_n=int(mask), lut=probe._level_tables()))
        return out

    @classmethod
    def from_landscapes(cls, agent, landscapes, routes, starts, metrics="host", sensors=None, noise=None, populations=None):
        """Trials that differ in their LANDSCAPE, their training route and their start.  `agent`: an UNTRAINED agent of the ensemble's
        model with the GPU sensor model; landscapes: a list of uint8[rows, cols, 3] of any shapes; routes: a list of
        (landscape_index, float64[n_r, 2]); starts and metrics as from_routes_with.  The landscapes become the engine's landscape set,
        every route is bounds-checked against and sensed on ITS landscape and trained into its own bank, all routes in one call.
        Member i gets what from_routes gives it, and the landscape of its route: `landscape` (so its bounds, and the host sensor
        model, are that landscape's) and `landscape_index`.
        sensors: None (every landscape under the agent's own sensor, the engine's one), or a list as long as `landscapes`: entry l is
        None (the agent's own configuration) or a dict with any of sensor_pixel_dimensions, n_sensor_levels and mask_middle_n, the
        sensor landscape l is sensed with; sensor_dimensions is refused (w × h is the engine's one).  Two sensors on one landscape:
        enter the landscape twice.  The members of a route on landscape l carry that entry's configuration and `sensor_index`, so
        their bounds are their own footprint's and their get_sensor_mat senses under their own entry.
        populations: as from_routes_with's, an entry per route.
        noise: None (the sensor is the deterministic model, and no noise row is ever set), or a dict with any of
            seed=0, amp_s=0, amp_v=0       recall: an integer amplitude in [0, 255], or a list with one per start
            train_amp_s=0, train_amp_v=0   the training views: likewise, or a list per route (0: a noiseless memory)
            streams=None                   None: a start's index; or a list of distinct ints in [0, 2**31), one per start
        (see the class).  A scene_familiarity read after a step re-senses that step's poses under that step's keys."""
        starts, routes = list(starts), list(routes)
        nz = cls._noise_arg(noise, len(starts), len(routes))
        if nz is not None and populations is not None:
            raise ValueError("noise with populations: the sensed step under a population table has no noise form")
        lands, points, land_of_route, entries = cls._landscape_args(agent, landscapes, routes, sensors)
        return cls._from_routes(agent, points, starts, metrics, lands, land_of_route, entries, populations=populations, noise=nz)

    @classmethod
    def _landscape_args(cls, agent, landscapes, routes, sensors):
        """from_landscapes' landscapes, routes and sensors, checked -> (the landscapes, every route's points, land_of_route, the
        sensor entries or None): what _from_routes takes."""
        lands = [np.asarray(l) for l in landscapes]
        if not lands or any(l.dtype != np.uint8 or l.ndim != 3 or l.shape[2] != 3 for l in lands):
            raise ValueError("landscapes must be one or more arrays uint8[rows, cols, 3]")
        routes = list(routes)
        for k, rt in enumerate(routes):
            if not isinstance(rt, (tuple, list)) or len(rt) != 2:
                raise ValueError("routes[%d] must be (landscape_index, float64[n_r, 2])" % k)
            l = rt[0]
            if isinstance(l, bool) or not isinstance(l, (int, np.integer)) or not 0 <= l < len(lands):
                raise ValueError("routes[%d]: landscape_index %r outside [0, %d)" % (k, l, len(lands)))
        land_of_route = [int(l) for l, _ in routes]
        entries = None if sensors is None else cls._sensor_entries(agent, len(lands), sensors)
        return lands, [pts for _, pts in routes], land_of_route, entries

    def _device_step(self, idx, xs, ys, angs):
        if self._lands is not None:
            self._noise_begin_step(idx)
            self._noise_set_rows([self.agents[i] for i in idx])
            results = getattr(self.engine, self._batch_call)(xs, ys, angs, self._banks[idx], land_of_member=self._lands[idx])
        else:
            results = getattr(self.engine, self._batch_call)(xs, ys, angs, self._banks[idx])
        self._rows = {id(self.agents[i]): results.angle_familiarity[k] for k, i in enumerate(idx)}
        return results

    def bank_info(self):
        """Per bank (route): the engine's dict of n_banks and arrays of R entries (views_trained, and the model's own figure)."""
        return getattr(self.engine, self._info_call)()


class MushroomRouteEnsemble(_RouteEnsemble):
    """MushroomEnsemble for trials that differ in their TRAINING ROUTE as well (the reference's grid varies training_path_curve on one
    landscape, scripts/run_experiment.py:57,208): the model's connectivity is shared, and every route has a memory bank of its own
    (FamiliarityEngine.mbank_set: n_kc bytes a route).  All routes are trained in one device call, and a step scores every running
    member's headings under its own route's bank in ONE device call (dv_mbank_sense_step), with the bits a lone agent trained on that
    route alone gives at the same pose.  Made by from_routes (see _RouteEnsemble).

    from_routes_with / from_landscapes(populations=[...]) makes trials that differ in the MODEL's own parameters too (capacity sweeps,
    replicates over the random wiring): the list has one entry per route, None (the agent's model) or a dict with any of n_kc, fan_in,
    sparsity, seed and channel -- a key an entry leaves out takes the model's value.  Equal entries share one population of the
    engine's population table (FamiliarityEngine.mbpop_set), and every route's bank has the cells, wiring, quota and channel of its
    entry; a route under two populations is entered twice, as a landscape under two sensors is.  Members carry `population_index` and
    `population` (dict(channel, n_kc, fan_in, n_active, sparsity, seed)); both are None without populations.  A member's rows are those
    of a lone agent built with mushroom_familiarity of its population and trained on its route alone.

    from_routes_with / from_landscapes(opponent=dict(turn=np.pi, gain=1)) gives every route an OPPONENT memory (Le Moel & Wystrach
    2020): route r keeps bank r, the attractive one, and gets bank R + r, the repulsive one, trained on the same points sensed at the
    route's headings plus `turn`; all 2 sum n_r views go up in the one training call, the attractive ones first.  A member's step reads
    ONE selection of firing cells out through both banks (FamiliarityEngine.mbset_sense_step_batch: banks [r, R + r], coefficients
    [1, -gain]), so angle_familiarity[a] = -(d_att - gain d_rep), and it steers by the first maximum of that difference.  Members
    carry `memory_bank` (r), `repulsive_bank` (R + r), `opponent_gain`, `repulsive_scenes` and, after a step, `bank_novelty`
    (int32[A, 2]: d_att and d_rep of every heading); bank_info() has 2 R entries.  Like every banked member, an opponent member
    steps with its ensemble only: its own step_forward is refused (a step of its own would read the attractive bank alone).  Not
    with `populations`: banks of different populations share no selection."""
    POPULATION_KEYS = ("n_kc", "fan_in", "sparsity", "seed", "channel")
    _metric = "mushroom"
    _takes = MushroomEnsemble._takes
    _batch_call = "mbank_sense_step_batch"
    _info_call = "mbank_info"                # dict(n_banks, views_trained int64[R], n_depressed int64[R])
    _one_route = "MushroomEnsemble"
    _reject_others = MushroomEnsemble._reject_others
    OPPONENT_KEYS = ("turn", "gain")
    MAX_GAIN = 1024

    def __init__(self, agents, metrics="host"):
        super(MushroomRouteEnsemble, self).__init__(agents, metrics=metrics)
        rep = [getattr(a, "repulsive_bank", None) for a in agents]
        if any(r is not None for r in rep) and any(r is None for r in rep):
            raise ValueError("MushroomRouteEnsemble: members with an opponent memory (a repulsive_bank) and members without one do not mix")
        # an opponent member's set of a step: banks (attractive, repulsive) under coefficients (1, -gain)
        self._sets = None if rep[0] is None else np.array([[a.memory_bank, a.repulsive_bank] for a in agents], dtype=np.int32)
        self._coefs = None if rep[0] is None else np.array([[1, -a.opponent_gain] for a in agents], dtype=np.int32)

    @classmethod
    def _opponent_arg(cls, opponent, n_starts, n_routes):
        """from_routes_with's / from_landscapes' `opponent` as dict(turn: a float per route, gain: an int per start), or None.
        ValueError names the entry."""
        if opponent is None:
            return None
        if not isinstance(opponent, dict):
            raise ValueError("opponent must be None or a dict with any of %r, got %r" % (cls.OPPONENT_KEYS, opponent))
        extra = sorted(set(opponent) - set(cls.OPPONENT_KEYS))
        if extra:
            raise ValueError("opponent: unknown keys %r (it holds any of %r)" % (extra, cls.OPPONENT_KEYS))

        def per(key, default, n, of, ok, rule):
            v = opponent.get(key, default)
            if isinstance(v, (list, tuple, np.ndarray)):
                if len(v) != n:
                    raise ValueError("opponent[%r] holds %d values for %d %s" % (key, len(v), n, of))
                items = [("opponent[%r][%d]" % (key, i), x) for i, x in enumerate(v)]
            else:
                items = [("opponent[%r]" % key, v)] * n
            for what, x in items:
                if isinstance(x, bool) or not ok(x):
                    raise ValueError("%s = %r: %s" % (what, x, rule))
            return [x for _, x in items]
        turn = per("turn", np.pi, n_routes, "routes", lambda x: isinstance(x, (int, float, np.integer, np.floating)) and np.isfinite(x),
                   "a turn is a finite angle in radians")
        gain = per("gain", 1, n_starts, "starts", lambda x: isinstance(x, (int, np.integer)) and 0 <= x <= cls.MAX_GAIN,
                   "a gain is an integer in [0, %d]" % cls.MAX_GAIN)
        return dict(turn=[float(t) for t in turn], gain=[int(g) for g in gain])

    @classmethod
    def from_routes_with(cls, agent, routes, starts, metrics="host", opponent=None, populations=None):
        """_RouteEnsemble.from_routes_with, and opponent: None (exactly the calls made without it), or a dict with any of
            turn=np.pi     the repulsive views look along the route's headings plus this angle: a float, or a list per route
            gain=1         an integer in [0, 1024], or a list per start
        (see the class).  There is no `noise` here: sensor noise rides the landscape table, so use
        from_landscapes([landscape], ..., noise=...)."""
        starts, routes = list(starts), list(routes)
        opp = cls._opponent_arg(opponent, len(starts), len(routes))
        if opp is not None and populations is not None:
            raise ValueError("opponent with populations: banks of different populations share no selection of firing cells")
        return cls._from_routes(agent, routes, starts, metrics, None, None, populations=populations, opponent=opp)

    @classmethod
    def from_landscapes(cls, agent, landscapes, routes, starts, metrics="host", sensors=None, noise=None, opponent=None, populations=None):
        """_RouteEnsemble.from_landscapes, and opponent as from_routes_with's.  Under `noise` the attractive training keys are the
        ones without an opponent, and repulsive view v of route r draws under (0xC0000000 | r) << 32 | v with the route's training
        amplitudes."""
        starts, routes = list(starts), list(routes)
        opp = cls._opponent_arg(opponent, len(starts), len(routes))
        if opp is not None and populations is not None:
            raise ValueError("opponent with populations: banks of different populations share no selection of firing cells")
        nz = cls._noise_arg(noise, len(starts), len(routes))
        if nz is not None and populations is not None:
            raise ValueError("noise with populations: the sensed step under a population table has no noise form")
        lands, points, land_of_route, entries = cls._landscape_args(agent, landscapes, routes, sensors)
        return cls._from_routes(agent, points, starts, metrics, lands, land_of_route, entries, populations=populations, noise=nz, opponent=opp)

    def _device_step(self, idx, xs, ys, angs):
        if self._sets is None:
            return super(MushroomRouteEnsemble, self)._device_step(idx, xs, ys, angs)
        lands = None
        if self._lands is not None:
            self._noise_begin_step(idx)
            self._noise_set_rows([self.agents[i] for i in idx])
            lands = self._lands[idx]
        results = self.engine.mbset_sense_step_batch(xs, ys, angs, self._sets[idx], self._coefs[idx], land_of_member=lands)
        self._rows = {id(self.agents[i]): results.angle_familiarity[k] for k, i in enumerate(idx)}
        for k, i in enumerate(idx):
            self.agents[i].bank_novelty = results.bank_novelty[k]
        return results

    @staticmethod
    def _train_banks(eng, n_routes, x, y, headings, bank_of_view, land_of_view=None, populations=None):
        if populations is None:
            eng.mbank_set(n_routes)
        else:
            eng.mbpop_set(*populations)                           # bank r is route r's, behind its entry's population
        if land_of_view is None:
            return eng.mbank_train_from_poses(x, y, headings, bank_of_view)
        return eng.mbank_train_from_poses(x, y, headings, bank_of_view, land_of_view=land_of_view)

    @classmethod
    def _population_entries(cls, agent, model, n_routes, populations):
        from .util import mushroom_population
        if isinstance(populations, dict) or not hasattr(populations, "__len__") or len(populations) != n_routes:
            raise ValueError("populations must be a list with one entry per route (%d), each None or a dict with any of %r"
                             % (n_routes, cls.POPULATION_KEYS))
        own = {k: getattr(model, k) for k in cls.POPULATION_KEYS}
        n_pixels = int(agent.sensor_dimensions[0]) * int(agent.sensor_dimensions[1])
        keys, pops, of_route = [], [], []
        for r, entry in enumerate(populations):
            if entry is not None and not isinstance(entry, dict):
                raise ValueError("populations[%d] must be None or a dict with any of %r" % (r, cls.POPULATION_KEYS))
            extra = sorted(set(entry or {}) - set(cls.POPULATION_KEYS))
            if extra:
                raise ValueError("populations[%d]: unknown keys %r (an entry holds any of %r)" % (r, extra, cls.POPULATION_KEYS))
            spec = dict(own, **(entry or {}))
            try:
                key = tuple(spec[k] for k in cls.POPULATION_KEYS)
                if key not in keys:
                    pop = mushroom_population(n_pixels, **spec)
                    keys.append(key)
                    pops.append(dict(pop, sparsity=spec["sparsity"], seed=spec["seed"]))
            except (ValueError, TypeError) as e:
                raise ValueError("populations[%d]: %s" % (r, e))
            of_route.append(keys.index(key))
        return pops, np.array(of_route, dtype=np.int32)

    def bank_info(self):
        """_RouteEnsemble.bank_info, and per bank n_kc, n_active and population_of_bank (zeros without populations), so that a bank's
        fill is n_depressed / n_kc."""
        info = dict(super(MushroomRouteEnsemble, self).bank_info())
        pops, n = getattr(self.engine, "mb_pops", None), int(info["n_banks"])
        if pops is None:
            model = self.agents[0].familiarity_model
            of_bank = np.zeros(n, dtype=np.int32)
            pops = [dict(n_kc=model.n_kc, n_active=model.n_active)]
        else:
            of_bank = np.asarray(self.engine.mb_pop_of_bank, dtype=np.int32)
        info.update(n_kc=np.array([pops[p]["n_kc"] for p in of_bank], dtype=np.int64),
                    n_active=np.array([pops[p]["n_active"] for p in of_bank], dtype=np.int64), population_of_bank=of_bank)
        return info


class InfomaxRouteEnsemble(_RouteEnsemble):
    """InfomaxEnsemble for trials that differ in their TRAINING ROUTE as well, the twin of MushroomRouteEnsemble: every route has a weight
    bank of its own on the one engine (FamiliarityEngine.ibank_set: n_hidden x h*w doubles a route), every bank begins as the model's own
    seeded W0, all routes are trained in one device call whose chains advance in lockstep (dv_ibank_train_from_poses), and a step scores
    every running member's headings under its own route's W in ONE device call (dv_ibank_sense_step), with the bits a lone agent trained
    on that route alone gives at the same pose.  Made by from_routes (see _RouteEnsemble).

    from_routes_with / from_landscapes(networks=[...]) makes trials that differ in the MODEL's own parameters too (learning-rate and
    capacity sweeps, replicates over the initial weights): the list has one entry per route, None (the agent's model) or a dict with any
    of n_hidden, learning_rate, seed and channel -- a key an entry leaves out takes the model's value.  Equal entries share one network
    of the engine's network table (FamiliarityEngine.inet_set), and every route's bank has the shape, rate, W0 and channel of its entry;
    a route under two networks is entered twice.  Members carry `network_index` and `network` (dict(channel, n_hidden, learning_rate,
    seed)); both are None without networks.  A member's rows are those of a lone agent built with infomax_familiarity of its network
    and trained on its route alone."""
    NETWORK_KEYS = ("n_hidden", "learning_rate", "seed", "channel")
    _metric = "infomax"
    _takes = InfomaxEnsemble._takes
    _batch_call = "ibank_sense_step_batch"
    _info_call = "ibank_info"                # dict(n_banks, views_trained int64[R], finite bool[R])
    _one_route = "InfomaxEnsemble"
    _reject_others = InfomaxEnsemble._reject_others

    @staticmethod
    def _train_banks(eng, n_routes, x, y, headings, bank_of_view, land_of_view=None, networks=None):
        if networks is None:
            eng.ibank_set(n_routes, eng.infomax_read_weights())      # (bank 0 holds the W0 the model's begin has just drawn)
        else:
            eng.inet_set(*networks)                                   # bank r is route r's, behind its entry's network
        if land_of_view is None:
            return eng.ibank_train_from_poses(x, y, headings, bank_of_view)
        return eng.ibank_train_from_poses(x, y, headings, bank_of_view, land_of_view=land_of_view)

    @classmethod
    def _population_entries(cls, agent, model, n_routes, populations):
        raise ValueError("%s has no populations: MushroomRouteEnsemble gives every route's bank cells and wiring of its own (an Infomax "
                         "route's own n_hidden, learning rate, seed and channel go in networks=)" % cls.__name__)

    @classmethod
    def _network_entries(cls, agent, model, n_routes, networks):
        """`networks` as (the distinct networks, network_of_route), or ValueError naming the entry."""
        from .util import infomax_network
        if isinstance(networks, dict) or not hasattr(networks, "__len__") or len(networks) != n_routes:
            raise ValueError("networks must be a list with one entry per route (%d), each None or a dict with any of %r"
                             % (n_routes, cls.NETWORK_KEYS))
        own = {k: getattr(model, k) for k in cls.NETWORK_KEYS}
        n_pixels = int(agent.sensor_dimensions[0]) * int(agent.sensor_dimensions[1])
        keys, nets, of_route = [], [], []
        for r, entry in enumerate(networks):
            if entry is not None and not isinstance(entry, dict):
                raise ValueError("networks[%d] must be None or a dict with any of %r" % (r, cls.NETWORK_KEYS))
            extra = sorted(set(entry or {}) - set(cls.NETWORK_KEYS))
            if extra:
                raise ValueError("networks[%d]: unknown keys %r (an entry holds any of %r)" % (r, extra, cls.NETWORK_KEYS))
            spec = dict(own, **(entry or {}))
            try:
                net = None
                if spec["n_hidden"] is not None:
                    key = tuple(spec[k] for k in cls.NETWORK_KEYS)
                else:                                             # (None: as many rows as the view has pixels -- equal to that number given)
                    net = infomax_network(n_pixels, **spec)
                    key = (net["n_hidden"],) + tuple(spec[k] for k in cls.NETWORK_KEYS[1:])
                if key not in keys:
                    net = net or infomax_network(n_pixels, **spec)
                    keys.append(key)
                    nets.append(dict(net, seed=spec["seed"]))
            except (ValueError, TypeError) as e:
                raise ValueError("networks[%d]: %s" % (r, e))
            of_route.append(keys.index(key))
        return nets, np.array(of_route, dtype=np.int32)

    @classmethod
    def from_routes_with(cls, agent, routes, starts, metrics="host", networks=None):
        """_RouteEnsemble.from_routes_with; networks: None, or a list with one entry per route, the route's own model parameters
        (see the class)."""
        return cls._from_routes(agent, list(routes), starts, metrics, None, None, networks=networks)

    @classmethod
    def from_landscapes(cls, agent, landscapes, routes, starts, metrics="host", sensors=None, noise=None, networks=None):
        """_RouteEnsemble.from_landscapes; networks: as from_routes_with's, an entry per route."""
        starts, routes = list(starts), list(routes)
        nz = cls._noise_arg(noise, len(starts), len(routes))
        lands, points, land_of_route, entries = cls._landscape_args(agent, landscapes, routes, sensors)
        return cls._from_routes(agent, points, starts, metrics, lands, land_of_route, entries, networks=networks, noise=nz)

    @classmethod
    def _from_routes(cls, agent, routes, starts, metrics, lands, land_of_route, sensors=None, networks=None, noise=None):
        nets = None
        if networks is not None:
            model = getattr(agent, "familiarity_model", None)
            cls._check_model(model)
            nets = cls._network_entries(agent, model, len(routes), networks)
        ens = super(InfomaxRouteEnsemble, cls)._from_routes(agent, routes, starts, metrics, lands, land_of_route, sensors,
                                                            table=None if nets is None else dict(networks=nets), noise=noise)
        for a in ens.agents:
            a.network_index = None if nets is None else int(nets[1][a.memory_bank])
            a.network = None if nets is None else {k: v for k, v in nets[0][a.network_index].items() if k != "w0"}
        return ens

    def bank_info(self):
        """_RouteEnsemble.bank_info, and per bank n_hidden, learning_rate and network_of_bank (zeros without networks)."""
        info = dict(super(InfomaxRouteEnsemble, self).bank_info())
        nets, n = getattr(self.engine, "infomax_nets", None), int(info["n_banks"])
        if nets is None:
            of_bank = np.zeros(n, dtype=np.int32)
            nets = [dict(n_hidden=self.engine.infomax_hidden, learning_rate=self.agents[0].familiarity_model.learning_rate)]
        else:
            of_bank = np.asarray(self.engine.infomax_net_of_bank, dtype=np.int32)
        info.update(n_hidden=np.array([nets[p]["n_hidden"] for p in of_bank], dtype=np.int64),
                    learning_rate=np.array([nets[p]["learning_rate"] for p in of_bank], dtype=np.float64), network_of_bank=of_bank)
        return info


class _WindowedMembers(object):
    """What SadsRouteEnsemble and SsdRouteEnsemble share of perfect memory WITH A TEMPORAL WINDOW: the arguments window,
    window_centres and relocalise_below of from_routes_with / from_landscapes, the members' attributes (window, memory_index,
    relocalise_below, relocalised, n_relocalisations), relocalise() and the window of a member's coming step."""
    WINDOW_MAX_VIEWS = 512                       # views of a member's window at most (FamiliarityEngine.RVWIN_MAX_VIEWS)

    @classmethod
    def _windows_arg(cls, window, window_centres, starts, route_lengths):
        """`window` and `window_centres` of from_routes_with / from_landscapes as two lists with an entry per start: (behind, ahead) or
        None (the member keeps its whole route), and the initial memory_index or None.  ValueError names the entry."""
        n = len(starts)
        if window is None:
            if window_centres is not None:
                raise ValueError("window_centres without window: a centre is the middle of a member's window")
            return [None] * n, [None] * n

        def pair(w, what):
            if isinstance(w, (int, np.integer)) and not isinstance(w, bool):
                w = (w, w)
            ok = isinstance(w, (tuple, list)) and len(w) == 2 and all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) and v >= 0
                                                                      for v in w)
            if not ok:
                raise ValueError("%s must be an int W >= 0 (W views behind and ahead) or a pair (behind, ahead) of such, got %r" % (what, w))
            if w[0] + w[1] + 1 > cls.WINDOW_MAX_VIEWS:
                raise ValueError("%s = %r: a window holds behind + ahead + 1 <= %d views" % (what, tuple(w), cls.WINDOW_MAX_VIEWS))
            return (int(w[0]), int(w[1]))
        if isinstance(window, list):                                # (a list: an entry per start; a pair is a tuple)
            if len(window) != n:
                raise ValueError("window holds %d entries for %d starts" % (len(window), n))
            wins = [None if w is None else pair(w, "window[%d]" % i) for i, w in enumerate(window)]
        else:
            wins = [pair(window, "window")] * n
        centres = [None] * n
        if window_centres is not None:
            centres = list(window_centres)
            if len(centres) != n:
                raise ValueError("window_centres holds %d entries for %d starts" % (len(centres), n))
            for i, m in enumerate(centres):
                if m is None:
                    continue
                if isinstance(m, bool) or not isinstance(m, (int, np.integer)):
                    raise ValueError("window_centres[%d] must be None or a view index within the member's route, got %r" % (i, m))
                if wins[i] is None:
                    raise ValueError("window_centres[%d] = %d, but member %d has no window" % (i, m, i))
                r = starts[i][0]
                if isinstance(r, (int, np.integer)) and 0 <= r < len(route_lengths) and not 0 <= m < route_lengths[r]:
                    raise ValueError("window_centres[%d] = %d outside [0, %d), the views of route %d" % (i, m, route_lengths[r], r))
                centres[i] = int(m)
        return wins, centres

    def _set_windows(self, wins, centres, thresholds=None):
        for i, (a, w, m) in enumerate(zip(self.agents, wins, centres)):
            a.window, a.memory_index = w, m
            a.relocalise_below = None if thresholds is None else thresholds[i]
            a.relocalised, a.n_relocalisations = False, 0

    @staticmethod
    def _thresholds_arg(relocalise_below, wins):
        """`relocalise_below` of from_routes_with / from_landscapes as a list with a float or None per start (wins: _windows_arg's):
        a threshold belongs to a member with a window.  ValueError names the entry."""
        n = len(wins)
        if relocalise_below is None:
            return [None] * n

        def one(t, what):
            if isinstance(t, bool) or not isinstance(t, (int, float, np.integer, np.floating)):
                raise ValueError("%s must be a familiarity (a float) or None, got %r" % (what, t))
            if np.isnan(t):
                raise ValueError("%s is NaN" % what)
            return float(t)
        if isinstance(relocalise_below, (list, tuple)):
            if len(relocalise_below) != n:
                raise ValueError("relocalise_below holds %d entries for %d starts" % (len(relocalise_below), n))
            out = [None if t is None else one(t, "relocalise_below[%d]" % i) for i, t in enumerate(relocalise_below)]
        else:
            out = [one(relocalise_below, "relocalise_below")] * n
        for i, (t, w) in enumerate(zip(out, wins)):
            if t is not None and w is None:
                raise ValueError("relocalise_below[%d] = %r, but member %d has no window: the threshold is a windowed member's loss test"
                                 % (i, t, i))
        return out

    def relocalise(self, members=None):
        """The members `members` (indices; None: all) forget which view they matched last: memory_index = None, so that their next step
        scores the whole route (global localisation) and centres their window anew."""
        for i in (range(len(self.agents)) if members is None else members):
            self.agents[i].memory_index = None

    def _window_of(self, agent):
        """[lo, hi) of the coming step of a member with a window and a centre: clipped at both ends of its route; else None."""
        w, m = getattr(agent, "window", None), getattr(agent, "memory_index", None)
        if w is None or m is None:
            return None
        return max(0, m - w[0]), min(len(agent.training_path), m + w[1] + 1)

    def _remember_views(self, idx, results):
        """After a device step: a member that is about to apply it (every one with a window that is not flagged) remembers the view its
        chosen heading matched, and whether the step re-localised it."""
        for k, i in enumerate(idx):
            a = self.agents[i]
            if getattr(a, "window", None) is not None and not results.flags[k] & 16:
                a.memory_index = int(results.angle_view[k, results.best_idex[k]])
                a.relocalised = bool(results.flags[k] & 32)           # (DV_RES_RELOCALISED: the step was the global search, by the rule)
                if a.relocalised:
                    a.n_relocalisations = getattr(a, "n_relocalisations", 0) + 1
                    self._step_windows[id(a)] = None                  # its scene_familiarity is the whole route's row: nothing is masked

    def _note_scene(self, agent, x, y, headings, weight):
        """NavEnsemble's note (a per-view extreme to work out when read, not the one-value models' fill), and the window of the step."""
        NavEnsemble._note_scene(self, agent, x, y, headings, weight)
        agent._scene_stale = (x, y, headings, weight, getattr(self, "_step_windows", {}).get(id(agent)))

    @staticmethod
    def _mask_scene(agent, stale):
        """A windowed step scored views [lo, hi) only: the others keep the reference's value for views never scored (:287)."""
        if len(stale) > 4 and stale[4] is not None:
            agent._scene_fam[:stale[4][0]] = np.inf
            agent._scene_fam[stale[4][1]:] = np.inf


class SadsRouteEnsemble(_WindowedMembers, _RouteEnsemble):
    """The route ensemble of the reference's own model, perfect memory (util.sads_familiarity): trials that differ in their start, their
    chem_weight, their TRAINING ROUTE and their LANDSCAPE step as one ensemble.  The engine keeps the sensed views of all routes side by
    side (FamiliarityEngine.rviews_set_from_poses: one call senses them all), and a step scores every running member's headings against
    the views of ITS OWN route under its own weight in ONE device call (dv_rviews_sense_step).  A member's angle_familiarity after a
    step is the reference's row bit for bit (what a lone agent made with exact=True gives at the same pose); its scene_familiarity is
    worked out when read (dv_rviews_scene), as NavEnsemble's members'.  A member's `memory_bank` is its route's place in the store.
    Made by from_routes / from_routes_with / from_landscapes (see _RouteEnsemble); chem_weights: one per member, default the model's.

    window=... makes members of perfect memory WITH A TEMPORAL WINDOW (sequence-aware matching): such a member carries `window` =
    (behind, ahead) and `memory_index`, the view of its own route its last applied step matched (angle_view of the heading it chose; a
    flagged or stopped member keeps its value).  With a memory_index m its step scores views [max(0, m - behind), min(len, m + ahead + 1))
    only (dv_rvwin_sense_step: one fused scoring launch), with the bits of oracle.step on that slice; with memory_index None (the
    first step without window_centres, or after relocalise()) it scores the whole route.  Its scene_familiarity is +inf outside the
    window of its last step.  Members without a window beside it step as ever: at most two device calls a step.

    relocalise_below=... gives windowed members a LOSS TEST: such a member carries `relocalise_below` (a familiarity, so at most
    max_familiarity), and a step whose largest windowed angle_familiarity is < that value (strictly, on the reference's doubles) is
    redone against the whole route INSIDE the same device call (dv_rvreloc_sense_step): the member's row, its memory_index and its
    scene_familiarity (nothing masked) are the whole-route step's, `relocalised` says that its last applied step was such a one, and
    `n_relocalisations` counts them.  A member that drifted off its window finds itself again without anybody calling relocalise()."""
    _metric = None
    _takes = "agents of the perfect-memory model (familiarity_model=sads_familiarity(...))"
    _info_call = "rviews_info"               # dict(n_routes, first int64[R + 1], shape, bytes)
    _one_route = "NavEnsemble"

    @classmethod
    def _check_model(cls, model):
        metric = getattr(model, "metric", None)
        if metric == "infomax":
            raise ValueError("SadsRouteEnsemble does not take an Infomax model: navsim_amd.InfomaxRouteEnsemble steps that one")
        if metric == "mushroom":
            raise ValueError("SadsRouteEnsemble does not take a mushroom-body model: navsim_amd.MushroomRouteEnsemble steps that one")
        if metric == "ncc":
            reject_ncc(model, "SadsRouteEnsemble")
        if metric is not None or not callable(getattr(model, "from_engine", None)) or getattr(model, "chem_weight", None) is None:
            if metric == "ssd":
                raise ValueError("SadsRouteEnsemble takes %s; navsim_amd.SsdRouteEnsemble steps the SSD model" % cls._takes)
            raise ValueError("SadsRouteEnsemble takes %s; the SSD models and foreign plug-ins have no routed form" % cls._takes)

    @classmethod
    def _check_member(cls, agent):
        func = getattr(agent, "_familiarity_func", None)
        cls._check_model(getattr(agent, "familiarity_model", None))
        if getattr(func, "metric", None) is not None:
            raise ValueError("SadsRouteEnsemble takes %s" % cls._takes)
        if getattr(agent, "_engine", None) is None:
            raise ValueError("SadsRouteEnsemble needs agents whose sensor model runs on the GPU (use_gpu_sensor=True)")
        if agent.training_path is None or func is None or getattr(func, "engine", None) is not agent._engine:
            raise ValueError("SadsRouteEnsemble needs the members from_routes makes")

    @staticmethod
    def _begin_model(model, eng, agent):
        """(nothing to begin: the store is made by the call that senses the routes)"""

    @staticmethod
    def _train_banks(eng, n_routes, x, y, headings, bank_of_view, land_of_view=None):
        first = np.concatenate([[0], np.cumsum(np.bincount(bank_of_view, minlength=n_routes))]).astype(np.int64)
        return eng.rviews_set_from_poses(x, y, headings, first, land_of_view=land_of_view)

    def __init__(self, agents, metrics="host"):
        super(SadsRouteEnsemble, self).__init__(agents, metrics=metrics)
        self._set_weights([a.chem_weight for a in self.agents])

    def _set_weights(self, weights):
        """Member i scores under weights[i] (None: the model's own), kept as its `chem_weight`."""
        w = [float(a.familiarity_model.chem_weight if x is None else x) for a, x in zip(self.agents, weights)]
        for a, x in zip(self.agents, w):
            a.chem_weight = x
        self._weights = np.array(w, dtype=np.float64)

    @staticmethod
    def _weights_arg(chem_weights, starts):
        if chem_weights is None:
            return None
        starts = list(starts)
        w = [float(x) for x in chem_weights]
        if len(w) != len(starts):
            raise ValueError("chem_weights holds %d weights for %d starts" % (len(w), len(starts)))
        if not all(0.0 <= x <= 1.0 for x in w):
            raise ValueError("chem_weights must lie in [0, 1], got %r" % (w,))
        return w

    @classmethod
    def from_routes_with(cls, agent, routes, starts, metrics="host", chem_weights=None, window=None, window_centres=None,
                         relocalise_below=None):
        """_RouteEnsemble.from_routes_with, and chem_weights: member i scores under chem_weights[i] (None: the model's weight).
        window: None (perfect memory: every step scores the whole route), or perfect memory with a temporal window -- an int W
        (W views behind and W ahead of the view the member matched last), a pair (behind, ahead), or a list with such an entry, or
        None, per start.  window_centres: a list with the initial `memory_index` (a view of the member's own route) or None per start;
        a windowed member without one scores its whole route in its first step (see the class).  relocalise_below: None, a float (every
        member's threshold), or a list with a float or None per start; a member with a threshold must have a window."""
        starts = list(starts)
        w = cls._weights_arg(chem_weights, starts)
        routes = list(routes)
        wins, centres = cls._windows_arg(window, window_centres, starts, [len(r) for r in routes])
        thresholds = cls._thresholds_arg(relocalise_below, wins)
        ens = cls._from_routes(agent, routes, starts, metrics, None, None)
        if w is not None:
            ens._set_weights(w)
        ens._set_windows(wins, centres, thresholds)
        return ens

    @classmethod
    def from_landscapes(cls, agent, landscapes, routes, starts, metrics="host", chem_weights=None, sensors=None, window=None,
                        window_centres=None, relocalise_below=None, noise=None):
        """_RouteEnsemble.from_landscapes (noise included), and chem_weights, window, window_centres and relocalise_below as
        from_routes_with takes them.  A windowed ensemble's two calls per step each get their own members' noise rows."""
        starts = list(starts)
        w = cls._weights_arg(chem_weights, starts)
        routes = list(routes)
        lengths = [len(rt[1]) if isinstance(rt, (tuple, list)) and len(rt) == 2 else 0 for rt in routes]
        wins, centres = cls._windows_arg(window, window_centres, starts, lengths)
        thresholds = cls._thresholds_arg(relocalise_below, wins)
        ens = super(SadsRouteEnsemble, cls).from_landscapes(agent, landscapes, routes, starts, metrics=metrics, sensors=sensors, noise=noise)
        if w is not None:
            ens._set_weights(w)
        ens._set_windows(wins, centres, thresholds)
        return ens

    def _device_step(self, idx, xs, ys, angs):
        """A member with a window and a centre goes to rvwin_sense_step, every other to rviews_sense_step: at most two device calls, and
        with no window anywhere the one call there was.  Where a member of the windowed call has a threshold (relocalise_below) the call
        carries every member's (-inf for those without: never lost), and a lost member's row comes back as the whole route's; with no
        threshold anywhere the calls are the ones there were.  The results come back as one RouteViewResults in the caller's order."""
        from .engine import RouteViewResults
        wins = [self._window_of(self.agents[i]) for i in idx]
        lands = None if self._lands is None else self._lands[idx]
        self._step_windows = {id(self.agents[i]): w for i, w in zip(idx, wins)}
        ks = [k for k, w in enumerate(wins) if w is not None]
        self._noise_begin_step(idx)
        if not ks:
            self._noise_set_rows([self.agents[i] for i in idx])
            results = self.engine.rviews_sense_step(xs, ys, angs, self._banks[idx], self._weights[idx], land_of_member=lands)
        else:
            xs, ys, angs = np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64), np.asarray(angs, dtype=np.float64)
            banks, weights = self._banks[idx], self._weights[idx]
            rest = [k for k, w in enumerate(wins) if w is None]
            taus = [getattr(self.agents[idx[k]], "relocalise_below", None) for k in ks]
            more = {} if all(t is None for t in taus) else dict(reloc_below=np.array([-np.inf if t is None else t for t in taus]))
            self._noise_set_rows([self.agents[idx[k]] for k in ks])
            parts = [(ks, self.engine.rvwin_sense_step(xs[ks], ys[ks], angs[ks], banks[ks], weights[ks], [wins[k][0] for k in ks],
                                                       [wins[k][1] for k in ks], land_of_member=None if lands is None else lands[ks], **more))]
            if rest:
                self._noise_set_rows([self.agents[idx[k]] for k in rest])
                parts.append((rest, self.engine.rviews_sense_step(xs[rest], ys[rest], angs[rest], banks[rest], weights[rest],
                                                                  land_of_member=None if lands is None else lands[rest])))
            n, A = angs.shape
            results = RouteViewResults(np.empty((n, A)), np.empty((n, A), dtype=np.int64), np.empty(n, dtype=np.int32),
                                       np.empty(n, dtype=np.uint32))
            for at, r in parts:
                results.angle_familiarity[at], results.angle_view[at] = r.angle_familiarity, r.angle_view
                results.best_idex[at], results.flags[at] = r.best_idex, r.flags
        self._remember_views(idx, results)
        return results

    def _read_scene(self):
        todo = [a for a in self.agents if a._scene_stale is not None and a._scene_owner is self]
        if not todo:
            return
        st = [a._scene_stale for a in todo]
        lands = None if self._lands is None else [a.landscape_index for a in todo]
        self._noise_set_rows(todo)                                # (the scene of the patches the last step scored: its keys)
        rows = self.engine.rviews_scene([t[0] for t in st], [t[1] for t in st], np.stack([t[2] for t in st]), [a.memory_bank for a in todo],
                                        [t[3] for t in st], land_of_member=lands)
        for a, row, t in zip(todo, rows, st):
            a._scene_stale = None
            a._scene_owner = None
            a._scene_fam[:] = row
            self._mask_scene(a, t)

    def scene_familiarity(self):
        """A list of float64[len(route of member i)]: every member's scene_familiarity after its last step, as NavEnsemble gives it
        (the rows are as long as the members' own routes, so they do not stack)."""
        if any(not a.track_scene_familiarity for a in self.agents):
            raise ValueError("construct the agents with track_scene_familiarity=True (the default) to read scene_familiarity")
        self._read_scene()
        return [a.scene_familiarity.copy() for a in self.agents]


class SsdRouteEnsemble(_WindowedMembers, _RouteEnsemble):
    """The route ensemble of the north star's literal metric, the sum of squared differences (util.ssd_familiarity(channel)): trials
    that differ in their start, their TRAINING ROUTE and their LANDSCAPE step as one ensemble.  The views of all routes lie in the
    engine's route view store (FamiliarityEngine.rviews_set_from_poses: one call senses them all, the store SadsRouteEnsemble uses),
    and a step scores channel `channel` of every running member's headings against the views of ITS OWN route on the int8 matrix cores
    in ONE device call (dv_rvssd_sense_step).  Every score is the exact integer of the reference's `ssds`, so a member's
    angle_familiarity (-SSD) is a lone agent's row bit for bit, and ties go to the first heading as np.argmax decides them.  A
    member's scene_familiarity is worked out when read (dv_rvssd_scene); its `memory_bank` is its route's place in the store.
    All members share the model's one channel.  Made by from_routes / from_routes_with / from_landscapes (see _RouteEnsemble).

    window=..., window_centres=..., relocalise_below=... and relocalise() are SadsRouteEnsemble's, with its members' attributes
    (window, memory_index, relocalise_below, relocalised, n_relocalisations): a member with a window and a memory_index m scores views
    [max(0, m - behind), min(len, m + ahead + 1)) of its route only (dv_rvssdw_sense_step: exact SSD on that slice), a member without
    either scores its whole route, at most two device calls a step.  relocalise_below is a familiarity, -SSD, so useful values are
    <= 0: a step whose largest windowed angle_familiarity is < it is redone against the whole route inside the same device call.
    scene_familiarity is +inf outside the window of a member's last step, and unmasked after a re-localised one."""
    _metric = "ssd"
    _takes = "agents of the SSD model (familiarity_model=ssd_familiarity(channel))"
    _info_call = "rviews_info"               # dict(n_routes, first int64[R + 1], shape, bytes)
    _one_route = "a lone NavBySceneFamiliarity"

    @classmethod
    def from_agent(cls, agent, poses):
        raise ValueError("SsdRouteEnsemble is made from routes (from_routes): it takes an untrained agent and trains every route itself")

    @classmethod
    def _reject_others(cls, agent):
        for obj in (agent, getattr(agent, "familiarity_model", None), getattr(agent, "_familiarity_func", None)):
            metric = getattr(obj, "metric", None)
            if metric == "infomax":
                raise ValueError("SsdRouteEnsemble does not take an Infomax model: navsim_amd.InfomaxRouteEnsemble steps that one")
            if metric == "mushroom":
                raise ValueError("SsdRouteEnsemble does not take a mushroom-body model: navsim_amd.MushroomRouteEnsemble steps that one")
            if metric == "ncc":
                reject_ncc(obj, "SsdRouteEnsemble")

    @classmethod
    def _reject_banked(cls, agent):
        """Its own members are the banked ones; another route ensemble's are refused by name."""
        if getattr(agent, "memory_bank", None) is not None and route_ensemble_name(agent) != cls.__name__:
            reject_banked(agent, cls.__name__)

    @classmethod
    def _check_model(cls, model):
        cls._reject_others(model)
        if getattr(model, "metric", None) != "ssd" or getattr(model, "channel", None) not in (0, 1, 2):
            if getattr(model, "metric", None) is None and getattr(model, "chem_weight", None) is not None:
                raise ValueError("SsdRouteEnsemble does not take a perfect-memory model: navsim_amd.SadsRouteEnsemble steps that one")
            raise ValueError("SsdRouteEnsemble takes %s" % cls._takes)

    @classmethod
    def _check_member(cls, agent):
        func = getattr(agent, "_familiarity_func", None)
        cls._reject_banked(agent)
        cls._check_model(getattr(agent, "familiarity_model", None))
        if getattr(agent, "_engine", None) is None:
            raise ValueError("SsdRouteEnsemble needs agents whose sensor model runs on the GPU (use_gpu_sensor=True)")
        if agent.training_path is None or func is None or getattr(func, "engine", None) is not agent._engine:
            raise ValueError("SsdRouteEnsemble needs the members from_routes makes")

    @staticmethod
    def _begin_model(model, eng, agent):
        """(nothing to begin: the store is made by the call that senses the routes)"""

    _train_banks = staticmethod(SadsRouteEnsemble._train_banks)

    def __init__(self, agents, metrics="host"):
        channels = [getattr(getattr(a, "familiarity_model", None), "channel", None) for a in agents]
        for i, ch in enumerate(channels):
            if ch in (0, 1, 2) and ch != channels[0] and channels[0] in (0, 1, 2):
                raise ValueError("SsdRouteEnsemble: member %d compares channel %d, member 0 channel %d: the members of an ensemble share "
                                 "one channel" % (i, ch, channels[0]))
        super(SsdRouteEnsemble, self).__init__(agents, metrics=metrics)
        self.channel = int(channels[0])

    @classmethod
    def from_routes_with(cls, agent, routes, starts, metrics="host", window=None, window_centres=None, relocalise_below=None):
        """_RouteEnsemble.from_routes_with, and window, window_centres and relocalise_below as SadsRouteEnsemble.from_routes_with takes
        them (relocalise_below in the unit of angle_familiarity, -SSD)."""
        starts, routes = list(starts), list(routes)
        wins, centres = cls._windows_arg(window, window_centres, starts, [len(r) for r in routes])
        thresholds = cls._thresholds_arg(relocalise_below, wins)
        ens = cls._from_routes(agent, routes, starts, metrics, None, None)
        ens._set_windows(wins, centres, thresholds)
        return ens

    @classmethod
    def from_landscapes(cls, agent, landscapes, routes, starts, metrics="host", sensors=None, window=None, window_centres=None,
                        relocalise_below=None, noise=None):
        """_RouteEnsemble.from_landscapes (noise included), and window, window_centres and relocalise_below as from_routes_with takes
        them."""
        starts, routes = list(starts), list(routes)
        lengths = [len(rt[1]) if isinstance(rt, (tuple, list)) and len(rt) == 2 else 0 for rt in routes]
        wins, centres = cls._windows_arg(window, window_centres, starts, lengths)
        thresholds = cls._thresholds_arg(relocalise_below, wins)
        ens = super(SsdRouteEnsemble, cls).from_landscapes(agent, landscapes, routes, starts, metrics=metrics, sensors=sensors, noise=noise)
        ens._set_windows(wins, centres, thresholds)
        return ens

    def _device_step(self, idx, xs, ys, angs):
        """A member with a window and a centre goes to rvssdw_sense_step, every other to rvssd_sense_step: at most two device calls,
        and with no window anywhere the one call there was.  Where a member of the windowed call has a threshold (relocalise_below) the
        call carries every member's (-inf for those without: never lost).  The results come back as one RouteSsdResults in the caller's
        order."""
        from .engine import RouteSsdResults
        wins = [self._window_of(self.agents[i]) for i in idx]
        lands = None if self._lands is None else self._lands[idx]
        self._step_windows = {id(self.agents[i]): w for i, w in zip(idx, wins)}
        ks = [k for k, w in enumerate(wins) if w is not None]
        self._noise_begin_step(idx)
        if not ks:
            self._noise_set_rows([self.agents[i] for i in idx])
            results = self.engine.rvssd_sense_step(xs, ys, angs, self._banks[idx], self.channel, land_of_member=lands)
        else:
            xs, ys, angs = np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64), np.asarray(angs, dtype=np.float64)
            banks = self._banks[idx]
            rest = [k for k, w in enumerate(wins) if w is None]
            taus = [getattr(self.agents[idx[k]], "relocalise_below", None) for k in ks]
            more = {} if all(t is None for t in taus) else dict(reloc_below=np.array([-np.inf if t is None else t for t in taus]))
            self._noise_set_rows([self.agents[idx[k]] for k in ks])
            parts = [(ks, self.engine.rvssdw_sense_step(xs[ks], ys[ks], angs[ks], banks[ks], [wins[k][0] for k in ks], [wins[k][1] for k in ks],
                                                        self.channel, land_of_member=None if lands is None else lands[ks], **more))]
            if rest:
                self._noise_set_rows([self.agents[idx[k]] for k in rest])
                parts.append((rest, self.engine.rvssd_sense_step(xs[rest], ys[rest], angs[rest], banks[rest], self.channel,
                                                                 land_of_member=None if lands is None else lands[rest])))
            n, A = angs.shape
            results = RouteSsdResults(np.empty((n, A)), np.empty((n, A), dtype=np.int64), np.empty(n, dtype=np.int32),
                                      np.empty(n, dtype=np.uint32))
            for at, r in parts:
                results.angle_ssd[at], results.angle_familiarity[at], results.angle_view[at] = r.angle_ssd, r.angle_familiarity, r.angle_view
                results.best_idex[at], results.flags[at] = r.best_idex, r.flags
        self._remember_views(idx, results)
        return results

    def _read_scene(self):
        todo = [a for a in self.agents if a._scene_stale is not None and a._scene_owner is self]
        if not todo:
            return
        st = [a._scene_stale for a in todo]
        lands = None if self._lands is None else [a.landscape_index for a in todo]
        self._noise_set_rows(todo)                                # (the scene of the patches the last step scored: its keys)
        rows = self.engine.rvssd_scene([t[0] for t in st], [t[1] for t in st], np.stack([t[2] for t in st]), [a.memory_bank for a in todo],
                                       self.channel, land_of_member=lands)
        for a, row, t in zip(todo, rows, st):
            a._scene_stale = None
            a._scene_owner = None
            np.negative(row, out=a._scene_fam)                    # min over headings of -SSD = -(max over headings of SSD)
            self._mask_scene(a, t)

    scene_familiarity = SadsRouteEnsemble.scene_familiarity


class NccRouteEnsemble(_RouteEnsemble):
    """The route ensemble of the correlation coefficient (util.ncc_familiarity(channel)): SsdRouteEnsemble without the window arguments,
    for the metric that does not change with the gain and offset of a view.  The views of all routes lie in the engine's route view
    store (FamiliarityEngine.rviews_set_from_poses: one call senses them all), and a step scores channel `channel` of every running
    member's headings against the views of ITS OWN route in ONE device call (dv_rvncc_sense_step: SSD's int8 GEMM and a 64-bit
    epilogue).  A member's angle_familiarity is a lone agent's row bit for bit, and ties go to the first heading as np.argmax decides
    them.  A member's scene_familiarity is worked out when read (dv_rvncc_scene); its `memory_bank` is its route's place in the store.
    All members share the model's one channel.  Made by from_routes / from_routes_with / from_landscapes (see _RouteEnsemble).
    Not built: windows and re-localisation, a channel per member."""
    _metric = "ncc"
    _takes = "agents of the NCC model (familiarity_model=ncc_familiarity(channel))"
    _info_call = "rviews_info"               # dict(n_routes, first int64[R + 1], shape, bytes)
    _one_route = "a lone NavBySceneFamiliarity"

    @classmethod
    def from_agent(cls, agent, poses):
        raise ValueError("NccRouteEnsemble is made from routes (from_routes): it takes an untrained agent and trains every route itself")

    @classmethod
    def _reject_ncc(cls, agent):
        """(its own model)"""

    @classmethod
    def _reject_others(cls, agent):
        for obj in (agent, getattr(agent, "familiarity_model", None), getattr(agent, "_familiarity_func", None)):
            metric = getattr(obj, "metric", None)
            if metric == "infomax":
                raise ValueError("NccRouteEnsemble does not take an Infomax model: navsim_amd.InfomaxRouteEnsemble steps that one")
            if metric == "mushroom":
                raise ValueError("NccRouteEnsemble does not take a mushroom-body model: navsim_amd.MushroomRouteEnsemble steps that one")
            if str(metric).startswith("ssd"):
                raise ValueError("NccRouteEnsemble does not take an SSD model: navsim_amd.SsdRouteEnsemble steps that one")

    @classmethod
    def _reject_banked(cls, agent):
        """Its own members are the banked ones; another route ensemble's are refused by name."""
        if getattr(agent, "memory_bank", None) is not None and route_ensemble_name(agent) != cls.__name__:
            reject_banked(agent, cls.__name__)

    @classmethod
    def _check_model(cls, model):
        cls._reject_others(model)
        if getattr(model, "metric", None) != "ncc" or getattr(model, "channel", None) not in (0, 1, 2):
            if getattr(model, "metric", None) is None and getattr(model, "chem_weight", None) is not None:
                raise ValueError("NccRouteEnsemble does not take a perfect-memory model: navsim_amd.SadsRouteEnsemble steps that one")
            raise ValueError("NccRouteEnsemble takes %s" % cls._takes)

    @classmethod
    def _check_member(cls, agent):
        func = getattr(agent, "_familiarity_func", None)
        cls._reject_banked(agent)
        cls._check_model(getattr(agent, "familiarity_model", None))
        if getattr(agent, "_engine", None) is None:
            raise ValueError("NccRouteEnsemble needs agents whose sensor model runs on the GPU (use_gpu_sensor=True)")
        if agent.training_path is None or func is None or getattr(func, "engine", None) is not agent._engine:
            raise ValueError("NccRouteEnsemble needs the members from_routes makes")

    @staticmethod
    def _begin_model(model, eng, agent):
        """(nothing to begin: the store is made by the call that senses the routes)"""

    _train_banks = staticmethod(SadsRouteEnsemble._train_banks)

    def __init__(self, agents, metrics="host"):
        channels = [getattr(getattr(a, "familiarity_model", None), "channel", None) for a in agents]
        for i, ch in enumerate(channels):
            if ch in (0, 1, 2) and ch != channels[0] and channels[0] in (0, 1, 2):
                raise ValueError("NccRouteEnsemble: member %d compares channel %d, member 0 channel %d: the members of an ensemble share "
                                 "one channel" % (i, ch, channels[0]))
        super(NccRouteEnsemble, self).__init__(agents, metrics=metrics)
        self.channel = int(channels[0])

    @classmethod
    def from_routes_with(cls, agent, routes, starts, metrics="host"):
        """_RouteEnsemble.from_routes_with (there are no populations, and no windows)."""
        return cls._from_routes(agent, list(routes), list(starts), metrics, None, None)

    @classmethod
    def from_landscapes(cls, agent, landscapes, routes, starts, metrics="host", sensors=None, noise=None):
        """_RouteEnsemble.from_landscapes, sensors and noise included (there are no populations, and no windows)."""
        return super(NccRouteEnsemble, cls).from_landscapes(agent, landscapes, routes, starts, metrics=metrics, sensors=sensors, noise=noise)

    def _device_step(self, idx, xs, ys, angs):
        lands = None if self._lands is None else self._lands[idx]
        self._noise_begin_step(idx)
        self._noise_set_rows([self.agents[i] for i in idx])
        return self.engine.rvncc_sense_step(xs, ys, angs, self._banks[idx], self.channel, land_of_member=lands)

    _note_scene = NavEnsemble._note_scene    # a per-view minimum to work out when read, not the one-value models' fill

    def _read_scene(self):
        todo = [a for a in self.agents if a._scene_stale is not None and a._scene_owner is self]
        if not todo:
            return
        st = [a._scene_stale for a in todo]
        lands = None if self._lands is None else [a.landscape_index for a in todo]
        self._noise_set_rows(todo)                                # (the scene of the patches the last step scored: its keys)
        rows = self.engine.rvncc_scene([t[0] for t in st], [t[1] for t in st], np.stack([t[2] for t in st]), [a.memory_bank for a in todo],
                                       self.channel, land_of_member=lands)
        for a, row in zip(todo, rows):
            a._scene_stale = None
            a._scene_owner = None
            a._scene_fam[:] = row

    scene_familiarity = SadsRouteEnsemble.scene_familiarity
