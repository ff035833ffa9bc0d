"""Scenes for task sets (tests/test_emulated_task_sets.py, tests/test_gpu_task_sets.py): a pool entry names
the task its episode is played under (swb_set_task_sets, swb_set_entry_task_sets).

The expectation comes from the oracle as it is, which knows no task sets: for every set g one `oracle.Engine(cfg_g, pool_g)` whose
configuration holds the set's task alone (`split`) and whose pool gives environment n the entries of ITS range that are played
under set g, in order.  The oracle's environments are independent of each other and `step(a, env_range=(n, n + 1))` steps one of
them, so environment n of oracle g IS the oracle "(n, g)": while environment n of the engine is in an episode of set g, it is
compared with environment n of oracle g.  The per-set subsequence of a cyclic entry list is itself cyclic, so the wrap-around of
the pool needs nothing more.  `Mixed` holds the oracles behind the surface of one and maps `episode` and `pool_entry`; every step
goes through the bar of tests/_parity.py.

What a stepping case must have seen -- decided on the oracle's side alone -- is asserted by `Mixed.assert_saw_everything`: a case
that misses one of the conditions fails rather than passing empty.  Seeds and task parameters were picked on the emulator so that
they hold at both batch sizes.
"""
import copy
import ctypes as C

import numpy as np

from spriteworld_amd import _abi
from spriteworld_amd import lowering
from spriteworld_amd import tasks
from spriteworld_amd import workloads
from tests import _parity

EPISODES_PER_ENV = 4          # with three sets the cycle does not divide the pool length
STEPS = 48


def copy_cfg(cfg):
  return _abi.SwbConfig.from_buffer_copy(bytes(cfg))


# --------------------------------------------------------------------------------------------------------------------------
# the oracle's side
# --------------------------------------------------------------------------------------------------------------------------
def split(cfg, sets, pool, set_of_entry=None):
  """[(cfg_g, pool_g)]: per set, the configuration with that set's task alone and the pool of the entries played under it --
  environment n's range holds the entries of its range in the mixed pool that name set g, in order (an environment without any
  gets entry 0, which it never plays)."""
  which = pool.task_set if set_of_entry is None else np.asarray(set_of_entry)
  out = []
  for g, s in enumerate(sets):
    c = copy_cfg(cfg)
    c.n_tasks, c.is_meta = s.n_tasks, s.is_meta
    c.meta_aggregator, c.meta_termination, c.meta_terminate_bonus = s.meta_aggregator, s.meta_termination, s.meta_terminate_bonus
    c.max_episode_length = s.max_episode_length
    for t in range(_abi.SWB_MAX_TASKS):
      c.tasks[t] = cfg.tasks[s.first_task + t] if t < s.n_tasks else _abi.SwbTask()
    idx, base, length = [], [], []
    for n in range(cfg.n_envs):
      mine = [e for e in range(pool.pool_base[n], pool.pool_base[n] + pool.pool_len[n]) if which[e] == g]
      base.append(len(idx) if mine else 0)
      length.append(max(len(mine), 1))
      idx.extend(mine)
    idx = np.asarray(idx or [0], np.int64)
    pg = lowering.Pool(len(idx), cfg.max_sprites, s.n_tasks)
    pg.n_sprites[:] = pool.n_sprites[idx]
    for name in lowering._POOL_SPRITE_ARRAYS:
      getattr(pg, name)[:] = getattr(pool, name)[idx]
    pg.label[:] = pool.label[idx, s.first_task:s.first_task + s.n_tasks]
    if pool.cell_label is not None:
      pg.cell_label = np.ascontiguousarray(pool.cell_label[idx, s.first_task:s.first_task + s.n_tasks])
    pg.pool_base, pg.pool_len = np.asarray(base, np.int32), np.asarray(length, np.int32)
    out.append((c, pg))
  return out


class Mixed(object):
  """The oracles of every set behind the surface of one oracle.Engine (step with env_range, state, render, evaluate,
  set_positions, set_sprite_attr), and what the run has seen."""

  def __init__(self, cfg, sets, pool):
    from oracle import oracle
    self.cfg, self.sets, self.N, self.G = cfg, sets, cfg.n_envs, len(sets)
    self.parts = split(cfg, sets, pool)
    self.oras = [oracle.Engine(c, p) for c, p in self.parts]
    self.base, self.len = np.asarray(pool.pool_base), np.asarray(pool.pool_len)
    self.set_of_entry = np.asarray(pool.task_set).copy()
    self.episode = np.zeros(self.N, np.int32)
    self.entry = np.zeros(self.N, np.int32)
    self.cur = np.zeros(self.N, np.int64)             # the set of the episode the environment is in
    self.pending = np.ones(self.N, bool)
    self.steps = np.zeros(self.N, np.int64)
    # can a set's task succeed at all?  (NoReward.success() is False whatever the sprites do: tasks.py:78-81)
    self.can_succeed = [any(cfg.tasks[s.first_task + t].kind != _abi.TASK_NO_REWARD for t in range(s.n_tasks)) for s in sets]
    self.episodes_of = np.zeros(self.G, np.int64)
    self.last_by_success = np.zeros(self.G, bool)
    self.last_by_timeout = np.zeros(self.G, bool)
    self.saw_switch = self.saw_wrap = False

  def step(self, a, render=True, env_range=None):
    i0, i1 = (0, self.N) if env_range is None else env_range
    res = None
    for n in range(i0, i1):
      if self.pending[n]:
        e = int(self.base[n] + self.episode[n] % self.len[n])
        g = int(self.set_of_entry[e])
        self.saw_switch |= bool(self.episode[n] > 0 and g != self.cur[n])
        self.saw_wrap |= bool(self.episode[n] >= self.len[n])
        self.episodes_of[g] += 1
        self.cur[n], self.entry[n], self.steps[n] = g, e, 0
        self.episode[n] += 1
      else:
        self.steps[n] += 1
      g = int(self.cur[n])
      o = self.oras[g].step(a, render=render, env_range=(n, n + 1))
      if res is None:
        res = {k: (None if v is None else np.zeros_like(v)) for k, v in o.items()}
      for k, v in o.items():
        if v is not None:
          res[k][n] = v[n]
      last = o['step_type'][n] == _abi.STEP_LAST
      if last and o['success'][n]:
        self.last_by_success[g] = True
      elif last and self.steps[n] >= self.sets[g].max_episode_length:
        self.last_by_timeout[g] = True
      self.pending[n] = last
    return res

  def _gather(self, per_oracle):
    return np.stack([per_oracle[int(self.cur[n])][n] for n in range(self.N)])

  def state(self):
    sts = [o.state() for o in self.oras]
    st = {k: self._gather([s[k] for s in sts]) for k in ('x', 'y', 'n_sprites', 'step_count', 'reset_next')}
    st['episode'], st['pool_entry'] = self.episode.copy(), self.entry.copy()
    return st

  def render(self):
    return self._gather([o.render() for o in self.oras])

  def evaluate(self):
    return self._gather([o.evaluate() for o in self.oras])

  def set_sprite_attr(self, env, sprite, attr, value):
    self.oras[int(self.cur[env])].set_sprite_attr(env, sprite, attr, value)

  def task_sets(self):
    return self.cur.astype(np.int32)

  def assert_saw_everything(self, what):
    assert (self.episodes_of >= 2).all(), (what, 'a set was played in fewer than two episodes', self.episodes_of)
    for g in range(self.G):
      assert self.last_by_timeout[g], (what, 'set %d saw no LAST by its own timeout' % g)
      assert self.last_by_success[g] or not self.can_succeed[g], (what, 'set %d saw no LAST by success' % g)
    assert self.saw_switch, (what, 'no environment played consecutive episodes of different sets')
    assert self.saw_wrap, (what, 'no episode started after its pool had wrapped')


# --------------------------------------------------------------------------------------------------------------------------
# scenes
# --------------------------------------------------------------------------------------------------------------------------
def _relax(cfg, terminate_distance=None, threshold=None, any_of=False):
  """Task parameters under which a random agent both succeeds and times out within a few dozen steps."""
  for t in range(cfg.n_tasks):
    if cfg.tasks[t].kind == _abi.TASK_FIND_GOAL and terminate_distance is not None:
      cfg.tasks[t].terminate_distance = terminate_distance
    if cfg.tasks[t].kind == _abi.TASK_CLUSTERING and threshold is not None:
      cfg.tasks[t].termination_threshold = threshold
  if any_of and cfg.is_meta:
    cfg.meta_termination = _abi.TERM_ANY


def _merge(parts, n_envs, assignment='cycle'):
  which = lowering.task_set_assignment(assignment, n_envs, EPISODES_PER_ENV, len(parts))
  return lowering.merge_task_sets(parts, which.reshape(-1))


def mix_s5(n_envs, aa, seed=0, lengths=(6, 9, 12), assignment='cycle'):
  """goal_s5 + cluster_s5 + sorting_s4: six sub-tasks, the sorting scenes padded from four to five sprite slots."""
  parts = []
  for g, (name, relax) in enumerate((('goal_s5', dict(terminate_distance=0.3)), ('cluster_s5', dict(threshold=0.9)),
                                     ('sorting_s4', dict(terminate_distance=0.3, any_of=True)))):
    cfg, pool, sample = workloads.build(name, n_envs, EPISODES_PER_ENV, seed + g, aa)
    cfg.max_episode_length = lengths[g]
    _relax(cfg, **relax)
    parts.append((cfg, pool))
  cfg, sets, pool = _merge(parts, n_envs, assignment)
  assert cfg.n_tasks == 6 and cfg.max_sprites == 5
  return cfg, sets, pool, _sampler(cfg)


def same_scene(name, n_envs, aa, seed=0, lengths=(6, 9, 12), kinds=('own', 'goal', 'none'), goal_cut=None, relax=None,
               goal_distance=0.3):
  """One workload's scenes under several tasks: its own, FindGoalPosition over the sprites its task's sub-task 0 labels 0 (for
  FindGoalPosition tasks: 1), and NoReward.  Every entry is labelled for EVERY set (the sprites are the same), so that a
  reassignment of entries is meaningful.  goal_cut: a y-threshold the FindGoalPosition filter also keys on."""
  cfg, pool, _ = workloads.build(name, n_envs, EPISODES_PER_ENV, seed, aa)
  _relax(cfg, **(relax or {}))
  own_kind = cfg.tasks[0].kind
  parts = []
  for g, kind in enumerate(kinds):
    c, pl = copy_cfg(cfg), copy.deepcopy(pool)
    if kind != 'own':
      c.n_tasks, c.is_meta, c.meta_aggregator, c.meta_termination, c.meta_terminate_bonus = 1, 0, 0, 0, 0.0
      for t in range(_abi.SWB_MAX_TASKS):
        c.tasks[t] = _abi.SwbTask()
      pl = lowering.Pool(pool.n_entries, pool.max_sprites, 1)
      for arr in lowering._POOL_SPRITE_ARRAYS + ('n_sprites',):
        getattr(pl, arr)[:] = getattr(pool, arr)
      pl.pool_base, pl.pool_len = pool.pool_base.copy(), pool.pool_len.copy()
    if kind == 'goal':
      lowering._lower_task(tasks.FindGoalPosition(filter_distrib=None, goal_position=(0.4, 0.6), terminate_distance=goal_distance,
                                                  raw_reward_multiplier=30., terminate_bonus=2.), c.tasks[0], bool(cfg.pos_is_f32))
      member = (pool.label[:, 0, :] == (1 if own_kind == _abi.TASK_FIND_GOAL else 0)).astype(np.int8)
      pl.label[:, 0, :] = member
      if goal_cut is not None:      # members only at y >= goal_cut: cell 1 of a grid of one y-cut
        c.tasks[0].n_ycuts, c.tasks[0].ycuts[0] = 1, goal_cut
        pl.cell_label = np.zeros((pool.n_entries, 1, pool.max_sprites, _abi.SWB_MAX_CELLS), np.int8)
        pl.cell_label[:, 0, :, 1] = member
    elif kind == 'none':
      c.tasks[0].kind = _abi.TASK_NO_REWARD
    c.max_episode_length = lengths[g]
    parts.append((c, pl))
  cfg_m, sets, pool_m = _merge(parts, n_envs)
  # every entry labelled for every set
  first = 0
  for c, pl in parts:
    pool_m.label[:, first:first + c.n_tasks] = pl.label
    if pl.cell_label is not None:
      pool_m.cell_label[:, first:first + c.n_tasks] = pl.cell_label
    first += c.n_tasks
  return cfg_m, sets, pool_m, _sampler(cfg_m)


def _sampler(cfg):
  """Random actions that move things: three clicks in four land on the centre of a random sprite of the environment (given the
  model's state), the motion is uniform."""
  N = cfg.n_envs

  def sample(rng, state=None):
    if cfg.action_space == _abi.ACTION_EMBODIED:
      return np.stack([rng.integers(0, 2, N), rng.integers(0, 4, N)], 1).astype(np.int32)
    a = rng.uniform(0.0, 1.0, size=(N, 4))
    if state is not None:
      for n in range(N):
        k = int(state['n_sprites'][n])
        if k and rng.random() < 0.75:
          s = int(rng.integers(0, k))
          a[n, 0], a[n, 1] = state['x'][n, s], state['y'][n, s]
          if cfg.action_space == _abi.ACTION_DRAG_AND_DROP:
            a[n, 2:] = a[n, :2] + rng.uniform(-0.5, 0.5, 2)
    return a.astype(np.float32) if cfg.action_is_f32 else a
  return sample


def null_actions(cfg):
  """A click that meets no sprite and moves nothing (Embodied: no such action)."""
  a = np.zeros((cfg.n_envs, 4), np.float32 if cfg.action_is_f32 else np.float64)
  a[:, :2] = -3.0
  a[:, 2:] = 0.5
  return a


# (scene builder, its arguments, environment of the engine, entries of variant() that must hold, environments emulated / on the GPU)
SCENES = {
    'mix_s5_aa5': (mix_s5, dict(aa=5), (), {'large_frames': 0, 'many_sprites': 0, 'paint_in_cover': 0}, (5, 14)),
    'mix_s5_aa1': (mix_s5, dict(aa=1, seed=2), (), {'paint_in_cover': 1}, (5, 14)),
    'mix_s5_large_frames': (mix_s5, dict(aa=5, seed=4), (('SWB_LARGE_FRAMES', '1'),), {'large_frames': 1, 'many_sprites': 0}, (5, 12)),
    'f64_cluster_f32a': (same_scene, dict(name='f64_cluster_f32a', aa=3, relax=dict(threshold=0.8)), (),
                         {'large_frames': 0, 'many_sprites': 0}, (5, 14)),
    'embodied_s12': (same_scene, dict(name='embodied_s12', aa=5, kinds=('own', 'none'), lengths=(7, 4),
                                      relax=dict(terminate_distance=0.31)), (), {'large_frames': 0, 'many_sprites': 0}, (4, 12)),
    'cluster_s40': (same_scene, dict(name='cluster_s40', aa=2, kinds=('own', 'goal'), lengths=(5, 8), relax=dict(threshold=0.14),
                                     goal_distance=0.44), (), {'many_sprites': 1}, (4, 12)),
    'meta_s24_f64': (same_scene, dict(name='meta_s24_f64', aa=2, kinds=('own', 'goal'), lengths=(9, 6), goal_cut=0.5,
                                      goal_distance=0.5, relax=dict(terminate_distance=0.2)), (), {'many_sprites': 1}, (4, 12)),
}


def build_scene(which, gpu):
  fn, kw, env, expect, sizes = SCENES[which]
  return fn(n_envs=sizes[1 if gpu else 0], **kw), env, expect


# --------------------------------------------------------------------------------------------------------------------------
# the engine beside the oracles
# --------------------------------------------------------------------------------------------------------------------------
def new_engine(make_engine, cfg, sets, pool):
  """An engine with task sets: created without a pool, given its sets, then its pool (Engine.set_pool uploads Pool.task_set)."""
  eng = make_engine(cfg, None)
  if sets is not None:
    eng.set_task_sets(sets)
  eng.set_pool(pool)
  return eng


class Runner(object):

  def __init__(self, make_engine, monkeypatch, scene, what, env=(), expect=None, stats=False):
    for k, v in env:
      monkeypatch.setenv(k, v)
    if stats:
      monkeypatch.setenv('SWB_LIST_STATS', '1')
    self.cfg, self.sets, self.pool, self.sample = scene
    self.what, self.t, self.N = what, 0, self.cfg.n_envs
    self.ora = Mixed(self.cfg, self.sets, self.pool)
    self.eng = new_engine(make_engine, self.cfg, self.sets, self.pool)
    v = self.eng.variant()
    for k, value in (expect or {}).items():
      assert v[k] == value, (what, k, v)
    self.held = None

  def step(self, a, active=None):
    act = np.ones(self.N, bool) if active is None else np.asarray(active, bool)
    want = None if self.held is None else {k: v.copy() for k, v in self.held.items()}
    for n in np.flatnonzero(act):
      out = self.ora.step(a, env_range=(int(n), int(n) + 1))
      if want is None:
        want = {k: np.zeros_like(v) for k, v in out.items()}
      for k in want:
        want[k][n] = out[k][n]
    self.eng.obs.fill_(0x5A)
    self.eng.step(a, active=None if active is None else act)
    got = self.eng.outputs_host()
    _parity.compare(self.t, self.ora, self.eng, want, got, what=self.what)
    np.testing.assert_array_equal(self.eng.task_sets().cpu().numpy(), self.ora.task_sets(), err_msg='task_sets ' + self.what)
    self.held = want
    self.t += 1
    return want, got

  def close(self):
    self.eng.close()


def against_the_oracles(make_engine, monkeypatch, which, gpu, seed=0, steps=STEPS):
  """STEPS steps of a mixed batch on its render path, every one through the bar; the conditions on what the run saw."""
  scene, env, expect = build_scene(which, gpu)
  r = Runner(make_engine, monkeypatch, scene, which, env, expect)
  rng = np.random.default_rng(seed + 100)
  for t in range(steps):
    r.step(r.sample(rng, r.ora.state() if t else None))
  r.ora.assert_saw_everything(which)
  assert r.eng.entry_task_sets().tolist() == r.pool.task_set.tolist()
  r.close()


def with_setter(make_engine, monkeypatch, gpu):
  """A live sprite setter on a handle with task sets: the override arrays join the flags the handle already owns."""
  scene = mix_s5(14 if gpu else 5, 5, seed=1)
  r = Runner(make_engine, monkeypatch, scene, 'with_setter')
  rng = np.random.default_rng(5)
  for t in range(3):
    r.step(r.sample(rng, r.ora.state() if t else None))
  for e in range(0, r.N, 2):
    r.ora.set_sprite_attr(e, 1, _abi.ATTR_SCALE, 0.3)
    r.eng.set_sprite_attr(e, 1, _abi.ATTR_SCALE, 0.3)
  assert r.eng.render().cpu().numpy().tobytes() == r.ora.render().tobytes()
  for t in range(STEPS - 3):
    r.step(r.sample(rng, r.ora.state()))
  r.ora.assert_saw_everything('with_setter')
  r.close()


def with_mask(make_engine, monkeypatch, gpu):
  """Masked steps: an environment that takes no part stays in its episode, and in its set."""
  scene = mix_s5(14 if gpu else 5, 5, seed=3)
  r = Runner(make_engine, monkeypatch, scene, 'with_mask')
  rng = np.random.default_rng(9)
  m = np.random.default_rng(10).random((2 * STEPS, r.N)) < 0.6
  m[0] = True
  for t in range(2 * STEPS):
    a = r.sample(rng, r.ora.state() if t else None)
    a[~m[t]] = np.nan
    r.step(a, active=m[t])
  r.ora.assert_saw_everything('with_mask')
  r.close()


def null_steps_reuse_records(make_engine, monkeypatch, gpu):
  """Null-action steps: nothing moves, so every step that is no reset takes the reward of its set's task from the record --
  swb_task_stats says so -- and the rewards still match the oracles', timeouts per set included."""
  scene = mix_s5(14 if gpu else 5, 5, seed=1)
  r = Runner(make_engine, monkeypatch, scene, 'null_steps', stats=True)
  a = null_actions(r.cfg)
  firsts = 0
  steps = 30
  for _ in range(steps):
    want, _ = r.step(a)
    firsts += int((want['step_type'] == _abi.STEP_FIRST).sum())
  reused, evaluated = r.eng.task_stats()
  # a FIRST evaluates and leaves the record; every other step of a run in which nothing moves reuses it
  assert reused + evaluated == steps * r.N
  assert evaluated == firsts, (reused, evaluated, firsts)
  assert reused > 0 and (r.ora.last_by_timeout).all()
  r.close()


def one_set_equals_no_sets(make_engine, monkeypatch, gpu):
  """A handle with one set equal to its config against a handle without sets, engine against engine: every output byte."""
  n_envs = 14 if gpu else 5
  for name, aa in (('cluster_s5', 5), ('sorting_s4', 5), ('goal_s5', 1)):
    cfg, pool, sample = workloads.build(name, n_envs, EPISODES_PER_ENV, 0, aa)
    cfg.max_episode_length = 7
    plain = new_engine(make_engine, cfg, None, pool)
    pool_s = copy.deepcopy(pool)
    pool_s.task_set = np.zeros(pool.n_entries, np.uint8)
    # (the handle's own task fields are unused on a handle with sets: garbage there must not matter)
    cfg_s = copy_cfg(cfg)
    cfg_s.max_episode_length, cfg_s.is_meta = 3, 0
    one = new_engine(make_engine, cfg_s, [lowering.task_set_of_config(cfg)], pool_s)
    rng = np.random.default_rng(3)
    for t in range(20):
      a = sample(rng)
      outs = []
      for eng in (plain, one):
        eng.obs.fill_(0x5A)
        eng.step(a)
        outs.append((eng.outputs_host(), eng.state()))
      for i in (0, 1):
        for k, v in outs[0][i].items():
          assert v.tobytes() == outs[1][i][k].tobytes(), (name, k, t)
    assert (one.task_sets().cpu().numpy() == 0).all()
    plain.close()
    one.close()


def reassignment(make_engine, monkeypatch, gpu, emu_error):
  """Entries change their set in the middle of episodes while nothing moves: swb_evaluate and the next step follow the new set
  at once (the task records of the old one are stale), checked against an oracle of the new set's configuration put into the
  same positions with set_positions."""
  from oracle import oracle
  n_envs = 14 if gpu else 5
  cfg, sets, pool, sample = same_scene('cluster_s5', n_envs, 5, seed=2, lengths=(9, 5, 12), goal_distance=0.05, relax=dict(threshold=50.))
  monkeypatch.setenv('SWB_LIST_STATS', '1')
  eng = new_engine(make_engine, cfg, sets, pool)
  model = Mixed(cfg, sets, pool)
  a0 = null_actions(cfg)
  for t in range(3):                                  # FIRST and two steps in which nothing moves: the records are in use
    want = model.step(a0)
    eng.step(a0)
    _parity.compare(t, model, eng, want, eng.outputs_host(), what='reassignment')
  assert eng.task_stats()[0] == 2 * n_envs
  with np.testing.assert_raises_regex(emu_error, 'names set 3'):
    eng.set_entry_task_sets(np.full(pool.n_entries, 3))
  assert eng.entry_task_sets().tolist() == pool.task_set.tolist()
  st = eng.state()
  for g_new in (1, 0):
    eng.set_entry_task_sets(np.full(pool.n_entries, g_new))
    assert (eng.task_sets().cpu().numpy() == g_new).all()
    # the oracle of the new set: every entry of the mixed pool, labelled for that set, brought to the same episode and step
    c, pl = split(cfg, sets, pool, set_of_entry=np.full(pool.n_entries, g_new))[g_new]
    assert pl.n_entries == pool.n_entries
    ora = oracle.Engine(c, pl)
    for t in range(3):
      out = ora.step(a0)
      assert (out['step_type'] != _abi.STEP_LAST).all(), 'the scene must not end under the new task before the comparison'
    ora.set_positions(st['x'], st['y'])
    np.testing.assert_array_equal(eng.evaluate().cpu().numpy(), ora.evaluate(), err_msg='evaluate under set %d' % g_new)
    reused = eng.task_stats()[0]
    probe = eng.save_state()                           # (the step below is taken twice, once per new set)
    a = sample(np.random.default_rng(11), st)
    want = ora.step(a)
    eng.step(a)
    assert eng.task_stats()[0] == reused, 'a record of the old set was reused'
    _parity.compare(3, ora, eng, want, eng.outputs_host(), what='reassignment to set %d' % g_new)
    eng.load_state(probe)
  eng.close()


def snapshots(make_engine, monkeypatch, gpu):
  """A snapshot saved in a mixed batch and loaded into other environments, which then continue as the source does -- in the
  source's set."""
  scene = mix_s5(14 if gpu else 6, 5, seed=1, assignment='per_env')
  r = Runner(make_engine, monkeypatch, scene, 'snapshots')
  rng = np.random.default_rng(5)
  for t in range(8):
    r.step(r.sample(rng, r.ora.state() if t else None))
  N = r.N
  src = np.arange(N)
  src[N // 2:] = np.arange(N - N // 2)                 # the upper half continues as the lower half does
  snap = r.eng.save_state()
  r.eng.load_state(snap, src.astype(np.int32))
  sets_now = r.eng.task_sets().cpu().numpy()
  assert sets_now.tolist() == r.ora.task_sets()[src].tolist() and len(set(sets_now[N // 2:].tolist())) > 1
  for t in range(14):
    a = r.sample(rng, r.ora.state())
    a = a[src]                                          # a copy takes its source's action
    want = r.ora.step(a)
    r.eng.step(a)
    got, st = r.eng.outputs_host(), r.eng.state()
    for k in ('step_type', 'success', 'obs'):
      assert got[k].tobytes() == want[k][src].tobytes(), (k, t)
    assert got['discount'].view(np.uint32).tolist() == want['discount'][src].view(np.uint32).tolist(), t
    _parity.assert_rewards_equal(got['reward'], want['reward'][src], 'snapshots t=%d' % t)
    ost = r.ora.state()
    for k in ('x', 'y', 'n_sprites', 'step_count', 'reset_next', 'episode', 'pool_entry'):
      assert st[k].tobytes() == ost[k][src].tobytes(), (k, t)
    assert not got['error'].any()
  r.close()


def fork(make_engine, monkeypatch, gpu):
  """The engine-level fork(2): a second engine with the same sets, the pool copied device to device (entry sets included),
  the states loaded: the copies continue bit-equal to their sources."""
  import torch
  scene = mix_s5(12 if gpu else 4, 5, seed=1)
  r = Runner(make_engine, monkeypatch, scene, 'fork')
  rng = np.random.default_rng(5)
  for t in range(7):
    r.step(r.sample(rng, r.ora.state() if t else None))
  N, M = r.N, 2
  cfg2 = copy_cfg(r.cfg)
  cfg2.n_envs = N * M
  child = make_engine(cfg2, None)
  child.set_task_sets(r.sets)
  child.copy_pool_from(r.eng, np.repeat(r.pool.pool_base, M), np.repeat(r.pool.pool_len, M))
  assert child.entry_task_sets().tolist() == r.pool.task_set.tolist()
  child.load_state(r.eng.save_state(), torch.arange(N * M) // M)
  for t in range(16):
    a = r.sample(rng, r.ora.state())
    _, got = r.step(a)
    child.obs.fill_(0x5A)
    child.step(np.repeat(a, M, axis=0))
    got2, st, st2 = child.outputs_host(), r.eng.state(), child.state()
    for k, v in got.items():
      assert got2[k].tobytes() == np.repeat(v, M, axis=0).tobytes(), (k, t)
    for k in ('x', 'y', 'n_sprites', 'step_count', 'reset_next', 'episode', 'pool_entry'):
      assert st2[k].tobytes() == np.repeat(st[k], M, axis=0).tobytes(), (k, t)
    assert child.task_sets().cpu().numpy().tolist() == np.repeat(r.ora.task_sets(), M).tolist()
  child.close()
  r.close()


def refusals(make_engine, monkeypatch, emu_error):
  import torch
  cfg, sets, pool, sample = mix_s5(4, 5)
  # after a pool has been installed
  eng = make_engine(cfg, pool_without_sets(pool))
  with np.testing.assert_raises_regex(emu_error, 'a pool has been installed'):
    eng.set_task_sets(sets)
  for call in (lambda: eng.task_sets(), lambda: eng.entry_task_sets(), lambda: eng.set_entry_task_sets(pool.task_set)):
    with np.testing.assert_raises_regex(emu_error, 'no task sets'):
      call()
  eng.close()
  # a sub-task range outside cfg.tasks, a second table
  eng = make_engine(cfg, None)
  for first, n in ((5, 2), (-1, 1), (0, 0), (6, 1)):
    bad = [lowering.task_set_of_config(cfg)]
    bad[0].first_task, bad[0].n_tasks, bad[0].is_meta = first, n, 1
    with np.testing.assert_raises_regex(emu_error, 'outside the 6 of the handle'):
      eng.set_task_sets(bad)
  with np.testing.assert_raises_regex(emu_error, r'outside \[1, 8\]'):
    eng._check(eng.lib.swb_set_task_sets(eng._h, 9, (_abi.SwbTaskSet * 9)()))
  eng.set_task_sets(sets)
  with np.testing.assert_raises_regex(emu_error, 'already'):
    eng.set_task_sets(sets)
  with np.testing.assert_raises_regex(emu_error, 'swb_set_pool has not been called'):
    eng.entry_task_sets()
  # an entry set >= n_sets changes nothing
  eng.set_pool(pool)
  bad = pool.task_set.copy()
  bad[-1] = 3
  with np.testing.assert_raises_regex(emu_error, 'entry %d names set 3' % (pool.n_entries - 1)):
    eng.set_entry_task_sets(bad)
  assert eng.entry_task_sets().tolist() == pool.task_set.tolist()
  # every rollout call
  eng.step(sample(np.random.default_rng(0)))
  actions = torch.zeros((2, cfg.n_envs, 3, 4), dtype=torch.float64)
  for call in (lambda: eng.rollout(actions), lambda: eng.rollout(actions, keep_steps=True),
               lambda: eng.rollout_sampled(_abi.SAMPLE_UNIFORM, 1, 3, 2), lambda: eng.rollout_guided(1, 3, 2,
                   motion_mean=torch.full((2, cfg.n_envs, 2), 0.5, dtype=torch.float64),
                   motion_std=torch.full((2, cfg.n_envs, 2), 0.1, dtype=torch.float64)),
               lambda: eng._check(eng.lib.swb_rollout_frames(eng._h, 3, None, C.c_void_p(eng.obs.data_ptr()), None, eng._stream())),
               lambda: eng._check(eng.lib.swb_rollout_step_frames(eng._h, 3, 0, None, C.c_void_p(eng.obs.data_ptr()), None, eng._stream()))):
    with np.testing.assert_raises_regex(emu_error, 'rollouts under task sets are not supported'):
      call()
  # swb_copy_pool across handles with different set tables
  other_sets = [_abi.SwbTaskSet.from_buffer_copy(bytes(s)) for s in sets]
  other_sets[1].max_episode_length += 1
  for table in (other_sets, None, sets[:2]):
    dst = make_engine(cfg, None)
    if table is not None:
      dst.set_task_sets(table)
    with np.testing.assert_raises_regex(emu_error, 'task sets differ'):
      dst.copy_pool_from(eng, pool.pool_base, pool.pool_len)
    dst.close()
  eng.close()


def pool_without_sets(pool):
  p = copy.deepcopy(pool)
  p.task_set = None
  return p
