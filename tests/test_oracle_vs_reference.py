"""Pins the oracle against the UNMODIFIED reference imported from /root/reference (build
container only; skipped where the reference tree is absent, e.g. on the GPU box)."""
import importlib

import numpy as np
import pytest

from oracle import ref_harness
from tests import _parity
from tests import _reference_cases
from tests._reference_cases import CONFIGS, fresh_episodes

pytestmark = pytest.mark.skipif(not ref_harness.reference_available(),
                                reason='reference tree not present')


class _OracleAsEngine(object):
  """The oracle behind the four members tests/_reference_cases.side_by_side drives an engine through."""

  def __init__(self, cfg, pool):
    from oracle import oracle
    self._ora = oracle.Engine(cfg, pool)
    self.state = self._ora.state

  def step(self, actions):
    self._out = self._ora.step(actions)

  def outputs_host(self):
    return self._out

  def close(self):
    pass


@pytest.mark.parametrize('module,mode', CONFIGS)
def test_oracle_equals_reference_environment(module, mode):
  _reference_cases.side_by_side(_OracleAsEngine, module, mode, seed=21, n_eps=30, n_steps=250)


def test_float64_sprites_and_motion_cost():
  """Test-style sprites built from Python floats (float64 positions) and a non-zero motion cost."""
  ref_harness.load_reference()
  from spriteworld import action_spaces, environment, renderers, sprite, tasks
  from oracle import oracle
  from spriteworld_amd import lowering
  rng = np.random.RandomState(5)

  def gen():
    return [sprite.Sprite(x=float(rng.uniform(0.1, 0.9)), y=float(rng.uniform(0.1, 0.9)),
                          shape=str(rng.choice(['star_5', 'spoke_4', 'hexagon', 'triangle'])),
                          angle=int(rng.randint(0, 360)), scale=float(rng.choice([0.1, 0.2, 0.35])),
                          c0=int(rng.randint(0, 256)), c1=int(rng.randint(0, 256)), c2=int(rng.randint(0, 256)),
                          x_vel=float(rng.uniform(-0.02, 0.02)), y_vel=float(rng.uniform(-0.02, 0.02)))
            for _ in range(4)]

  episodes = [gen() for _ in range(12)]
  for aspace in (action_spaces.SelectMove(scale=0.3, motion_cost=0.7),
                 action_spaces.DragAndDrop(scale=0.5, motion_cost=1.3)):
    task = tasks.FindGoalPosition(goal_position=(0.3, 0.6), terminate_distance=0.1, terminate_bonus=5.,
                                  weights_dimensions=(1, 3), raw_reward_multiplier=7)
    rends = {'image': renderers.PILRenderer(image_size=(32, 32), anti_aliasing=3, bg_color=(10, 200, 30))}
    cfg = lowering.lower_config(task, aspace, rends, False, 15, 1, 4,
                                pos_is_f32=(lowering.position_dtype(episodes) == np.float32))
    assert cfg.pos_is_f32 == 0
    pool = lowering.lower_episodes(episodes, task, rends, max_sprites=4).assign_round_robin(1)
    eng = oracle.Engine(cfg, pool)
    it = fresh_episodes(episodes)
    env = environment.Environment(task=task, action_space=aspace, renderers=rends,
                                  init_sprites=lambda: next(it), keep_in_frame=False, max_episode_length=15)
    arng = np.random.RandomState(9)
    for t in range(150):
      a = arng.uniform(0, 1, 4)
      ts = env.step(a)
      out = eng.step(a[None])
      assert int(ts.step_type) == int(out['step_type'][0]), t
      r = np.nan if ts.reward is None else float(ts.reward)
      assert (np.isnan(r) and np.isnan(out['reward'][0])) or _parity.bits(r) == _parity.bits(out['reward'][0]), (t, r, out['reward'][0])
      assert np.array_equal(ts.observation['image'], out['obs'][0]), t


def test_far_and_huge_sprites():
  """Sprites of scale up to 20 at positions in [-20, 20] (canvas coordinates of thousands of pixels on a 96-pixel canvas),
  keep_in_frame=False: the frames, step types and rewards of the unmodified reference, and no flag from the oracle."""
  ref_harness.load_reference()
  from spriteworld import action_spaces, environment, renderers, sprite, tasks
  from oracle import oracle
  from spriteworld_amd import lowering
  rng = np.random.RandomState(23)

  def gen():
    def xy():
      return float(rng.uniform(-0.5, 1.5) if rng.uniform() < 0.4 else rng.uniform(-20., 20.))
    return [sprite.Sprite(x=xy(), y=xy(), shape=str(rng.choice(['star_5', 'spoke_4', 'hexagon', 'triangle', 'square', 'circle'])),
                          angle=int(rng.randint(0, 360)), scale=float(np.exp(rng.uniform(np.log(0.05), np.log(20.)))),
                          c0=int(rng.randint(0, 256)), c1=int(rng.randint(0, 256)), c2=int(rng.randint(0, 256)),
                          x_vel=float(rng.uniform(-0.5, 0.5)), y_vel=float(rng.uniform(-0.5, 0.5)))
            for _ in range(4)]

  episodes = [gen() for _ in range(60)]
  task = tasks.FindGoalPosition(goal_position=(0.3, 0.6), terminate_distance=0.1, terminate_bonus=5.,
                                weights_dimensions=(1, 3), raw_reward_multiplier=7)
  aspace = action_spaces.DragAndDrop(scale=0.5, motion_cost=1.3)
  rends = {'image': renderers.PILRenderer(image_size=(32, 32), anti_aliasing=3, bg_color=(10, 200, 30))}
  cfg = lowering.lower_config(task, aspace, rends, False, 15, 1, 4, pos_is_f32=False)
  assert cfg.keep_in_frame == 0
  pool = lowering.lower_episodes(episodes, task, rends, max_sprites=4).assign_round_robin(1)
  eng = oracle.Engine(cfg, pool)
  it = fresh_episodes(episodes)
  env = environment.Environment(task=task, action_space=aspace, renderers=rends,
                                init_sprites=lambda: next(it), keep_in_frame=False, max_episode_length=15)
  arng = np.random.RandomState(9)
  bg = np.array([10, 200, 30], np.uint8)
  partly = fully = 0
  for t in range(110):                # (a sprite outside the frame ends the episode: nearly every second step starts one)
    a = arng.uniform(-0.5, 1.5, 4)
    ts = env.step(a)
    out = eng.step(a[None])
    assert int(ts.step_type) == int(out['step_type'][0]), t
    r = np.nan if ts.reward is None else float(ts.reward)
    assert (np.isnan(r) and np.isnan(out['reward'][0])) or _parity.bits(r) == _parity.bits(out['reward'][0]), (t, r, out['reward'][0])
    assert np.array_equal(ts.observation['image'], out['obs'][0]), t
    assert out['error'][0] == 0, t
    is_bg = (out['obs'][0] == bg).all(axis=-1)
    partly += int(is_bg.any() and not is_bg.all())
    fully += int(not is_bg.any())
  assert partly >= 10 and fully >= 5, (partly, fully)


@pytest.mark.parametrize('module,mode,motion_cost', [
    ('spriteworld.configs.cobra.goal_finding_more_distractors', 'train', 0.0),
    ('spriteworld.configs.cobra.clustering', 'train', 0.0),
    ('spriteworld.configs.cobra.clustering', 'test', 0.6),
    ('spriteworld.configs.cobra.sorting', 'train', 0.3),
    ('spriteworld.configs.cobra.exploration', 'train', 1.1),
])
def test_float32_actions_match_reference(module, mode, motion_cost):
  """float32 action arrays (the dtype action_spec() declares): numpy keeps float32 arithmetic."""
  ref_harness.load_reference()
  from spriteworld import action_spaces, environment
  from spriteworld import renderers as ref_renderers
  from oracle import oracle
  from spriteworld_amd import lowering
  seed, n_eps, n_steps = 33, 20, 200
  np.random.seed(seed)
  config = importlib.import_module(module).get_config(mode)
  config['action_space'] = action_spaces.SelectMove(scale=0.25, motion_cost=motion_cost)
  episodes = [config['init_sprites']() for _ in range(n_eps)]
  task, aspace, rends = config['task'], config['action_space'], config['renderers']
  S = max(len(e) for e in episodes)
  cfg = lowering.lower_config(task, aspace, rends, True, config['max_episode_length'], 1, S,
                              pos_is_f32=(lowering.position_dtype(episodes) == np.float32),
                              action_dtype=np.float32)
  assert cfg.action_is_f32 == 1
  pool = lowering.lower_episodes(episodes, task, rends, max_sprites=S).assign_round_robin(1)
  eng = oracle.Engine(cfg, pool)
  it = fresh_episodes(episodes)
  config = dict(config, init_sprites=lambda: next(it))
  config['renderers'] = dict(rends, success=ref_renderers.Success())
  env = environment.Environment(**config)
  rng = np.random.RandomState(seed + 1)
  for t in range(n_steps):
    a = rng.uniform(0, 1, 4).astype(np.float32)
    ts = env.step(a)
    out = eng.step(a[None])
    assert int(ts.step_type) == int(out['step_type'][0]), t
    r = np.nan if ts.reward is None else float(ts.reward)
    assert (np.isnan(r) and np.isnan(out['reward'][0])) or _parity.bits(r) == _parity.bits(out['reward'][0]), (t, r, out['reward'][0])
    assert np.array_equal(ts.observation['image'], out['obs'][0]), t
    pos = np.array([s.position for s in env._sprites], dtype=np.float64).reshape(-1, 2)
    st = eng.state()
    n = st['n_sprites'][0]
    assert np.array_equal(pos[:, 0], st['x'][0, :n]) and np.array_equal(pos[:, 1], st['y'][0, :n]), t


@pytest.mark.parametrize('space', ['select', 'embodied'])
def test_ragged_episodes_from_empty_to_sixteen_sprites(space):
  """Episodes of 0, 1, ... 16 sprites (the engine's maximum), some without any target: empty scenes,
  an Embodied agent that is alone, NaN rewards when no sprite passes the filter (tasks.py:140-142)."""
  ref_harness.load_reference()
  from spriteworld import action_spaces, environment, renderers, sprite, tasks
  from spriteworld import factor_distributions as distribs
  from oracle import oracle
  from spriteworld_amd import lowering
  rng = np.random.RandomState(17)

  def gen(n):
    return [sprite.Sprite(x=np.float32(rng.uniform(0.05, 0.95)), y=np.float32(rng.uniform(0.05, 0.95)),
                          shape=str(rng.choice(['square', 'triangle', 'circle', 'star_4'])),
                          scale=float(rng.choice([0.08, 0.15])), c0=np.float32(rng.uniform(0, 1)),
                          c1=np.float32(0.8), c2=np.float32(1.0)) for _ in range(n)]

  counts = [0, 1, 16, 0, 3, 2, 16, 1, 7, 0, 12, 5]
  episodes = [gen(n) for n in counts]
  task = tasks.FindGoalPosition(filter_distrib=distribs.Continuous('c0', 0., 0.3), terminate_distance=0.2)
  aspace = action_spaces.SelectMove(scale=0.4) if space == 'select' else action_spaces.Embodied(step_size=0.1)
  rends = {'image': renderers.PILRenderer(image_size=(64, 64), anti_aliasing=5, color_to_rgb=renderers.color_maps.hsv_to_rgb),
           'success': renderers.Success()}
  if space == 'embodied':       # Embodied needs a body: the reference indexes sprites[-1] (action_spaces.py:195)
    episodes = [e for e in episodes if e]
  cfg = lowering.lower_config(task, aspace, rends, True, 6, 1, 16, pos_is_f32=True)
  pool = lowering.lower_episodes(episodes, task, rends, max_sprites=16).assign_round_robin(1)
  eng = oracle.Engine(cfg, pool)
  it = fresh_episodes(episodes)
  env = environment.Environment(task=task, action_space=aspace, renderers=rends, init_sprites=lambda: next(it),
                                max_episode_length=6)
  arng = np.random.RandomState(3)
  for t in range(90):
    if space == 'select':
      a = arng.uniform(0, 1, 4)
      ts = env.step(a)
    else:
      a = np.array([arng.randint(0, 2), arng.randint(0, 4)])
      ts = env.step([int(a[0]), int(a[1])])
    out = eng.step(a[None])
    assert int(ts.step_type) == int(out['step_type'][0]), t
    r = np.nan if ts.reward is None else float(ts.reward)
    assert (np.isnan(r) and np.isnan(out['reward'][0])) or _parity.bits(r) == _parity.bits(out['reward'][0]), (t, r, out['reward'][0])
    assert bool(ts.observation['success']) == bool(out['success'][0]), t
    st = eng.state()
    pos = np.array([sp.position for sp in env._sprites], dtype=np.float64).reshape(-1, 2)
    n = st['n_sprites'][0]
    assert n == len(pos)
    assert np.array_equal(pos[:, 0], st['x'][0, :n]) and np.array_equal(pos[:, 1], st['y'][0, :n]), t
    assert np.array_equal(ts.observation['image'], out['obs'][0]), t


@pytest.mark.parametrize('seed', range(20))
def test_randomised_reference_configurations(seed):
  """Seeded random environments built from the reference's own classes (non-square images, any
  anti-aliasing, all shapes, rotations, float32 / float64 sprites, velocities, every task and action
  space, with and without keep_in_frame) against the oracle, step for step."""
  ref_harness.load_reference()
  from spriteworld import action_spaces, environment, renderers, sprite, tasks
  from spriteworld import constants
  from spriteworld import factor_distributions as distribs
  from oracle import oracle
  from spriteworld_amd import lowering
  rng = np.random.RandomState(1000 + seed)
  w, h = (int(4 * rng.randint(4, 30)) for _ in range(2))
  aa = int(rng.choice([1, 2, 3, 5]))
  S = int(rng.randint(1, 9))
  shapes_ = list(rng.choice(sorted(constants.SHAPES), size=int(rng.randint(1, 5)), replace=False))
  f32 = bool(rng.randint(0, 2))
  hsv = bool(rng.randint(0, 2))
  keep = bool(rng.randint(0, 2))
  vel = bool(rng.randint(0, 2))

  def num(lo, hi):
    v = rng.uniform(lo, hi)
    return np.float32(v) if f32 else float(v)

  def gen(n):
    out = []
    for _ in range(n):
      color = (num(0, 1), num(0.3, 1), num(0.5, 1)) if hsv else tuple(int(c) for c in rng.randint(0, 256, 3))
      out.append(sprite.Sprite(x=num(-0.05, 1.05) if not keep else num(0, 1), y=num(0, 1),
                               shape=str(rng.choice(shapes_)), angle=int(rng.randint(0, 360)) if rng.randint(0, 2) else 0,
                               scale=float(rng.choice([0.03, 0.08, 0.13, 0.25, 0.5])),
                               c0=color[0], c1=color[1], c2=color[2],
                               x_vel=float(rng.uniform(-0.02, 0.02)) if vel else 0.0,
                               y_vel=float(rng.uniform(-0.02, 0.02)) if vel else 0.0))
    return out

  kind = int(rng.randint(0, 3)) if S >= 4 else 0
  if kind == 0:
    key = 'c0'
    thr = 0.5 if hsv else 128
    filt = distribs.Continuous(key, 0, thr) if rng.randint(0, 2) else None
    task = tasks.FindGoalPosition(filter_distrib=filt, goal_position=(rng.uniform(0.2, 0.8), rng.uniform(0.2, 0.8)),
                                  terminate_distance=float(rng.uniform(0.05, 0.4)), terminate_bonus=float(rng.randint(0, 3)),
                                  sparse_reward=bool(rng.randint(0, 2)), raw_reward_multiplier=float(rng.randint(1, 60)))
  elif kind == 1:
    thr = 0.5 if hsv else 128
    top = 1.0 if hsv else 256
    task = tasks.Clustering([distribs.Continuous('c0', 0, thr), distribs.Continuous('c0', thr, top)],
                            termination_threshold=float(rng.uniform(1.0, 3.0)), terminate_bonus=float(rng.randint(0, 2)),
                            sparse_reward=bool(rng.randint(0, 2)), reward_range=float(rng.randint(1, 12)))
  else:
    thr = 0.5 if hsv else 128
    top = 1.0 if hsv else 256
    subs = [tasks.FindGoalPosition(filter_distrib=distribs.Continuous('c0', 0, thr), goal_position=(0.25, 0.75), terminate_distance=0.3),
            tasks.FindGoalPosition(filter_distrib=distribs.Continuous('c0', thr, top), goal_position=(0.75, 0.25), terminate_distance=0.3)]
    task = tasks.MetaAggregated(subs, reward_aggregator=str(rng.choice(['sum', 'max', 'min', 'mean'])),
                                termination_criterion=str(rng.choice(['all', 'any'])), terminate_bonus=float(rng.randint(0, 2)))
  which = int(rng.randint(0, 3))
  aspace = [action_spaces.SelectMove(scale=0.4, motion_cost=float(rng.choice([0.0, 0.7]))),
            action_spaces.DragAndDrop(scale=0.5, motion_cost=float(rng.choice([0.0, 1.3]))),
            action_spaces.Embodied(step_size=0.1, motion_cost=float(rng.choice([0.0, 0.4])))][which]
  rends = {'image': renderers.PILRenderer(image_size=(w, h), anti_aliasing=aa,
                                          bg_color=tuple(int(c) for c in rng.randint(0, 256, 3)) if rng.randint(0, 2) else None,
                                          color_to_rgb=renderers.color_maps.hsv_to_rgb if hsv else None),
           'success': renderers.Success()}

  def valid(ep):     # Clustering needs every cluster populated and more sprites than clusters
    if kind != 1:
      return True
    thr_ = 0.5 if hsv else 128
    lo = sum(1 for sp in ep if sp.c0 < thr_)
    return 1 <= lo < len(ep) and len(ep) > 2
  episodes = []
  while len(episodes) < 8:
    ep = gen(S if kind else int(rng.randint(max(1, S // 2), S + 1)))
    if valid(ep):
      episodes.append(ep)
  max_len = int(rng.randint(3, 12))
  cfg = lowering.lower_config(task, aspace, rends, keep, max_len, 1, S,
                              pos_is_f32=(lowering.position_dtype(episodes) == np.float32))
  pool = lowering.lower_episodes(episodes, task, rends, max_sprites=S).assign_round_robin(1)
  eng = oracle.Engine(cfg, pool)
  it = fresh_episodes(episodes)
  env = environment.Environment(task=task, action_space=aspace, renderers=rends, init_sprites=lambda: next(it),
                                keep_in_frame=keep, max_episode_length=max_len)
  arng = np.random.RandomState(seed)
  for t in range(60):
    if which == 2:
      a = np.array([arng.randint(0, 2), arng.randint(0, 4)])
      try:
        ts = env.step([int(a[0]), int(a[1])])
      except ZeroDivisionError:
        assert eng.step(a[None])['error'][0] & 1
        return
    else:
      a = arng.uniform(0, 1, 4)
      try:
        ts = env.step(a)
      except ZeroDivisionError:
        assert eng.step(a[None])['error'][0] & 1
        return
    out = eng.step(a[None])
    assert not out['error'][0], t
    assert int(ts.step_type) == int(out['step_type'][0]), t
    r = np.nan if ts.reward is None else float(ts.reward)
    assert (np.isnan(r) and np.isnan(out['reward'][0])) or _parity.bits(r) == _parity.bits(out['reward'][0]), (t, r, out['reward'][0])
    assert bool(ts.observation['success']) == bool(out['success'][0]), t
    st = eng.state()
    pos = np.array([sp.position for sp in env._sprites], dtype=np.float64).reshape(-1, 2)
    n = st['n_sprites'][0]
    assert n == len(pos)
    assert np.array_equal(pos[:, 0], st['x'][0, :n]) and np.array_equal(pos[:, 1], st['y'][0, :n]), t
    assert np.array_equal(ts.observation['image'], out['obs'][0]), t


@pytest.mark.parametrize('f32', [True, False], ids=['f32pos', 'f64pos'])
@pytest.mark.parametrize('name', __import__('tests._position_cases', fromlist=['CASES']).CASES)
def test_tasks_that_filter_on_position_match_the_reference(name, f32):
  """Round 6: filters / cluster distributions keyed on x, y (the reference evaluates `contains(sprite.factors)` at EVERY step,
  tasks.py:134-137, 196-205).  The lowering tabulates each sprite's label over the cells the filter's interval bounds cut the
  plane into (with the reference's own contains()), the oracle looks the sprite's cell up every step: rewards, success, step
  types bit for bit against the unmodified reference while sprites are dragged across the cuts and clipped onto the frame
  (x = 0.0 / 1.0 exactly: the half-open bounds), float32 and float64 positions, Python-float and np.float64 bounds."""
  ref_harness.load_reference()
  from spriteworld import environment
  from spriteworld import renderers as ref_renderers
  from oracle import oracle
  from spriteworld_amd import _abi, lowering
  from tests import _position_cases as pc
  ns = pc.namespace_of_reference()
  task, aspace, rends, keep, max_len = pc.environment_parts(ns, name)
  episodes = pc.episodes_of(ns, name, f32)
  assert (lowering.position_dtype(episodes) == np.float32) == f32
  cfg = lowering.lower_config(task, aspace, rends, keep, max_len, 1, pc.N_SPRITES, pos_is_f32=f32)
  assert sum(cfg.tasks[t].n_xcuts + cfg.tasks[t].n_ycuts for t in range(cfg.n_tasks)) > 0
  pool = lowering.lower_episodes(episodes, task, rends, max_sprites=pc.N_SPRITES).assign_round_robin(1)
  assert pool.cell_label is not None
  eng = oracle.Engine(cfg, pool)
  it = fresh_episodes(episodes)
  env = environment.Environment(task=task, action_space=aspace, renderers=dict(rends, success=ref_renderers.Success()),
                                init_sprites=lambda: next(it), keep_in_frame=keep, max_episode_length=max_len)
  rng = np.random.RandomState(77)
  changed = 0
  prev = None
  for t in range(300):
    a = rng.uniform(0, 1, 4)
    if t % 3 == 0:            # click ON a sprite, so that something moves most steps
      s = env._sprites[rng.randint(len(env._sprites))]
      a[:2] = np.asarray(s.position, dtype=np.float64)
    try:
      ts = env.step(a)
    except (ValueError, ZeroDivisionError) as e:      # Davies-Bouldin with one cluster left / a zero score: the oracle flags it
      out = eng.step(a[None])
      want = _abi.ENV_ERR_DB_LABELS if isinstance(e, ValueError) else _abi.ENV_ERR_DB_ZERO
      assert out['error'][0] & want, (t, e)
      break
    out = eng.step(a[None])
    assert int(ts.step_type) == int(out['step_type'][0]), t
    r = np.nan if ts.reward is None else float(ts.reward)
    assert (np.isnan(r) and np.isnan(out['reward'][0])) or _parity.bits(r) == _parity.bits(out['reward'][0]), (t, r, out['reward'][0])
    assert bool(ts.observation['success']) == bool(out['success'][0]), t
    assert np.array_equal(ts.observation['image'], out['obs'][0]), t
    # how often membership really changed inside an episode (the case must exercise what it is for)
    subs = lowering.subtasks_of(task)
    lab = tuple(lowering._label_of(sub, s) for sub in subs for s in env._sprites)    # pylint: disable=protected-access
    if prev is not None and int(ts.step_type) == 1 and lab != prev:
      changed += 1
    prev = lab
  else:
    assert changed >= 5, changed
