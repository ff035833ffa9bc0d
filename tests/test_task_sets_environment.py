"""`BatchedEnvironment.from_configs`: one batch whose episodes are played under the tasks of several
reference-style configs, against one oracle per config (tests/_task_sets_cases.Mixed) -- on the emulated engine (CPU) and,
marked `gpu`, on the device.  The episodes are drawn on the host, so the oracles play the very pool the engine holds."""
import numpy as np
import pytest

from spriteworld_amd import lowering
from tests import _parity
from tests import _task_sets_cases as cases

BACKENDS = [pytest.param('emu'), pytest.param('gpu', marks=pytest.mark.gpu)]
LENGTHS = (5, 8, 11)


def _configs(keep_in_frame=True, scale=0.25):
  from spriteworld_amd import action_spaces, renderers, sprite_generators, tasks
  from spriteworld_amd import factor_distributions as distribs
  common = [distribs.Continuous('x', 0.1, 0.9), distribs.Continuous('y', 0.1, 0.9),
            distribs.Discrete('shape', ['square', 'triangle', 'circle']), distribs.Discrete('scale', [0.2]),
            distribs.Continuous('c1', 0.3, 1.), distribs.Continuous('c2', 0.9, 1.)]
  red, blue = distribs.Continuous('c0', 0., 0.4), distribs.Continuous('c0', 0.5, 0.9)
  gen = lambda *counts: sprite_generators.chain_generators(*[
      sprite_generators.generate_sprites(distribs.Product(common + [c0]), num_sprites=k) for c0, k in zip((red, blue), counts)])
  rend = lambda: {'image': renderers.PILRenderer(image_size=(64, 64), anti_aliasing=5, color_to_rgb=renderers.color_maps.hsv_to_rgb)}
  aspace = lambda: action_spaces.SelectMove(scale=scale)
  goal = tasks.FindGoalPosition(filter_distrib=red, terminate_distance=0.3)
  cluster = tasks.Clustering([red, blue], termination_threshold=1.2, terminate_bonus=0., reward_range=10.)
  sort = tasks.MetaAggregated([tasks.FindGoalPosition(filter_distrib=d, goal_position=g, terminate_distance=0.3, raw_reward_multiplier=20.)
                               for d, g in ((red, (0.25, 0.25)), (blue, (0.75, 0.75)))], reward_aggregator='sum',
                              termination_criterion='any')
  return [dict(task=t, action_space=aspace(), renderers=rend(), init_sprites=gen(*counts), max_episode_length=m,
               keep_in_frame=keep_in_frame)
          for t, counts, m in ((goal, (2, 2), LENGTHS[0]), (cluster, (2, 3), LENGTHS[1]), (sort, (1, 2), LENGTHS[2]))]


def _environment(monkeypatch, backend, n_envs, **kwargs):
  from spriteworld_amd import environment
  if backend == 'emu':
    from tests import _emu_engine
    monkeypatch.setattr(environment._engine, 'Engine', _emu_engine.EmuTorchEngine)
  np.random.seed(11)
  env = environment.BatchedEnvironment.from_configs(_configs(), n_envs, episodes_per_env=4, check_errors=1, **kwargs)
  assert env.engine.pool is not None and env.num_task_sets == 3
  return env


def _model(env):
  return cases.Mixed(env._cfg, env.engine.task_set_table, env.engine.pool)


@pytest.mark.parametrize('backend', BACKENDS)
def test_steps_resets_masks_and_the_set_the_agent_sees(monkeypatch, backend):
  n = 5 if backend == 'emu' else 14
  env = _environment(monkeypatch, backend, n)
  cfg, pool = env._cfg, env.engine.pool
  assert cfg.n_tasks == 4 and cfg.max_sprites == 5
  assert [(s.first_task, s.n_tasks, s.is_meta, s.max_episode_length) for s in env.engine.task_set_table] == [
      (0, 1, 0, LENGTHS[0]), (1, 1, 0, LENGTHS[1]), (2, 2, 1, LENGTHS[2])]
  which = pool.task_set.reshape(n, 4)
  assert which.tolist() == [[(e + k) % 3 for k in range(4)] for e in range(n)]
  # an entry is drawn from its own config's generator, and labelled for the sub-tasks of EVERY set (a reassignment finds them):
  # the goal task's filter and the first sorting sub-task's are the clustering's cluster 0, the second's its cluster 1
  assert pool.n_sprites.reshape(n, 4).tolist() == np.asarray([4, 5, 3])[which].tolist()
  live = np.arange(5)[None, :] < pool.n_sprites[:, None]
  for row, cluster in ((0, 0), (2, 0), (3, 1)):
    assert (pool.label[:, row][live] == (pool.label[:, 1][live] == cluster)).all(), row
  assert set(pool.label[:, 1][live].tolist()) == {0, 1}
  model = _model(env)
  e = env.engine
  null = env.null_actions().cpu().numpy()
  held = model.step(null)
  ts = env.reset()
  assert ts.step_type is e.step_type and ts.observation['image'] is e.obs
  _parity.compare(0, model, e, held, e.outputs_host(), what='from_configs')
  sample = cases._sampler(cfg)
  rng = np.random.default_rng(3)
  for t in range(1, 50):
    a = sample(rng, model.state())
    active = rng.random(n) < 0.7 if t % 3 == 0 else None
    for i in (range(n) if active is None else np.flatnonzero(active)):
      out = model.step(a, env_range=(int(i), int(i) + 1))
      for k in held:
        held[k][i] = out[k][i]
    env.step(a if active is None else np.where(active[:, None], a, np.nan), active=active)
    _parity.compare(t, model, e, held, e.outputs_host(), what='from_configs')
    assert env.task_sets().cpu().numpy().tolist() == model.task_sets().tolist()
  model.assert_saw_everything('from_configs')
  env.close()


@pytest.mark.parametrize('backend', BACKENDS)
def test_fork_snapshots_run_episodes_and_the_rollout_refusals(monkeypatch, backend):
  n = 4 if backend == 'emu' else 12
  env = _environment(monkeypatch, backend, n)
  from spriteworld_amd import _lib
  if backend == 'emu':
    from tests import _emu_engine
    error = _emu_engine.EmuError
  else:
    error = _lib.SwbError
  sample = cases._sampler(env._cfg)
  rng = np.random.default_rng(5)
  env.reset()
  for _ in range(6):
    env.step(sample(rng, env.state()))
  child = env.fork(2)
  assert child.num_task_sets == 3 and child.engine.entry_task_sets().tolist() == env.engine.entry_task_sets().tolist()
  snap = env.save_state()
  taken, seen = [], []
  for t in range(12):
    a = sample(rng, env.state())
    env.step(a)
    child.step(np.repeat(a, 2, axis=0))
    got, got2 = env.engine.outputs_host(), child.engine.outputs_host()
    for k, v in got.items():
      assert got2[k].tobytes() == np.repeat(v, 2, axis=0).tobytes(), (k, t)
    sets_now = env.task_sets().cpu().numpy().copy()
    assert child.task_sets().cpu().numpy().tolist() == np.repeat(sets_now, 2).tolist()
    taken.append(a)
    seen.append((got, sets_now))
  assert len(set(np.concatenate([s for _, s in seen]).tolist())) == 3
  env.load_state(snap)                                 # back to where the fork was taken: the same steps give the same again
  for t, a in enumerate(taken):
    env.step(a)
    got = env.engine.outputs_host()
    for k, v in seen[t][0].items():
      assert got[k].tobytes() == v.tobytes(), (k, t)
    assert env.task_sets().cpu().numpy().tolist() == seen[t][1].tolist()
  for call in (lambda: env.rollout(np.zeros((n, 3, 2, 4))), lambda: env.rollout_random(3, 2), lambda: env.rollout_guided(3, 2),
               lambda: env.plan_cem(4, 2, iterations=1)):
    with pytest.raises(error, match='rollouts under task sets are not supported'):
      call()
  played = env.state()['episode']
  stats = env.run_episodes(lambda ts, active: env.null_actions(), episodes_per_env=3)
  assert stats.episodes.cpu().numpy().tolist() == [3] * n
  # every episode ends by the time limit of ITS set at the latest
  which = env.engine.pool.task_set.reshape(n, 4)
  longest = sum(np.asarray(LENGTHS)[which[np.arange(n), (played + k) % 4]] for k in range(3))
  length = stats.length.cpu().numpy()
  assert (length <= longest).all() and (length >= 3).all() and (length > min(LENGTHS)).any()
  child.close()
  env.close()


def test_what_from_configs_refuses(monkeypatch):
  from spriteworld_amd import action_spaces, environment
  from tests import _emu_engine
  monkeypatch.setattr(environment._engine, 'Engine', _emu_engine.EmuTorchEngine)
  make = environment.BatchedEnvironment.from_configs
  np.random.seed(1)
  for field, change in (('action_space', lambda c: c.update(action_space=action_spaces.SelectMove(scale=0.5))),
                        ('action_space', lambda c: c.update(action_space=action_spaces.DragAndDrop(scale=0.25))),
                        ('keep_in_frame', lambda c: c.update(keep_in_frame=False)),
                        ('renderers', lambda c: c.update(renderers=dict(c['renderers'], success=None)))):
    configs = _configs()
    change(configs[1])
    with pytest.raises(lowering.LoweringError, match='config 1 differs from config 0 in ' + field):
      make(configs, 4, episodes_per_env=4)
  with pytest.raises(lowering.LoweringError, match='sub-tasks'):
    make(_configs() + _configs() + _configs()[:1], 4, episodes_per_env=4)
  with pytest.raises(lowering.LoweringError, match='between 1 and 8'):
    make([_configs()[0]] * 9, 4, episodes_per_env=4)
  with pytest.raises(lowering.LoweringError, match=r'int array \[4, 4\]'):
    make(_configs(), 4, task_set_of_entry=np.zeros((4, 3), np.int64), episodes_per_env=4)
  env = make(_configs(), 4, task_set_of_entry='per_env', episodes_per_env=4)
  assert env.engine.pool.task_set.reshape(4, 4).tolist() == [[0] * 4, [1] * 4, [2] * 4, [0] * 4]
  env.reset()
  assert env.task_sets().tolist() == [0, 1, 2, 0]
  explicit = np.asarray([[2, 2, 0, 0]] * 4)
  env.set_task_set_of_entry(explicit)
  assert env.task_sets().tolist() == [2] * 4 and env.engine.entry_task_sets().tolist() == explicit.reshape(-1).tolist()
  env.refill_pool()                                    # a fresh pool, drawn and labelled under the new assignment
  assert env.engine.entry_task_sets().tolist() == explicit.reshape(-1).tolist()
  assert env.engine.pool.n_sprites.reshape(4, 4).tolist() == [[3, 3, 4, 4]] * 4
  env.close()
  plain = environment.BatchedEnvironment(**dict(_configs()[0], num_envs=2, episodes_per_env=2, device_reset=False))
  assert plain.num_task_sets == 0
  with pytest.raises(lowering.LoweringError, match='no task sets'):
    plain.set_task_set_of_entry('cycle')
  plain.close()


def _shared_configs():
  """Three tasks over ONE generator object: what the device samplers take."""
  configs = _configs()
  for c in configs:
    c['init_sprites'] = configs[1]['init_sprites']
  return configs


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('device_reset', ['auto', 'tree'])
def test_shared_init_sprites_are_sampled_on_the_device_and_refreshed(monkeypatch, backend, device_reset):
  from spriteworld_amd import environment
  if backend == 'emu':
    from tests import _emu_engine
    monkeypatch.setattr(environment._engine, 'Engine', _emu_engine.EmuTorchEngine)
  n = 5 if backend == 'emu' else 14
  env = environment.BatchedEnvironment.from_configs(_shared_configs(), n, episodes_per_env=4, check_errors=1, seed=5,
                                                    device_reset=device_reset, refresh_every=0)
  e = env.engine
  assert env._sampler is not None and e.pool is None       # ('tree' keeps the plain sampler where the generator lowers to it)
  assert env.num_task_sets == 3 and env._cfg.n_tasks == 4
  which = e.entry_task_sets()
  assert which.reshape(n, 4).tolist() == [[(i + k) % 3 for k in range(4)] for i in range(n)]
  pool = e.get_pool()                                  # what the device drew, labelled per sprite for all four sub-tasks
  assert pool.task_set.tolist() == which.tolist() and (pool.n_sprites == 5).all()
  for row, cluster in ((0, 0), (2, 0), (3, 1)):
    assert (pool.label[:, row] == (pool.label[:, 1] == cluster)).all(), row
  assert sorted(set(pool.label[:, 1].reshape(-1).tolist())) == [0, 1]
  model = cases.Mixed(env._cfg, e.task_set_table, pool)
  held = model.step(env.null_actions().cpu().numpy())
  env.reset()
  _parity.compare(0, model, e, held, e.outputs_host(), what='device sampled')
  sample = cases._sampler(env._cfg)
  rng = np.random.default_rng(3)
  for t in range(1, 40):
    a = sample(rng, model.state())
    want = model.step(a)
    env.step(a)
    _parity.compare(t, model, e, want, e.outputs_host(), what='device sampled')
    assert env.task_sets().cpu().numpy().tolist() == model.task_sets().tolist()
  model.assert_saw_everything('device sampled')
  # a refresh redraws the idle entries and keeps every entry's set; the live episodes go on
  playing = e.state()['pool_entry']
  env.refresh_pool()
  assert e.entry_task_sets().tolist() == which.tolist()
  fresh = e.get_pool()
  idle = np.setdiff1d(np.arange(4 * n), playing)
  assert (fresh.x[idle] != pool.x[idle]).any() and (fresh.x[playing] == pool.x[playing]).all()
  env.step(sample(rng, model.state()))
  assert not e.outputs_host()['error'].any()
  env.close()


def test_device_reset_is_refused_for_different_generators_and_reassignment_is_safe(monkeypatch):
  from spriteworld_amd import environment
  from tests import _emu_engine
  monkeypatch.setattr(environment._engine, 'Engine', _emu_engine.EmuTorchEngine)
  np.random.seed(3)
  for device_reset in (True, 'tree'):
    with pytest.raises(lowering.LoweringError, match='share one init_sprites'):
      environment.BatchedEnvironment.from_configs(_configs(), 4, episodes_per_env=4, device_reset=device_reset)
  env = environment.BatchedEnvironment.from_configs(_configs(), 4, episodes_per_env=4)       # 'auto': drawn on the host
  assert env._sampler is None and env.engine.pool is not None
  # every entry to the clustering: the step after follows the oracle of that task on the very pool, labels included
  env.reset()
  env.set_task_set_of_entry(np.ones((4, 4), np.int64))
  pool = env.engine.get_pool()
  model = cases.Mixed(env._cfg, env.engine.task_set_table, pool)
  null = env.null_actions().cpu().numpy()
  model.step(null)
  a = cases._sampler(env._cfg)(np.random.default_rng(1), model.state())
  want = model.step(a)
  env.step(a)
  _parity.compare(1, model, env.engine, want, env.engine.outputs_host(), what='reassigned')
  assert np.isfinite(want['reward']).all() and (want['reward'] != 0).any()
  env.close()
