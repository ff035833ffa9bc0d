"""Device-side reset sampling (swb_sample_pool): lowering on CPU, bit-for-bit draws on the GPU.  The sampler configurations
and the bodies the emulated suite shares are in tests/_sampler_cases.py."""
import numpy as np
import pytest

from spriteworld_amd import _abi
from spriteworld_amd import action_spaces
from spriteworld_amd import device_sampler
from spriteworld_amd import factor_distributions as distribs
from spriteworld_amd import lowering
from spriteworld_amd import renderers as renderer_lib
from spriteworld_amd import shapes
from spriteworld_amd import sprite as sprite_lib
from spriteworld_amd import tasks

from tests import _sampler_cases as cases
from tests import _sampler_model
from tests._sampler_cases import CASES

def test_philox_known_answers():
  # Random123 kat_vectors, philox4x32-10
  assert _sampler_model.philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
  f = 0xffffffff
  assert _sampler_model.philox4x32_10((f, f, f, f), (f, f)) == (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)
  assert (_sampler_model.philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) ==
          (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))


@pytest.mark.parametrize('case', sorted(CASES))
def test_lowering_fills_the_spec(case):
  sampler, task, rend = CASES[case]()
  spec = sampler.lower(task, rend)
  assert spec.n_groups == len(sampler.groups)
  assert spec.deg_cos[90] == np.cos(np.radians(90)) and spec.deg_sin[270] == np.sin(np.radians(270))
  if case == 'sorting_like':
    assert spec.n_alternatives == 9 and spec.alternatives[0].n == 2 and sampler.max_sprites == 2
    assert [spec.groups[g].label[g] for g in range(5)] == [1] * 5 and spec.groups[0].label[1] == 0
  for g in range(spec.n_groups):
    assert spec.groups[g].factor('x').kind == _abi.FACTOR_UNIFORM_F32
    assert 1 <= spec.groups[g].n_shapes <= _abi.SWB_MAX_CANDIDATES
  if case == 'cobra_like':
    assert spec.color_map == 1 and spec.shuffle == _abi.SWB_MAX_GROUPS
    assert [spec.groups[g].label[0] for g in range(2)] == [1, 0]
    assert (spec.groups[1].count_min, spec.groups[1].count_max) == (1, 3)
    assert sampler.max_sprites == 5
  if case == 'mixed_types':
    assert spec.color_map == 0
    assert spec.groups[0].factor('angle').kind == _abi.FACTOR_UNIFORM_INT
    assert spec.groups[0].factor('c0').kind == _abi.FACTOR_UNIFORM_INT
    assert spec.groups[1].factor('angle').kind == _abi.FACTOR_DISCRETE and spec.groups[1].factor('angle').n == 4
    # Clustering labels: group a has c1 in cluster 0; group b has the default c1 = 0, also inside
    # Continuous('c1', 0, 128) -> first match wins (tasks.py:196-205)
    assert [spec.groups[g].label[0] for g in range(3)] == [0, 0, 0]


def test_setminus_lowers_to_holdout_boxes():
  sampler, task, rend = cases._holdouts()
  spec = sampler.lower(task, rend)
  grp = spec.groups[0]
  assert grp.n_holdouts == 2 and spec.groups[1].n_holdouts == 0
  assert grp.holdouts[0].redraw_mask == 0b11 and grp.holdouts[0].box_mask == 0b11
  assert (grp.holdouts[0].lo[0], grp.holdouts[0].hi[1]) == (0.5, 0.9)
  assert grp.holdouts[1].redraw_mask == 0b100 and (grp.holdouts[1].lo[2], grp.holdouts[1].hi[2]) == (0.08, 0.12)
  # the model never leaves a sprite inside a hold-out box
  label = lambda f: int(task._filter_distrib.contains(f))
  got = _sampler_model.sample_pool(spec, 400, 3, 99, rend['image']._color_to_rgb, [label], shapes.SHAPE_NAMES)
  tx, ty, ts = got['x'][:, :2], got['y'][:, :2], got['scale'][:, :2]
  assert not ((tx >= 0.5) & (ty >= 0.5)).any() and ((tx >= 0.5) | (ty >= 0.5)).any()
  assert not ((ts >= 0.08) & (ts < 0.12)).any() and (ts < 0.08).any() and (ts >= 0.12).any()
  assert ((got['x'][:, 2] >= 0.5) & (got['y'][:, 2] >= 0.5)).any()      # distractors are not held out


def test_partial_shuffle_keeps_the_body_on_top():
  sampler, task, rend = cases._embodied_like()
  spec = sampler.lower(task, rend)
  assert spec.shuffle == 2 and spec.n_groups == 3
  label = lambda f: int(task._filter_distrib.contains(f))
  got = _sampler_model.sample_pool(spec, 600, 4, 17, rend['image']._color_to_rgb, [label], shapes.SHAPE_NAMES)
  n = got['n_sprites']
  top = got['scale'][np.arange(600), n - 1]
  assert (top == 0.07).all()                                         # body always last (front-most)
  first_is_target = got['label'][n == 3, 0, 0].mean()                # 1 target among 2 shuffled objects
  assert abs(first_is_target - 0.5) < 0.1
  np.random.seed(0)
  for _ in range(30):
    sprites = sampler()
    assert sprites[-1].scale == 0.07 and 2 <= len(sprites) <= 4


def test_from_generator_reads_generator_closures():
  from spriteworld_amd import sprite_generators as gens
  a = distribs.Product([distribs.Continuous('x', 0., 1.), distribs.Continuous('y', 0., 1.)])
  b = distribs.Product([distribs.Continuous('x', 0., 1.), distribs.Continuous('y', 0., 1.), distribs.Discrete('scale', [0.2])])
  s = device_sampler.from_generator(gens.shuffle(gens.chain_generators(
      gens.generate_sprites(a, num_sprites=2), gens.generate_sprites(b, num_sprites=lambda: np.random.randint(1, 4)))))
  assert [(lo, hi) for _, lo, hi, _ in s.groups] == [(2, 2), (1, 3)] and s.shuffle == _abi.SWB_MAX_GROUPS
  s = device_sampler.from_generator(gens.chain_generators(
      gens.shuffle(gens.chain_generators(gens.generate_sprites(a, 1), gens.generate_sprites(b, 2))),
      gens.generate_sprites(b, 1)))
  assert len(s.groups) == 3 and s.shuffle == 2
  assert device_sampler.from_generator(gens.generate_sprites(a, 3)).shuffle == 0
  ga, gb = gens.generate_sprites(a, 1), gens.generate_sprites(b, 1)
  s = device_sampler.from_generator(gens.shuffle(gens.sample_generator(
      [gens.chain_generators(ga, gb), gens.chain_generators(gb, ga), ga])))
  assert len(s.groups) == 2 and s.alternatives == [[0, 1], [1, 0], [0]] and s.max_sprites == 2
  with pytest.raises(lowering.LoweringError):
    device_sampler.from_generator(gens.sample_generator([ga, gb], p=[0.3, 0.7]))
  with pytest.raises(lowering.LoweringError):
    device_sampler.from_generator(lambda: [])
  with pytest.raises(lowering.LoweringError):
    device_sampler.from_generator(gens.generate_sprites(a, num_sprites=lambda: 3))
  with pytest.raises(lowering.LoweringError):     # shuffled part not leading
    device_sampler.from_generator(gens.chain_generators(gens.generate_sprites(a, 1), gens.shuffle(gens.generate_sprites(b, 2))))


def test_every_reference_config_lowers_to_a_device_sampler():
  """from_generator + lower on the reference's own config dicts (both modes): the label probing, the
  SetMinus hold-outs, integer colours / angles and the partially shuffled embodied generator."""
  from oracle import ref_harness
  if not ref_harness.reference_available():
    pytest.skip('reference tree not present')
  import importlib
  ref_harness.load_reference()
  expect_groups = {'goal_finding_new_position': 2, 'goal_finding_new_shape': 1, 'goal_finding_more_distractors': 2,
                   'goal_finding_more_targets': 2, 'clustering': 2, 'sorting': None, 'exploration': 1,
                   'goal_finding_embodied': 3}
  np.random.seed(0)
  for pkg in ('cobra', 'examples'):
    for name, n_groups in expect_groups.items():
      try:
        mod = importlib.import_module('spriteworld.configs.%s.%s' % (pkg, name))
      except ImportError:
        continue
      for mode in ('train', 'test'):
        config = mod.get_config(mode)
        sampler = device_sampler.from_generator(config['init_sprites'])
        spec = sampler.lower(config['task'], config['renderers'])
        assert spec.n_groups == (n_groups or (5 if mode == 'train' else 2)), (name, mode)
        if name == 'goal_finding_embodied':
          assert spec.shuffle == 2
        if name == 'sorting':
          assert spec.n_alternatives == (9 if mode == 'train' else 0)
        if name == 'goal_finding_new_position' and mode == 'train':
          assert spec.groups[0].n_holdouts == 1
        # host episodes of the same generator fit the sampler's bounds
        for _ in range(5):
          assert len(config['init_sprites']()) <= sampler.max_sprites
  # examples/goal_finding_clustering mixes random counts, integer colours and a SetMinus scale
  mod = importlib.import_module('spriteworld.configs.examples.goal_finding_clustering')
  for mode in ('train', 'test'):
    config = mod.get_config(mode)
    sampler = device_sampler.from_generator(config['init_sprites'])
    spec = sampler.lower(config['task'], config['renderers'])
    assert spec.color_map == 0 and spec.n_groups >= 4


def test_host_call_draws_valid_sprites():
  sampler, _, _ = cases._mixed_types()
  np.random.seed(0)
  for _ in range(20):
    sprites = sampler()
    assert 3 <= len(sprites) <= 5
    assert all(isinstance(s, sprite_lib.Sprite) for s in sprites)


def test_value_dependent_labels_are_refused():
  wide = distribs.Product([distribs.Continuous('x', 0., 1.), distribs.Continuous('y', 0., 1.),
                           distribs.Continuous('c0', 0., 1.)])
  sampler = device_sampler.DeviceSampler([(wide, 3)])
  task = tasks.FindGoalPosition(filter_distrib=distribs.Continuous('c0', 0., 0.4))
  with pytest.raises(lowering.LoweringError, match='depends on the sampled factors'):
    sampler.lower(task, {'image': renderer_lib.PILRenderer()})


def test_unsupported_distributions_are_refused():
  mix = distribs.Mixture([distribs.Continuous('x', 0., .5), distribs.Continuous('x', .5, 1.)])
  with pytest.raises(lowering.LoweringError, match='cannot be sampled on the device'):
    device_sampler.DeviceSampler([(distribs.Product([mix, distribs.Continuous('y', 0., 1.)]), 1)])
  f64 = distribs.Product([distribs.Continuous('x', 0., 1., dtype='float64'), distribs.Continuous('y', 0., 1.)])
  with pytest.raises(lowering.LoweringError):
    device_sampler.DeviceSampler([(f64, 1)]).lower(tasks.NoReward(), {'image': renderer_lib.PILRenderer()})


# ------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize('case', sorted(CASES))
def test_device_pool_matches_the_model_bit_for_bit(case):
  cases.pool_matches_the_model_case(case)


@pytest.mark.gpu
def test_shards_draw_the_episodes_of_the_whole_job():
  cases.shards_case()


@pytest.mark.gpu
def test_sampled_environment_steps_like_one_built_from_the_same_pool():
  """Stepping a device-sampled pool == stepping the same pool uploaded from the host (swb_set_pool)."""
  import torch
  from spriteworld_amd import engine as engine_lib
  env, sampler, task, rend = cases.make_env('cobra_like', num_envs=64, episodes_per_env=2)
  pool = env.engine.get_pool()
  twin = engine_lib.Engine(env._cfg, pool)
  g = torch.Generator(device='cpu').manual_seed(5)
  env.reset()
  twin.reset_all()
  twin.step(env.null_actions(), render=True)
  assert torch.equal(twin.obs, env.engine.obs)
  for _ in range(20):
    act = torch.rand((64, 4), generator=g, dtype=torch.float64)
    ts = env.step(act.cuda())
    twin.step(act.cuda())
    assert torch.equal(twin.obs, ts.observation['image'])
    np.testing.assert_array_equal(twin.reward.cpu().numpy(), env.engine.reward.cpu().numpy())   # NaN on FIRST
    assert torch.equal(twin.step_type, env.engine.step_type)
  env.check()
  env.close()
  twin.close()


@pytest.mark.gpu
def test_device_reset_option_reads_the_generator_closures():
  from spriteworld_amd import environment
  from tests import _surface_cases
  config = _surface_cases._cobra_like_config(n_targets=2, n_distractors=1)
  env = environment.BatchedEnvironment(num_envs=256, episodes_per_env=4, device_reset=True, **config)
  assert env._sampler is not None and env._sampler.max_sprites == 3
  pool = env.engine.get_pool()
  assert (pool.n_sprites == 3).all() and (pool.label.sum(axis=2) == 2).all()       # two targets per episode
  ts = env.reset()
  for _ in range(30):
    ts = env.step(env.sample_actions())
  env.check()
  env.close()
  single = environment.Environment(device_reset='auto', **config)
  ts = single.reset()
  assert ts.first() and ts.observation['image'].shape == (64, 64, 3)
  single.close()
  config['init_sprites'] = lambda: _surface_cases._cobra_like_config()['init_sprites']()
  with pytest.raises(lowering.LoweringError):
    environment.BatchedEnvironment(num_envs=4, device_reset=True, **config)
  env = environment.BatchedEnvironment(num_envs=4, device_reset='auto', **config)     # host fallback
  assert env._sampler is None
  env.close()


@pytest.mark.gpu
def test_refresh_pool_redraws_everything_but_the_live_entries():
  cases.refresh_case()


@pytest.mark.gpu
@pytest.mark.parametrize('refresh_every,early_ends', [(5, False), ('auto', True)])
def test_refresh_every_keeps_episodes_fresh(refresh_every, early_ends):
  """With refresh_every the same (env, pool slot) never serves the same episode twice.  refresh_every = 5 with episodes that
  always last their 5 steps (FIRST + max_episode_length = 4; the task cannot succeed): the pool is redrawn right after every
  LAST step.  'auto' (every 2 * (episodes_per_env - 1) = 2 steps) gives the guarantee whatever ends an episode early -- here a
  task that succeeds now and then.  (Until round 5 the first case ran with the succeeding task: a single early success within
  the 40 steps made an environment wrap to an entry not yet redrawn, and the test failed once in a while.)"""
  from spriteworld_amd import environment
  np.random.seed(11)
  sampler, task, rend = cases._cobra_like()
  if not early_ends:
    task = tasks.FindGoalPosition(filter_distrib=distribs.Continuous('c0', 0., 0.4), terminate_distance=1e-9)
  else:
    task = tasks.FindGoalPosition(filter_distrib=distribs.Continuous('c0', 0., 0.4), terminate_distance=0.45)
  env = environment.BatchedEnvironment(task=task, action_space=action_spaces.SelectMove(scale=0.25), renderers=rend,
                                       init_sprites=sampler, max_episode_length=4, num_envs=32, episodes_per_env=2,
                                       refresh_every=refresh_every)
  env.reset()
  seen = set()
  lasts = 0
  for _ in range(40):
    ts = env.step(env.sample_actions())
    first = (ts.step_type == 0).cpu().numpy()
    lasts += int((ts.step_type == 2).sum().item())
    if first.any():
      st = env.state()
      for e in np.flatnonzero(first):
        key = (int(e), tuple(np.round(st['x'][e], 6)))      # the episode's initial positions
        assert key not in seen
        seen.add(key)
  assert len(seen) > 32 * 4
  if early_ends:
    assert lasts > 32 * 40 // 5 + 16                          # episodes did end before their fifth step
  env.check()
  env.close()


@pytest.mark.gpu
def test_refill_draws_new_statistically_uniform_episodes():
  env, sampler, task, rend = cases.make_env('cobra_like', num_envs=2048, episodes_per_env=4)
  a = env.engine.get_pool()
  env.refill_pool()
  b = env.engine.get_pool()
  assert not np.array_equal(a.x, b.x)
  live = np.arange(a.x.shape[1])[None, :] < b.n_sprites[:, None]
  x = b.x[live]
  assert 0.1 <= x.min() and x.max() < 0.9 and abs(x.mean() - 0.5) < 0.01 and abs(x.std() - 0.8 / 12 ** 0.5) < 0.01
  counts = np.bincount(b.n_sprites, minlength=6)[3:6] / len(b.n_sprites)   # 2 targets + randint(1, 4)
  assert np.all(np.abs(counts - 1 / 3) < 0.03)
  # shuffle: a target (label 1) lands in every z slot about equally often among 3-sprite episodes
  three = b.n_sprites == 3
  first = b.label[three, 0, 0].mean()
  assert abs(first - 2 / 3) < 0.05
  shapes_used = np.bincount(b.shape[live], minlength=shapes.shape_index('circle') + 1)
  assert (shapes_used > 0).sum() == 3
  env.close()


# ------------------------------------------------------------- statistical parity with the reference
def test_model_matches_the_reference_generators_statistically():
  """The Philox draw scheme (restated in _sampler_model, bit-equal to the device) and the reference's
  own MT19937-driven generators produce the same distribution of episodes."""
  from oracle import ref_harness
  if not ref_harness.reference_available():
    pytest.skip('reference tree not present')
  from scipy import stats
  ref_harness.load_reference()
  from spriteworld import factor_distributions as rd
  from spriteworld import sprite_generators as rg
  from spriteworld import renderers as rr
  from spriteworld import tasks as rt
  common = [rd.Continuous('x', 0.1, 0.9), rd.Continuous('y', 0.1, 0.9),
            rd.Discrete('shape', ['square', 'triangle', 'circle']), rd.Discrete('scale', [0.13]),
            rd.Continuous('c1', 0.3, 1.), rd.Continuous('c2', 0.9, 1.)]
  target = rd.Product(common + [rd.Continuous('c0', 0., 0.4)])
  distractor = rd.Product(common + [rd.Continuous('c0', 0.5, 0.9)])
  task = rt.FindGoalPosition(filter_distrib=rd.Continuous('c0', 0., 0.4), terminate_distance=0.1)
  rend = {'image': rr.PILRenderer(image_size=(64, 64), anti_aliasing=5, color_to_rgb=rr.color_maps.hsv_to_rgb)}
  # the reference's classes lower unchanged (duck-typed)
  sampler = device_sampler.DeviceSampler([(target, 2), (distractor, (1, 4))], shuffle=True, seed=1)
  spec = sampler.lower(task, rend)
  P = 3000
  label_fn = lambda f: int(task._filter_distrib.contains(f))
  got = _sampler_model.sample_pool(spec, P, 5, sampler.next_seed(), rr.color_maps.hsv_to_rgb, [label_fn],
                                   shapes.SHAPE_NAMES)
  gen = rg.shuffle(rg.chain_generators(rg.generate_sprites(target, num_sprites=2),
                                       rg.generate_sprites(distractor, num_sprites=lambda: np.random.randint(1, 4))))
  np.random.seed(123)
  ref_eps = [gen() for _ in range(P)]
  ref_n = np.array([len(e) for e in ref_eps])
  assert stats.chisquare(np.bincount(got['n_sprites'], minlength=6)[3:], np.bincount(ref_n, minlength=6)[3:]).pvalue > 1e-3
  live = np.arange(5)[None, :] < got['n_sprites'][:, None]
  for key, col in (('x', got['x']), ('y', got['y']), ('c0', got['color'][..., 0]), ('c1', got['color'][..., 1])):
    ref_vals = np.array([float(s.factors[key]) for e in ref_eps for s in e])
    assert stats.ks_2samp(col[live], ref_vals).pvalue > 1e-3, key
  for ch in range(3):
    ref_rgb = np.array([rr.color_maps.hsv_to_rgb(s.color)[ch] for e in ref_eps for s in e], dtype=np.float64)
    assert stats.ks_2samp(got['rgb'][..., ch][live].astype(np.float64), ref_rgb).pvalue > 1e-3
  # z-order: P(back-most sprite is a target)
  ref_first = np.mean([e[0].c0 < 0.4 for e in ref_eps])
  assert abs(got['label'][:, 0, 0].mean() - ref_first) < 0.04
  ref_shapes = np.bincount([shapes.shape_index(s.shape) for e in ref_eps for s in e], minlength=len(shapes.SHAPE_NAMES))
  got_shapes = np.bincount(got['shape'][live], minlength=len(shapes.SHAPE_NAMES))
  nz = ref_shapes > 0
  assert (got_shapes > 0).tolist() == nz.tolist()
  assert stats.chisquare(got_shapes[nz] * (ref_shapes[nz].sum() / got_shapes[nz].sum()), ref_shapes[nz]).pvalue > 1e-3


def test_emulated_sampler_records_the_type_of_every_scale(monkeypatch):
  from spriteworld_amd import environment
  from tests import _emu_engine
  monkeypatch.setattr(environment._engine, 'Engine', _emu_engine.EmuTorchEngine)
  cases.recorded_scale_types_case()


@pytest.mark.gpu
def test_device_sampler_records_the_type_of_every_scale():
  cases.recorded_scale_types_case()
