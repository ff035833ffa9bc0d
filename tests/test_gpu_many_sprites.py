"""GPU: the many-sprite path (handles of 17 to 64 sprites: swb_ms_state_kernel, then the large-frame render kernels) against
the CPU oracle.  Bar of tests/test_gpu_parity.py: state, rewards, step types, discounts and success bit-exact, frames +-0.
SWB_MANY_SPRITES=1 (read at swb_create) sends workloads of up to 16 sprites down the same path."""
import numpy as np
import pytest

from spriteworld_amd import _abi
from spriteworld_amd import lowering
from spriteworld_amd import workloads
from tests import _many_sprites_cases as cases
from tests import _parity

pytestmark = pytest.mark.gpu


def _gpu(cfg, pool):
  from spriteworld_amd import engine
  return engine.Engine(cfg, pool)


@pytest.mark.parametrize('name,n_envs,steps,aa', [('ragged_s64', 64, 16, 5), ('ragged_s64', 48, 10, 1), ('ragged_s64_embodied', 48, 16, 5),
                                                   ('cluster_s40', 32, 10, 5), ('cluster_s40_f32a', 32, 8, 3), ('meta_s24_f64', 48, 16, 5)])
def test_gpu_many_sprite_workloads(name, n_envs, steps, aa):
  firsts, most = cases.run_parity(_gpu, name, n_envs, steps, aa)
  assert firsts >= n_envs and most > _abi.SWB_TUNED_SPRITES


@pytest.mark.parametrize('name,n_envs,steps,aa', [('ragged_s16', 32, 10, 5), ('embodied_s12', 16, 6, 5), ('f64_drag', 32, 8, 3),
                                                   ('fuzz_3', 16, 8, 5), ('fuzz_11', 16, 8, 5), ('fuzz_23', 16, 8, 5)])
def test_gpu_many_sprite_path_forced(monkeypatch, name, n_envs, steps, aa):
  monkeypatch.setenv('SWB_MANY_SPRITES', '1')
  cases.run_parity(_gpu, name, n_envs, steps, aa)


def _sub_pool(pool, envs):
  idx = np.concatenate([np.arange(pool.pool_base[e], pool.pool_base[e] + pool.pool_len[e]) for e in envs])
  sub = lowering.Pool(len(idx), pool.max_sprites, pool.n_tasks)
  for f in lowering.Pool.FIELDS + ('angle', 'color', 'attr_f32'):
    if f not in ('pool_base', 'pool_len'):
      setattr(sub, f, np.ascontiguousarray(getattr(pool, f)[idx]))
  sub.pool_base = np.ascontiguousarray(np.cumsum([0] + [int(pool.pool_len[e]) for e in envs[:-1]]), dtype=np.int32)
  sub.pool_len = np.ascontiguousarray(pool.pool_len[envs], dtype=np.int32)
  return sub


def test_gpu_ragged_s64_8192_environments():
  """8192 environments of 0 .. 64 sprites at anti_aliasing 5: a sample of 48 environments against the oracle stepping
  exactly those, every step."""
  from oracle import oracle
  from spriteworld_amd import engine
  N = 8192
  cfg, pool, sample = workloads.build('ragged_s64', N, episodes_per_env=2, seed=5, anti_aliasing=5)
  eng = engine.Engine(cfg, pool)
  assert eng.variant()['many_sprites'] == 1
  envs = np.sort(np.random.default_rng(1).choice(N, 48, replace=False))
  envs[0] = 1                                    # (an environment whose first episode has 64 sprites)
  envs = np.unique(envs)
  scfg, _, _ = workloads.build('ragged_s64', len(envs), episodes_per_env=2, seed=5, anti_aliasing=5)
  ora = oracle.Engine(scfg, _sub_pool(pool, envs))
  rng = np.random.default_rng(9)
  for t in range(8):
    a = sample(rng)
    eng.step(a)
    got = eng.outputs_host()
    want = ora.step(np.ascontiguousarray(a[envs]))
    st_g, st_o = eng.state(), ora.state()
    assert not got['error'].any()
    np.testing.assert_array_equal(got['obs'][envs], want['obs'], err_msg='frames t=%d' % t)
    np.testing.assert_array_equal(got['step_type'][envs], want['step_type'])
    np.testing.assert_array_equal(got['discount'][envs].view(np.uint32), want['discount'].view(np.uint32))
    np.testing.assert_array_equal(got['success'][envs], want['success'])
    gr, wr = got['reward'][envs], want['reward']
    assert np.array_equal(np.isnan(gr), np.isnan(wr))
    ok = ~np.isnan(wr)
    np.testing.assert_array_equal(_parity.bits(gr[ok]), _parity.bits(wr[ok]))
    np.testing.assert_array_equal(_parity.bits(st_g['x'][envs]), _parity.bits(st_o['x']))
    np.testing.assert_array_equal(_parity.bits(st_g['y'][envs]), _parity.bits(st_o['y']))
    np.testing.assert_array_equal(st_g['n_sprites'][envs], st_o['n_sprites'])
  assert st_g['n_sprites'].max() == 64
  eng.close()


def test_gpu_setters_on_sprites_beyond_sixteen():
  cases.setters_case(_gpu, n_envs=16)


def test_gpu_render_and_evaluate():
  cases.render_and_evaluate_case(_gpu, n_envs=16)


def test_gpu_batched_environment_of_32_sprites():
  """A BatchedEnvironment built from a reference-style generator of 32 sprites (this package's sprite_generators /
  factor_distributions), driven through reset() / step(): its time steps equal the oracle's on the pool it installed."""
  import torch
  from oracle import oracle
  from spriteworld_amd import action_spaces, environment, renderers, sprite_generators, tasks
  from spriteworld_amd import factor_distributions as distribs
  common = [distribs.Continuous('x', 0.1, 0.9), distribs.Continuous('y', 0.1, 0.9),
            distribs.Discrete('shape', ['square', 'triangle', 'circle']), distribs.Discrete('scale', [0.06]),
            distribs.Continuous('c1', 0.3, 1.), distribs.Continuous('c2', 0.9, 1.)]
  targets = distribs.Product(common + [distribs.Continuous('c0', 0., 0.4)])
  others = distribs.Product(common + [distribs.Continuous('c0', 0.5, 0.9)])
  gen = sprite_generators.shuffle(sprite_generators.chain_generators(sprite_generators.generate_sprites(targets, num_sprites=8),
                                                                     sprite_generators.generate_sprites(others, num_sprites=24)))
  task = tasks.FindGoalPosition(filter_distrib=distribs.Continuous('c0', 0., 0.4), terminate_distance=0.1)
  rend = {'image': renderers.PILRenderer(image_size=(64, 64), anti_aliasing=5, color_to_rgb=renderers.color_maps.hsv_to_rgb),
          'success': renderers.Success()}
  np.random.seed(3)
  env = environment.BatchedEnvironment(task=task, action_space=action_spaces.SelectMove(scale=0.25), renderers=rend,
                                       init_sprites=gen, max_episode_length=10, num_envs=64, episodes_per_env=4, refresh_every=0)
  assert env._max_sprites == 32
  assert env.engine.variant()['many_sprites'] == 1 and env.engine.variant()['state_kernel'] == 'swb_ms_state_kernel'
  ora = oracle.Engine(env.engine.cfg, env.engine.get_pool())
  ts = env.reset()
  want = ora.step(np.zeros((64, 4)))
  rng = np.random.default_rng(4)
  for t in range(12):
    np.testing.assert_array_equal(ts.step_type.cpu().numpy(), want['step_type'], err_msg='t=%d' % t)
    np.testing.assert_array_equal(ts.observation['image'].cpu().numpy(), want['obs'], err_msg='t=%d' % t)
    np.testing.assert_array_equal(ts.observation['success'].cpu().numpy(), want['success'].astype(bool))
    r, wr = ts.reward.cpu().numpy(), want['reward']
    assert np.array_equal(np.isnan(r), np.isnan(wr))
    ok = ~np.isnan(wr)
    np.testing.assert_array_equal(_parity.bits(r[ok]), _parity.bits(wr[ok]))
    a = rng.uniform(0, 1, size=(64, 4))
    ts = env.step(torch.as_tensor(a))
    want = ora.step(a)
  env.close()


def test_gpu_variant_names_the_many_sprite_kernels(monkeypatch):
  from spriteworld_amd import engine
  cfg, pool, _ = workloads.build('cluster_s40', 8, episodes_per_env=2)
  eng = engine.Engine(cfg, pool)
  v = eng.variant()
  assert v['many_sprites'] == 1 and v['large_frames'] == 1 and v['state_kernel'] == 'swb_ms_state_kernel'
  assert v['kernel'] == 'swb_lf_raster_kernel + swb_lf_vertical_kernel' and v['cover_kernel'] == 'none'
  eng.close()
  cfg, pool, _ = workloads.build('ragged_s16', 8, episodes_per_env=2)
  eng = engine.Engine(cfg, pool)
  assert eng.variant()['many_sprites'] == 0 and 'state_kernel' not in eng.variant()
  eng.close()
