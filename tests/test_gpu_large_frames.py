"""GPU: the large-frame render path (canvases wider than 640 px, images wider than 256 columns) against the CPU oracle.

Bar of tests/test_gpu_parity.py: state, rewards, step types, discounts and success bit-exact, frames +-0.  Geometries
beyond the tuned kernels take the large-frame path by themselves; SWB_LARGE_FRAMES=1 (read at swb_create) sends the
existing stress workloads there too.
"""
import numpy as np
import pytest

from spriteworld_amd import workloads
from tests import _parity
from tests import _setter_cases

pytestmark = pytest.mark.gpu


def _engine(cfg, pool):
  from spriteworld_amd import engine
  return engine.Engine(cfg, pool)


def _run(name, n_envs, steps, aa, seed=0):
  _parity.run(_engine, name, n_envs, steps, aa, seed=seed, expect={'large_frames': 1})


@pytest.mark.parametrize('geom,aa,n_envs,steps', [('256x256', 10, 6, 4), ('256x256', 5, 16, 6), ('160x160', 5, 32, 6),
                                                  ('200x120', 5, 32, 6), ('320x320', 2, 32, 6), ('512x512', 1, 32, 6)])
def test_large_frame_geometries(geom, aa, n_envs, steps):
  _run('geom_' + geom, n_envs, steps, aa)


@pytest.mark.parametrize('seed', range(6))
def test_large_frames_forced_randomised_configurations(monkeypatch, seed):
  monkeypatch.setenv('SWB_LARGE_FRAMES', '1')
  _run('fuzz_%d' % seed, 64, 8, 5, seed=seed)


@pytest.mark.parametrize('name,n_envs,steps,aa', [('tiny_s6', 128, 8, 5), ('tiny_s6', 128, 6, 1), ('wide_s4', 64, 8, 5),
                                                   ('ragged_s16', 96, 8, 5), ('embodied_s12', 48, 6, 5), ('goal_s5', 128, 24, 5),
                                                   ('cluster_s5', 128, 10, 1)])
def test_large_frames_forced_stress_workloads(monkeypatch, name, n_envs, steps, aa):
  monkeypatch.setenv('SWB_LARGE_FRAMES', '1')
  _run(name, n_envs, steps, aa)


@pytest.mark.parametrize('n_vertices', [33, 64])
def test_large_frames_forced_shapes_of_33_to_64_edges(monkeypatch, n_vertices):
  from spriteworld_amd import shapes
  from tests import _util
  monkeypatch.setenv('SWB_LARGE_FRAMES', '1')
  with _util.swapped_shape('circle', shapes.polygon(n_vertices)):
    _run('cluster_s5', 64, 6, 5)


def test_large_frames_forced_sprites_out_of_frame(monkeypatch):
  """f64_drag: no clipping to the frame, sprites leave it (and the episode ends)."""
  monkeypatch.setenv('SWB_LARGE_FRAMES', '1')
  _run('f64_drag', 64, 12, 3)


def test_large_frames_forced_tasks_that_filter_on_position(monkeypatch):
  from oracle import oracle
  from spriteworld_amd import engine, lowering
  from tests import _position_cases as pc
  monkeypatch.setenv('SWB_LARGE_FRAMES', '1')
  ns = pc.namespace_of_mirrors()
  name = pc.CASES[0]
  task, aspace, rends, keep, max_len = pc.environment_parts(ns, name)
  n_envs = 32
  episodes = pc.episodes_of(ns, name, True, n_episodes=3 * n_envs)
  cfg = lowering.lower_config(task, aspace, rends, keep, max_len, n_envs, pc.N_SPRITES, pos_is_f32=True)
  pool = lowering.lower_episodes(episodes, task, rends, max_sprites=pc.N_SPRITES).assign_round_robin(n_envs, 3)
  ora, eng = oracle.Engine(cfg, pool), engine.Engine(cfg, pool)
  assert eng.variant()['large_frames'] == 1
  rng = np.random.default_rng(11)
  for t in range(10):
    a = rng.uniform(0.0, 1.0, size=(n_envs, 4))
    want = ora.step(a)
    eng.step(a)
    _parity.compare(t, ora, eng, want, eng.outputs_host())
  eng.close()


def test_large_frames_sprite_setters(monkeypatch):
  monkeypatch.setenv('SWB_LARGE_FRAMES', '1')
  _setter_cases.run_parity(_engine, 'goal_s5', 32, 5, 5, expect={'large_frames': 1}, render_every=1)


def test_large_frame_setters_on_a_large_canvas():
  _setter_cases.run_parity(_engine, 'geom_160x160', 8, 4, 5, expect={'large_frames': 1}, render_every=1)


def test_large_frames_render_equals_the_step_frame_and_trim_is_a_no_op():
  from spriteworld_amd import engine
  cfg, pool, sample = workloads.build('geom_256x256', 16, episodes_per_env=2, seed=4, anti_aliasing=5)
  eng = engine.Engine(cfg, pool)
  rng = np.random.default_rng(9)
  for _ in range(5):           # (Engine.step trims after its third rendering step)
    eng.step(sample(rng))
  frame = eng.outputs_host()['obs'].copy()
  eng.obs.fill_(0x33)
  np.testing.assert_array_equal(eng.render().cpu().numpy(), frame)
  assert eng.trim() == 0
  info = eng.variant()
  assert info['large_frames'] == 1 and info['run_list_bytes'] == 0 and 'swb_lf_raster_kernel' in info['kernel']
  eng.close()


def test_large_frames_chunked(monkeypatch):
  """A scratch budget of three environments' horizontal pass: 20 environments in 7 chunks, every one rendered."""
  monkeypatch.setenv('SWB_LF_SCRATCH_BYTES', str(3 * 800 * 160 * 3))
  _run('geom_160x160', 20, 4, 5)


def test_batched_environment_with_the_demo_renderer():
  """A reference-style config with the reference demo's renderer (256 x 256 at anti_aliasing 10, a 2560 px canvas) and
  device-side resets: every frame equals the oracle's rendering of the state the environment reports."""
  from oracle import oracle
  from spriteworld_amd import action_spaces, environment, renderers, sprite_generators, tasks
  from spriteworld_amd import factor_distributions as distribs
  factors = distribs.Product([
      distribs.Continuous('x', 0.1, 0.9), distribs.Continuous('y', 0.1, 0.9),
      distribs.Discrete('shape', ['triangle', 'square', 'circle', 'star_5']), distribs.Discrete('scale', [0.13, 0.2]),
      distribs.Continuous('angle', 0, 360, dtype='int32'),
      distribs.Continuous('c0', 0., 1.), distribs.Continuous('c1', 0.3, 1.), distribs.Continuous('c2', 0.5, 1.)])
  env = environment.BatchedEnvironment(
      task=tasks.FindGoalPosition(terminate_distance=0.075), action_space=action_spaces.SelectMove(scale=0.5),
      renderers={'image': renderers.PILRenderer(image_size=(256, 256), anti_aliasing=10, color_to_rgb=renderers.hsv_to_rgb)},
      init_sprites=sprite_generators.generate_sprites(factors, num_sprites=4), max_episode_length=6, num_envs=8,
      episodes_per_env=4, seed=3, device_reset=True)
  assert env.engine.variant()['large_frames'] == 1
  rng = np.random.default_rng(5)
  ts = env.reset()
  for t in range(8):
    if t:
      ts = env.step(rng.uniform(0.0, 1.0, size=(8, 4)))
    frames = ts.observation['image'].cpu().numpy()
    st, pool = env.state(), env.engine.get_pool()
    for i in range(8):
      e, n = int(st['pool_entry'][i]), int(st['n_sprites'][i])
      want = oracle.render_sprites(env._cfg, st['x'][i, :n], st['y'][i, :n], pool.shape[e, :n], pool.scale[e, :n],
                                   pool.cos_a[e, :n], pool.sin_a[e, :n], pool.rgb[e, :n, :3])
      np.testing.assert_array_equal(frames[i], want, err_msg='env %d t=%d' % (i, t))
