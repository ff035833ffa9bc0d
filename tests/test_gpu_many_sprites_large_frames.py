"""GPU: the many-sprite state kernel (17 to 64 sprites) on large, wide and non-square frames; both paths at the limits the code
states (4096 canvas pixels in either direction, 1024 image columns, 64 sprites, the vertex budget of the raster kernel's LDS)
and one step past them; more than 65 535 environments on the large-frame path.  Against the CPU oracle, every step: state,
rewards, step types, discounts and success bit-exact, frames +-0 (tests/_parity.compare).

The oracle's time per frame, one thread of the build container's CPU, sizes environments x steps of every case (a case's oracle
work stays under 20 s there):

  canvas (image, anti_aliasing)      4 sprites   64 sprites
  1280 x 1280 (256 x 256, 5)          0.027 s     0.037 s
  2560 x 2560 (256 x 256, 10)         0.103 s     0.110 s
  4096 x 4096 (256 x 256, 16)         0.219 s     0.262 s
  4096 x 256  (1024 x 64, 4)          0.020 s     0.020 s
  256 x 4096  (64 x 1024, 4)          0.018 s     0.023 s
  1024 x 1024 (128 x 128, 8)          0.015 s     0.013 s
  1024 x 1024 (1024 x 1024, 1)        0.002 s     0.004 s
  1000 x 600, 800 x 800               0.010 s     0.009 s
  640 x 128, 512 x 512 (AA 1)       <= 0.003 s  <= 0.001 s

The module's oracle work adds up to about 110 s there (cross 70 s, limits 12 s, 65 600 environments 5 s of frames and 20 s of
drawing the pools, the rest 5 s)."""
import numpy as np
import pytest

from spriteworld_amd import lowering
from spriteworld_amd import workloads
from tests import _many_sprites_cases as cases
from tests import _parity

pytestmark = pytest.mark.gpu


def _gpu(cfg, pool):
  from spriteworld_amd import engine
  return engine.Engine(cfg, pool)


def _error():
  from spriteworld_amd import _lib
  return _lib.SwbError


# S, image (w, h), anti_aliasing, task, action space, float32 positions, environments, steps.  Below 64 environments the raster
# kernel takes blocks of 16 canvas rows, from 64 on blocks of 64.
CROSS = [(64, (256, 256), 5, 'goal', 'select', True, 64, 6),        # full sprite tables on a 1280 px canvas, 20 row blocks: 14 s
         (17, (256, 256), 10, 'goal', 'drag', True, 24, 6),         # the demo renderer just over the tuned sprite count: 16 s
         (40, (128, 128), 8, 'cluster', 'select', True, 96, 8),     # Clustering (13 clusters) away from 64 x 64: 12 s
         (24, (320, 64), 2, 'meta', 'select', False, 96, 8),        # > 256 columns, non-square, MetaAggregated f64 + velocities: 2 s
         (64, (512, 512), 1, 'goal', 'drag', True, 48, 8),          # the AA 1 store into obs, 64 sprites: 1 s
         (64, (200, 120), 5, 'goal', 'embodied', True, 64, 8),      # non-square, Embodied: 5 s
         (64, (320, 320), 2, 'goal', 'select', False, 4, 6)]        # a handful of environments


@pytest.mark.parametrize('S,size,aa,task,space,f32,n_envs,steps', CROSS)
def test_gpu_many_sprites_on_large_frames(S, size, aa, task, space, f32, n_envs, steps):
  got = cases.run_scene(_gpu, cases.scene(S, size, aa, n_envs, task=task, space=space, f32=f32, seed=S), steps)
  assert got['most'] == S


def test_gpu_many_sprites_on_large_frames_chunked(monkeypatch):
  """33 sprites at 160 x 160, anti_aliasing 5, a scratch budget of three environments' horizontal pass: 20 environments in 7
  chunks."""
  monkeypatch.setenv('SWB_LF_SCRATCH_BYTES', str(3 * 800 * 160 * 3))
  cases.run_scene(_gpu, cases.scene(33, (160, 160), 5, 20), 5)


def test_gpu_setters_beyond_sixteen_on_a_large_canvas():
  cases.setters_case(_gpu, steps=4, built=cases.scene(40, (160, 160), 5, 16, episodes_per_env=3, seed=1))


def test_gpu_render_and_evaluate_on_a_large_canvas():
  cases.render_and_evaluate_case(_gpu, built=cases.scene(40, (160, 160), 5, 16, task='cluster', max_len=30, seed=2))


# the accepted side of each limit: 4096 px wide, 4096 px tall, both (anti_aliasing 16: Lanczos windows of 97 taps), 1024 columns
LIMITS = [((1024, 64), 4, 4), ((64, 1024), 4, 4), ((256, 256), 16, 3), ((1024, 16), 1, 4), ((1024, 1024), 1, 4)]


@pytest.mark.parametrize('size,aa,n_envs', LIMITS)
def test_gpu_limits_with_64_sprites(size, aa, n_envs):
  """64 circles: 1920 polygon vertices, the largest scene of built-in shapes (104 KB of LDS at a 4096 px wide canvas)."""
  built = cases.scene(64, size, aa, n_envs, space='drag', max_len=1, shape_names=('circle',), ragged=False, seed=aa)
  cases.run_scene(_gpu, built, 3, want_most=64)


@pytest.mark.parametrize('size,aa,n_envs', LIMITS)
def test_gpu_limits_with_4_sprites(monkeypatch, size, aa, n_envs):
  """(SWB_LARGE_FRAMES=1: a canvas of 256 x 4096 with up to 16 sprites is otherwise the tuned kernels'.)"""
  monkeypatch.setenv('SWB_LARGE_FRAMES', '1')
  built = cases.scene(4, size, aa, n_envs, max_len=1, ragged=False, seed=aa, scales=(0.05, 0.3, 0.6))
  cases.run_scene(_gpu, built, 3, many=False, check_claims=False, want_most=4)


def test_gpu_refusals_one_step_past_each_limit():
  cases.refusals_case(_gpu, _error())


@pytest.mark.parametrize('size,aa,budget', [((64, 64), 5, 3844), ((1024, 16), 4, 3420)])
def test_gpu_vertex_budget_is_a_boundary(size, aa, budget):
  """(160 KiB - 4384 B of head - 4 waves x (canvas width + span mask + 1024 B of crossings)) / 40 B per vertex, in steps of 4
  vertices: at a 320 px and at a 4096 px canvas."""
  assert cases.vertex_budget_case(_gpu, _error(), size, aa) == budget


def _sub_pool(pool, envs):
  idx = np.concatenate([np.arange(pool.pool_base[e], pool.pool_base[e] + pool.pool_len[e]) for e in envs])
  sub = lowering.Pool(len(idx), pool.max_sprites, pool.n_tasks)
  for f in lowering.Pool.FIELDS + ('angle', 'color', 'attr_f32'):
    if f not in ('pool_base', 'pool_len'):
      setattr(sub, f, np.ascontiguousarray(getattr(pool, f)[idx]))
  sub.pool_base = np.ascontiguousarray(np.cumsum([0] + [int(pool.pool_len[e]) for e in envs[:-1]]), dtype=np.int32)
  sub.pool_len = np.ascontiguousarray(pool.pool_len[envs], dtype=np.int32)
  return sub


N_BIG = 65536 + 64
UNWRITTEN = 0xA5          # no byte of a background or of a sprite colour of these scenes (asserted)


def _big_batch(built, steps, many):
  """More environments than a grid dimension holds (65 535): lf_render renders them in two chunks.  Only a sample leaves the
  device -- environments 0, 65 534, 65 535 (the second chunk's first), 65 536, the last one and 91 drawn ones -- against the
  oracle stepping exactly those; every other frame is shown written by a reduction on the device."""
  import ctypes
  import torch
  from oracle import oracle
  from spriteworld_amd import _abi
  cfg, pool, sample = built
  N = cfg.n_envs
  assert N == N_BIG
  assert not (pool.rgb[:, :, :3] == UNWRITTEN).all(axis=2).any() and tuple(cfg.bg_rgb)[:3] != (UNWRITTEN,) * 3
  eng = _gpu(cfg, pool)
  v = eng.variant()
  assert v['large_frames'] == 1 and v['many_sprites'] == int(many)
  pick = np.unique(np.concatenate([[0, 65534, 65535, 65536, N - 1], np.random.default_rng(1).choice(N, 91, replace=False)]))
  scfg = _abi.SwbConfig.from_buffer_copy(bytes(cfg))
  scfg.n_envs = len(pick)
  ora = oracle.Engine(scfg, _sub_pool(pool, pick))
  idx = torch.as_tensor(pick, device=eng.device)
  rng = np.random.default_rng(9)
  for t in range(steps):
    a = sample(rng)
    eng.obs.fill_(UNWRITTEN)
    eng.step(a)
    want = ora.step(np.ascontiguousarray(a[pick]))
    assert int(eng.error.max().item()) == 0
    unwritten = (eng.obs.view(N, -1) == UNWRITTEN).all(dim=1)
    assert not bool(unwritten.any().item()), ('frames left unwritten', torch.nonzero(unwritten)[:8].flatten().tolist(), t)
    np.testing.assert_array_equal(eng.obs[idx].cpu().numpy(), want['obs'], err_msg='frames t=%d' % t)
    np.testing.assert_array_equal(eng.step_type[idx].cpu().numpy(), want['step_type'])
    np.testing.assert_array_equal(eng.success[idx].cpu().numpy(), want['success'])
    np.testing.assert_array_equal(eng.discount[idx].cpu().numpy().view(np.uint32), want['discount'].view(np.uint32))
    gr, wr = eng.reward[idx].cpu().numpy(), want['reward']
    assert np.array_equal(np.isnan(gr), np.isnan(wr))
    ok = ~np.isnan(wr)
    np.testing.assert_array_equal(_parity.bits(gr[ok]), _parity.bits(wr[ok]))
    st_g, st_o = eng.state(), ora.state()
    np.testing.assert_array_equal(_parity.bits(st_g['x'][pick]), _parity.bits(st_o['x']))
    np.testing.assert_array_equal(_parity.bits(st_g['y'][pick]), _parity.bits(st_o['y']))
    for k in ('step_count', 'reset_next', 'episode', 'n_sprites'):
      np.testing.assert_array_equal(st_g[k][pick], st_o[k], err_msg=k)
  eng.close()


def test_gpu_65600_environments_at_anti_aliasing_1(monkeypatch):
  """cluster_s5 at anti_aliasing 1 on the large-frame kernels: no scratch, the chunk is min(N, 65 535) -- two raster launches."""
  monkeypatch.setenv('SWB_LARGE_FRAMES', '1')
  _big_batch(workloads.build('cluster_s5', N_BIG, episodes_per_env=1, seed=5, anti_aliasing=1), 4, many=False)


def test_gpu_65600_environments_of_small_frames():
  """20 sprites on a 16 x 16 image at anti_aliasing 2: 1536 B of scratch per environment, so the clamp to 65 535 environments
  and not the scratch budget sets the chunk, and the vertical kernel runs with gridDim.z = 65 535."""
  assert 65535 * 32 * 16 * 3 < 256 << 20
  built = cases.scene(20, (16, 16), 2, N_BIG, scales=(0.05, 0.2, 0.4), seed=6, shape_names=('square', 'triangle', 'star_5'),
                      pool_entries=9973)        # (a prime: environments 65 535 and 65 536 play episodes 5697 and 5698)
  _big_batch(built, 4, many=True)


@pytest.mark.parametrize('total', [40, 64])
def test_gpu_device_sampler_of_forty_and_sixty_four_sprites(total):
  cases.device_sampler_case(total, num_envs=4)


def test_gpu_factors_and_sprite_types_beyond_sixteen():
  cases.factors_case(_gpu, n_envs=8)


@pytest.mark.parametrize('n_vertices,embodied', [(33, False), (64, False), (33, True), (64, True)])
def test_gpu_shapes_of_33_and_64_vertices_on_the_many_sprite_state_kernel(n_vertices, embodied):
  got = cases.wide_shapes_case(_gpu, n_vertices, embodied, 48, 12, aa=5)
  assert got['moved'] > 0
