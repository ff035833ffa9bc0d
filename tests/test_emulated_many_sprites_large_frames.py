"""The many-sprite state kernel (17 to 64 sprites) on large, wide and non-square frames, and both paths at the limits the
code states (4096 canvas pixels in either direction, 1024 image columns, 64 sprites, the vertex budget of the raster kernel's
LDS), on the emulated library against the oracle: state, rewards, step types and discounts bit-exact, frames +-0.  The
scenarios are those of tests/test_gpu_many_sprites_large_frames.py scaled to what the emulator carries (2 or 3 environments,
3 steps, strips instead of squares at the 4096 px limits).  TEST INFRASTRUCTURE: the emulator proves the arithmetic and control
flow of the kernel source, not what hipcc makes of it for gfx950 -- the GPU module runs the real thing."""
import pytest

from tests import _many_sprites_cases as cases


def _emu(cfg, pool):
  from tests import _emu_engine
  return _emu_engine.EmuEngine(cfg, pool)


def _error():
  from tests import _emu_engine
  return _emu_engine.EmuError


# S, image (w, h), anti_aliasing, task, action space, float32 positions
CROSS = [(24, (96, 96), 8, 'goal', 'select', True),          # a 768 px canvas: 48 blocks of 16 rows
         (40, (320, 36), 1, 'cluster', 'select', True),      # Clustering (13 clusters); the AA 1 store into obs at 320 columns; a last block of 4 rows
         (64, (200, 40), 4, 'goal', 'embodied', True),       # a non-square 800 x 160 canvas, full sprite tables
         (24, (320, 16), 2, 'meta', 'drag', False),          # more than 256 columns, MetaAggregated, float64 + velocities
         (64, (512, 32), 1, 'goal', 'drag', True),           # 512 columns at AA 1, 64 sprites
         (17, (64, 64), 10, 'goal', 'select', True)]         # just over the tuned sprite count on a 640 px canvas


@pytest.mark.parametrize('S,size,aa,task,space,f32', CROSS)
def test_emulated_many_sprites_on_large_frames(S, size, aa, task, space, f32):
  built = cases.scene(S, size, aa, 2, task=task, space=space, f32=f32, max_len=1, seed=S)
  got = cases.run_scene(_emu, built, 3)
  assert got['most'] == S


def test_emulated_many_sprites_on_large_frames_chunked(monkeypatch):
  """33 sprites at 40 x 40, anti_aliasing 5, a scratch budget of two environments' horizontal pass: three environments in
  chunks of two and one."""
  monkeypatch.setenv('SWB_LF_SCRATCH_BYTES', str(2 * 200 * 40 * 3))
  cases.run_scene(_emu, cases.scene(33, (40, 40), 5, 3, max_len=1), 3)


def test_emulated_setters_beyond_sixteen_on_a_large_canvas():
  cases.setters_case(_emu, steps=3, built=cases.scene(40, (176, 16), 4, 3, episodes_per_env=3, seed=1))      # (a 704 x 64 canvas)


def test_emulated_render_and_evaluate_on_a_large_canvas():
  cases.render_and_evaluate_case(_emu, built=cases.scene(40, (176, 16), 4, 3, task='cluster', max_len=30, seed=2))


# the accepted side of each limit, as strips: 4096 px wide, 1024 columns at AA 1, 4096 px tall, 4096 px tall at AA 16 (a
# Lanczos window of 97 taps)
LIMITS = [((1024, 16), 4), ((1024, 16), 1), ((16, 1024), 4), ((16, 256), 16)]


def _limit_case(size, aa):
  """(environments, steps): the canvases of 4096 rows cost the emulator 10 s a frame of 64 sprites, so they run one environment
  for two steps (no reset: the 4096 px wide strips, 64 rows, see one)."""
  return (1, 2) if aa * size[1] > 1024 else (2, 3)


@pytest.mark.parametrize('size,aa', LIMITS)
def test_emulated_limits_with_64_sprites(size, aa):
  """64 circles: 1920 polygon vertices, the largest scene of built-in shapes (104 KB of LDS at a 4096 px wide canvas)."""
  n_envs, steps = _limit_case(size, aa)
  tiny, small, large = cases.default_scales(size, aa)
  scales = (tiny, small / 4, small / 2, small, 0.12) if n_envs == 1 else None        # (4096 rows: one sprite in five of 550 rows)
  built = cases.scene(64, size, aa, n_envs, space='drag', max_len=1, episodes_per_env=1, shape_names=('circle',), ragged=False,
                      seed=aa, scales=scales)
  cases.run_scene(_emu, built, steps, want_most=64, want_reset=steps > 2)


@pytest.mark.parametrize('size,aa', LIMITS)
def test_emulated_limits_with_4_sprites(monkeypatch, size, aa):
  """(SWB_LARGE_FRAMES=1: a canvas of 256 x 4096 with up to 16 sprites is otherwise the tuned kernels'.)"""
  monkeypatch.setenv('SWB_LARGE_FRAMES', '1')
  n_envs, steps = _limit_case(size, aa)
  built = cases.scene(4, size, aa, n_envs, max_len=1, episodes_per_env=1, ragged=False, seed=aa, scales=(0.05, 0.3, 0.6))
  cases.run_scene(_emu, built, steps, many=False, check_claims=False, want_most=4, want_reset=steps > 2)


def test_emulated_refusals_one_step_past_each_limit():
  cases.refusals_case(_emu, _error())


@pytest.mark.parametrize('size,aa,budget', [((64, 64), 5, 3844), ((1024, 16), 4, 3420)])
def test_emulated_vertex_budget_is_a_boundary(size, aa, budget):
  """(160 KiB - 4384 B of head - 4 waves x (canvas width + span mask + 1024 B of crossings)) / 40 B per vertex, in steps of 4
  vertices: at a 320 px and at a 4096 px canvas."""
  assert cases.vertex_budget_case(_emu, _error(), size, aa) == budget


@pytest.mark.parametrize('n_vertices,embodied', [(33, False), (64, False), (64, True)])
def test_emulated_shapes_of_33_and_64_vertices_on_the_many_sprite_state_kernel(n_vertices, embodied):
  got = cases.wide_shapes_case(_emu, n_vertices, embodied, 2, 10)
  assert got['moved'] > 0
