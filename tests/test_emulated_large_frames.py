"""The large-frame render path (canvases wider than 640 px, images wider than 256 columns) on the emulated library.

The kernel source (tests/emu: the C-ABI host side and every kernel, compiled for the host against the emulation of the HIP
runtime) against the oracle, to the bar of the `-m gpu` parity tests: state, rewards, step types and discounts bit-exact,
frames +-0.  Geometries beyond the tuned kernels take the large-frame path by themselves; SWB_LARGE_FRAMES=1 sends the
existing workloads there too.  TEST INFRASTRUCTURE: the emulator proves the arithmetic and control flow of the source, not
its speed -- tests/test_gpu_large_frames.py runs the real thing.
"""
import numpy as np
import pytest

from spriteworld_amd import workloads
from tests import _parity
from tests import _util


def _emu(cfg, pool):
  from tests import _emu_engine
  return _emu_engine.EmuEngine(cfg, pool)


def _run(name, n_envs, steps, aa, seed=0):
  """-> the FIRST steps seen."""
  return _parity.run(_emu, name, n_envs, steps, aa, seed=seed, episodes_per_env=2, expect={'large_frames': 1})[0]


@pytest.mark.parametrize('geom,aa', [('96x96', 8), ('200x40', 4), ('320x32', 1)])
def test_emulated_large_frame_geometries(geom, aa):
  """Geometries the tuned kernels refuse: a 768 px canvas, a non-square 800 x 160 canvas (the reference's canvas is
  (AA * image_size[0]) wide and (AA * image_size[1]) tall), an image of 320 columns at anti_aliasing 1."""
  _run('geom_' + geom, 2, 3, aa)


def test_emulated_large_frames_across_a_reset(monkeypatch):
  """Episodes of at most 12 steps: the state phase resets environments from the pool and the render kernels draw the new
  episode."""
  monkeypatch.setenv('SWB_LARGE_FRAMES', '1')
  firsts = _run('geom_64x48', 2, 15, 3)
  assert firsts > 2          # (the first step, and resets after it)


@pytest.mark.parametrize('name,n_envs,steps,aa', [('goal_s5', 3, 4, 5), ('tiny_s6', 3, 3, 5), ('tiny_s6', 3, 3, 1),
                                                   ('cluster_s5', 2, 3, 2), ('geom_100x60', 2, 2, 3)])
def test_emulated_large_frames_forced(monkeypatch, name, n_envs, steps, aa):
  monkeypatch.setenv('SWB_LARGE_FRAMES', '1')
  _run(name, n_envs, steps, aa)


@pytest.mark.parametrize('n_vertices', [33, 64])
def test_emulated_large_frames_shapes_of_33_to_64_edges(monkeypatch, n_vertices):
  from spriteworld_amd import shapes
  monkeypatch.setenv('SWB_LARGE_FRAMES', '1')
  with _util.swapped_shape('circle', shapes.polygon(n_vertices)):
    _run('tiny_s6', 3, 3, 5)


def test_emulated_large_frames_chunked(monkeypatch):
  """A scratch budget of one environment's horizontal pass: every environment rendered in a chunk of its own."""
  monkeypatch.setenv('SWB_LARGE_FRAMES', '1')
  monkeypatch.setenv('SWB_LF_SCRATCH_BYTES', str(64 * 5 * 64 * 3))
  _run('goal_s5', 3, 3, 5)


def test_emulated_large_frames_sprite_setters(monkeypatch):
  from tests import _setter_cases
  monkeypatch.setenv('SWB_LARGE_FRAMES', '1')
  _setter_cases.run_parity(_emu, 'goal_s5', 3, 3, 3, expect={'large_frames': 1})


def test_emulated_large_frames_render_and_trim():
  """observation() (swb_render: the render kernels alone) equals the step's frame; trim() is a successful no-op."""
  cfg, pool, sample = workloads.build('geom_96x96', 2, episodes_per_env=2, seed=4, anti_aliasing=8)
  eng = _emu(cfg, pool)
  rng = np.random.default_rng(9)
  for _ in range(2):
    eng.step(sample(rng))
  frame = eng.outputs_host()['obs'].copy()
  eng.obs.fill_(0x33)
  np.testing.assert_array_equal(eng.render().numpy(), frame)
  info = eng.variant()
  assert info['large_frames'] == 1 and info['run_list_bytes'] == 0 and 'swb_lf_raster_kernel' in info['kernel']
  assert eng.trim() == 0
  eng.close()


def test_emulated_limits_name_the_limit(monkeypatch):
  from tests import _emu_engine
  for name, aa, what in (('geom_256x256', 17, '4096'), ('geom_1028x16', 1, '1024'), ('geom_516x16', 8, '4128x128 too large: at most 4096')):
    cfg, pool, _ = workloads.build(name, 1, episodes_per_env=1, anti_aliasing=aa)
    with pytest.raises(_emu_engine.EmuError, match=what):
      _emu(cfg, pool)
  # the height alone: a 256 px wide canvas of up to 16 sprites is a large frame only when sent there (the tuned kernels take
  # 4100 rows; tests/_many_sprites_cases.refusals_case has the case with 20 sprites, unforced)
  monkeypatch.setenv('SWB_LARGE_FRAMES', '1')
  cfg, pool, _ = workloads.build('geom_64x1025', 1, episodes_per_env=1, anti_aliasing=4)
  with pytest.raises(_emu_engine.EmuError, match='256x4100 too large: at most 4096'):
    _emu(cfg, pool)
