"""The kernel SOURCE against the oracle and the reference's recorded outputs, on the CPU.

tests/emu compiles spriteworld_amd/csrc (the C-ABI host side and the fused step kernel, every variant incl. the OV
builds) for the host against an emulation of the HIP runtime and of the wave-level builtins: work-items are fibres,
cross-lane operations (ballot, readlane, shuffles, DPP moves, wave barriers) are rendezvous of the 64 lanes that also
check that all lanes arrive from the same source line.  These tests are what the CPU suite can say about the device
code where no GPU exists: same inputs, same bar as the `-m gpu` parity tests (tests/_parity.py: state, rewards, step types,
discounts bit-exact; frames +-0), at sizes the emulator finishes in seconds.  The scenarios with a body of their own are shared
with tests/test_gpu_parity.py (tests/_kernel_cases.py), tests/test_gpu_vs_reference.py (tests/_reference_cases.py) and the
`-m gpu` tests of the sampler and the host surface (tests/_sampler_cases.py, tests/_surface_cases.py).

TEST INFRASTRUCTURE: the emulated library is never loaded by the product, proves nothing about timing, register
allocation or anything else the hipcc build adds -- the `-m gpu` tests run the real thing.  What it does prove is the
arithmetic and control flow of the kernel source, e.g. before a kernel change is taken to the (scarce) GPU.
"""
import numpy as np
import pytest

from tests import _kernel_cases as cases
from tests import _parity
from tests import _reference_cases
from tests import _sampler_cases
from tests import _surface_cases
from tests import _util


def _emu(cfg, pool):
  from tests import _emu_engine
  return _emu_engine.EmuEngine(cfg, pool)


def _run(name, n_envs, steps, aa, seed=0):
  _parity.run(_emu, name, n_envs, steps, aa, seed=seed)


# the workloads tests/test_gpu_parity.py runs through `_parity.run` (every kernel variant, every task / action space / dtype), a few
# environments each
@pytest.mark.parametrize('name,n_envs,steps,aa', [
    ('goal_s5', 3, 4, 5), ('cluster_s5', 3, 4, 5), ('goal_s5', 3, 3, 1), ('cluster_s5', 3, 3, 1), ('embodied_s12', 2, 3, 5),
    ('sorting_s4', 3, 4, 5), ('f64_drag', 4, 5, 3), ('f64_cluster', 4, 5, 3), ('cluster6_s12', 3, 4, 2), ('cluster9_s16', 3, 4, 2), ('ragged_s16', 8, 4, 5),
    ('ragged_s16_embodied', 8, 4, 5), ('wide_s4', 2, 3, 5), ('wide_s4', 2, 3, 1), ('tiny_s6', 4, 3, 5), ('tiny_s6', 4, 3, 1),
    ('goal_s5_f32a', 3, 4, 5), ('cluster_s5_f32a', 3, 4, 5), ('f64_drag_f32a', 3, 4, 3), ('f64_cluster_f32a', 3, 4, 3),
    ('sorting_s4_f32a', 3, 4, 5)])
def test_emulated_kernel_equals_oracle(name, n_envs, steps, aa):
  _run(name, n_envs, steps, aa)


@pytest.mark.parametrize('n_vertices', [33, 40, 64])
@pytest.mark.parametrize('name,n_envs,aa', [('cluster_s5', 3, 5), ('goal_s5', 3, 1), ('tiny_s6', 4, 5)])
def test_emulated_kernel_shapes_of_33_to_64_edges(n_vertices, name, n_envs, aa):
  """The C ABI takes shapes of up to SWB_MAX_SHAPE_VERTS = 64 vertices; from 33 on an edge gets ONE lane of the edge-lane scatter
  (G = 64 / n_edges = 1), whose lane -> edge reciprocal is then 2^16 itself (round 4 packed it in 16 bits: every lane served
  edge 0 -- ADVICE round 4).  No built-in shape has more than 30 vertices: the circle is swapped for a regular n-gon."""
  from spriteworld_amd import shapes
  with _util.swapped_shape('circle', shapes.polygon(n_vertices)):
    _run(name, n_envs, 3, aa)


@pytest.mark.parametrize('geom,aa', [('96x48', 3), ('48x96', 2), ('256x64', 2), ('160x160', 4), ('128x128', 1),
                                     ('100x60', 3), ('64x256', 1), ('32x32', 8), ('32x512', 4)])
def test_emulated_kernel_image_geometries(geom, aa):
  _run('geom_' + geom, 2, 2, aa)


@pytest.mark.parametrize('seed', range(8))
def test_emulated_kernel_randomised_configurations(seed):
  _run('fuzz_%d' % seed, 3, 3, 5, seed=seed)


def test_emulated_run_list_capacity_follows_the_sprite_count():
  """Ten sprites on a 60-row canvas (192 x 60 at anti_aliasing = 3; seed 2681 of tools/fuzz_sweep.py, found in round 5): rows of
  four to eight visible spans, 241 .. 300 units of run list for 60 rows -- the capacity was 4 units per canvas row whatever the
  sprite count, the environment was flagged SWB_ENV_ERR_SPAN_OVERFLOW at step 7 and its frame was short of a batch of rows.
  Now (S + 1) units per row: any scene of convex sprites, folded or not."""
  _run('fuzz_2681', 64, 8, 5, seed=2681)


@pytest.mark.parametrize('name,n_envs,aa', [('embodied_s12', 2, 5), ('ragged_s16', 6, 5), ('cluster_s5', 3, 1)])
def test_emulated_kernel_span_overflow_slots(monkeypatch, name, n_envs, aa):
  """Rows with more than three visible spans take the HBM overflow path when the LDS lists are switched off."""
  monkeypatch.setenv('SWB_LDS_SPAN_CAP', '0')
  _run(name, n_envs, 3, aa)


# ---- the hand-off between the two kernels of a step (round 3): bands of output rows, cost-ordered dispatch, list capacity
@pytest.mark.parametrize('bands,band_tasks', [(1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (8, 0), (8, 1)])
@pytest.mark.parametrize('name,n_envs,aa', [('cluster_s5', 3, 5), ('embodied_s12', 2, 5), ('geom_100x60', 2, 3), ('geom_64x256', 2, 1),
                                            ('geom_96x48', 2, 3), ('cluster_s5', 3, 1)])
def test_emulated_kernel_any_number_of_bands(monkeypatch, bands, name, n_envs, aa, band_tasks):
  """The resample / fill kernel splits an image into bands of output rows (one wave each); a band starts with the output rows
  already in flight at its first canvas row.  Every band count gives the same frames -- whether the second kernel's tasks are
  whole lists (every band of a list in the list's place of the cost order) or single bands filed under their own cost
  (round 6, swb_params::band_tasks: what launches of four waves or more per SIMD use)."""
  monkeypatch.setenv('SWB_BANDS', str(bands))
  monkeypatch.setenv('SWB_BAND_TASKS', str(band_tasks))
  _run(name, n_envs, 3, aa)


def test_emulated_kernel_without_cost_ordered_dispatch(monkeypatch):
  monkeypatch.setenv('SWB_NO_COST_ORDER', '1')
  _run('cluster_s5', 11, 4, 5)
  _run('cluster_s5', 11, 3, 1)
  _run('geom_256x64', 3, 2, 2)


@pytest.mark.parametrize('name,n_envs,aa', [('cluster_s5', 19, 5), ('embodied_s12', 5, 5), ('ragged_s16', 13, 5), ('geom_128x128', 9, 1),
                                            ('sorting_s4', 11, 5), ('cluster_s5', 13, 1), ('tiny_s6', 7, 1)])
def test_emulated_cover_launches_in_cost_order(monkeypatch, name, n_envs, aa):
  monkeypatch.setenv('SWB_COVER_ORDER', '1')
  cases.cover_cost_order_case(_emu, name, n_envs, aa)


@pytest.mark.parametrize('seed', [1, 4, 6])
def test_emulated_cover_cost_order_on_randomised_configurations(monkeypatch, seed):
  """Random task / action space / geometry / sprite count configurations (the fuzz workloads) with the cost-ordered cover launch
  and short dealing rounds switched on: the dispatch never changes a result."""
  monkeypatch.setenv('SWB_COVER_ORDER', '1')
  monkeypatch.setenv('SWB_DEAL_SHIFT', '1')
  _run('fuzz_%d' % seed, 21, 4, 5, seed=seed)


@pytest.mark.parametrize('shift', ['1', '2'])
def test_emulated_kernel_cost_order_dealt_in_alternating_rounds(monkeypatch, shift):
  """The resample / fill blocks of a shard take its cost-ordered tasks in rounds of 2^deal_shift blocks, odd rounds in ascending
  order (32 blocks per round on the GPU: the compute units of an XCD; SWB_DEAL_SHIFT shortens the rounds so that small batches
  have several, with a short last one).  Every task is served exactly once."""
  monkeypatch.setenv('SWB_DEAL_SHIFT', shift)
  for n in (33, 70, 97):
    _run('cluster_s5', n, 2, 5)
  _run('geom_256x64', 21, 2, 2)
  _run('geom_128x128', 35, 2, 1)


@pytest.mark.parametrize('name,aa', [('embodied_s12', 5), ('geom_256x64', 2), ('geom_128x128', 1)])
def test_emulated_kernel_cost_order_files_every_column_group(name, aa):
  """Images wider than 64 columns: every (environment, group of 64 columns) is a task of its own in the cost-ordered lists,
  filed under the length of that group's run list."""
  for n in (1, 7, 9):
    _run(name, n, 2, aa)


@pytest.mark.parametrize('name,aa', [('cluster_s5', 5), ('cluster_s5', 1)])
def test_emulated_kernel_cost_order_covers_every_environment(name, aa):
  """Sizes that do not divide by the eight shards or the four waves of a resample block."""
  for n in (1, 7, 9, 33):
    _run(name, n, 3, aa)


@pytest.mark.parametrize('name,n_envs', [('cluster_s5', 3), ('tiny_s6', 4), ('wide_s4', 2), ('ragged_s16', 8)])
def test_emulated_fill_kernel_for_narrow_images(monkeypatch, name, n_envs):
  """anti_aliasing = 1: images of up to 64 columns are painted by the cover kernel itself (the default, in every other AA = 1
  case of this file); SWB_NO_PAINT_IN_COVER sends them through the run lists and the fill kernel like wider images."""
  monkeypatch.setenv('SWB_NO_PAINT_IN_COVER', '1')
  _run(name, n_envs, 3, 1)


@pytest.mark.parametrize('run_cap,bands,n_envs', [(24, 1, 4), (8, 4, 1), (12, 8, 3), (40, 2, 5)])
def test_emulated_kernel_run_list_overflow_is_flagged(monkeypatch, run_cap, bands, n_envs):
  """The emulated build counts run-record reads at or beyond the capacity."""
  monkeypatch.setenv('SWB_BANDS', str(bands))
  monkeypatch.setenv('SWB_BAND_TASKS', str(n_envs & 1))    # (either form of the second kernel's tasks)
  cases.run_list_overflow_case(_emu, monkeypatch, [('cluster_s5', 5), ('wide_s4', 1)], run_cap, n_envs, steps=3, quantifier=np.any)


@pytest.mark.parametrize('run_cap,bands,arena', [(8, 1, 1 << 20), (8, 4, 1 << 20), (12, 8, 1 << 20), (40, 2, 1 << 20), (24, 1, 600)])
def test_emulated_kernel_run_lists_continue_in_the_shared_arena(monkeypatch, run_cap, bands, arena):
  """An arena of 600 units is too small: two 12-sprite scenes at 128x128 need thousands."""
  cases.arena_move_case(_emu, monkeypatch, [('cluster_s5', 5, 3, 5), ('geom_160x48', 3, 3, 1), ('embodied_s12', 2, 3, 5)], run_cap, bands,
                        arena, episodes_per_env=2, seed=1, rng_seed=0, exhausted_by=None if arena >= 1 << 20 else 'embodied_s12')


def test_emulated_run_lists_are_trimmed_after_the_third_rendering_launch():
  cases.trim_case(_emu, [('embodied_s12', 3, 5), ('cluster_s5', 6, 5), ('geom_160x48', 3, 1)], seed=2, rng_seed=5, steps=7, total_halves=False)


@pytest.mark.parametrize('name', _util.golden_cases())
def test_emulated_kernel_reproduces_the_reference_fixtures(name):
  """tests/golden/*.npz (outputs recorded from the unmodified reference): the first 50 steps of every fixture."""
  cfg, pool, z = _util.load_golden(name)
  eng = _emu(cfg, pool)

  def step(a):
    eng.step(a)
    return eng.outputs_host()

  short = {k: z[k] for k in z.files}
  short['actions'] = z['actions'][:50]
  _util.check_against_golden(eng, cfg, short, eng.state, step, 'emu/' + name)
  eng.close()


@pytest.mark.parametrize('name,n_envs,steps,aa', [('goal_s5', 6, 5, 5), ('cluster_s5', 6, 4, 1), ('embodied_s12', 3, 3, 5),
                                                   ('geom_256x64', 3, 3, 2), ('geom_32x32', 3, 3, 8)])
def test_emulated_ov_kernels_sprite_setters(name, n_envs, steps, aa):
  """The scenarios of tests/test_gpu_setters.py on the emulated library: swb_set_sprite_attr's host arithmetic, the
  override arrays and the OV builds of the step kernel against the oracle's setters."""
  from tests import _setter_cases
  _setter_cases.run_parity(_emu, name, n_envs, steps, aa)


def test_emulated_setters_factors_and_reset():
  from tests import _emu_engine, _setter_cases
  _setter_cases.factors_and_reset_case(_emu, _emu_engine.EmuError)


def test_emulated_live_sprite_handles(monkeypatch):
  """environment.BatchedEnvironment + sprite.LiveSprite on the emulated library, checked against matplotlib."""
  from spriteworld_amd import environment
  from tests import _emu_engine, _setter_cases
  monkeypatch.setattr(environment._engine, 'Engine', _emu_engine.EmuTorchEngine)
  _setter_cases.live_sprite_case()


def test_emulator_refuses_cross_lane_operations_under_divergence():
  """The rendezvous checks the call site: the build carries a self-test kernel whose lanes reach two different
  ballots; it must be caught (subprocess: the emulator aborts)."""
  import subprocess
  import sys
  code = ('import ctypes, sys; sys.path.insert(0, %r); from tests.emu import build_emu; '
          'l = ctypes.CDLL(build_emu.build()); l.emu_selftest_divergent_ballot()' % _util.ROOT)
  p = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True)
  assert p.returncode != 0 and 'divergent control flow' in p.stderr, p.stderr[-500:]


# ---- the device-side reset sampler (swb_sampler.hip.inc, one work-item per pool entry) on the emulated library: the bodies of
# tests/_sampler_cases.py (the `-m gpu` tests of tests/test_device_sampler.py), the engine interface backed by the emulator
def _patch_engine(monkeypatch):
  from spriteworld_amd import environment
  from tests import _emu_engine
  monkeypatch.setattr(environment._engine, 'Engine', _emu_engine.EmuTorchEngine)


@pytest.mark.parametrize('case', ['cobra_like', 'embodied_like', 'holdouts', 'hsv_mixed', 'mixed_types', 'sorting_like'])
def test_emulated_sampler_kernel_equals_the_python_model(monkeypatch, case):
  assert sorted(_sampler_cases.CASES) == ['cobra_like', 'embodied_like', 'holdouts', 'hsv_mixed', 'mixed_types', 'sorting_like']
  _patch_engine(monkeypatch)
  _sampler_cases.pool_matches_the_model_case(case)


def test_emulated_sampler_shards_and_refresh(monkeypatch):
  _patch_engine(monkeypatch)
  _sampler_cases.shards_case()
  _sampler_cases.refresh_case()


@pytest.mark.skipif(not __import__('oracle.ref_harness', fromlist=['x']).reference_available(), reason='reference tree not present')
def test_emulated_factors_kernel_equals_reference_sprite_factors():
  """renderers/handcrafted.py:29-82 SpriteFactors of the UNMODIFIED reference on a running environment (incl. sprites
  modified through the setters, sprite.py:152-175) against swb_factors of the emulated library, every step."""
  import copy
  from oracle import ref_harness
  ref_harness.load_reference()
  from spriteworld import action_spaces, environment, renderers, sprite, tasks
  from spriteworld_amd import _abi, lowering, shapes
  from spriteworld_amd import sprite as sprite_lib
  rng = np.random.RandomState(8)
  names = list(shapes.SHAPES.keys())

  def gen():
    return [sprite.Sprite(x=float(rng.uniform(0.2, 0.8)), y=float(rng.uniform(0.2, 0.8)), shape=str(rng.choice(names)),
                          angle=float(rng.choice([0, 40, 200])), scale=float(rng.choice([0.1, 0.2])),
                          c0=int(rng.randint(0, 256)), c1=int(rng.randint(0, 256)), c2=int(rng.randint(0, 256)),
                          x_vel=float(rng.uniform(-0.01, 0.01)), y_vel=float(rng.uniform(-0.01, 0.01)))
            for _ in range(int(rng.randint(1, 4)))]

  episodes = [gen() for _ in range(5)]
  task = tasks.FindGoalPosition(goal_position=(0.5, 0.5), terminate_distance=0.05)
  aspace = action_spaces.SelectMove(scale=0.2)
  rends = {'image': renderers.PILRenderer(image_size=(32, 32), anti_aliasing=2), 'factors': renderers.SpriteFactors()}
  cfg = lowering.lower_config(task, aspace, {'image': rends['image']}, True, 9, 1, 3,
                              pos_is_f32=(lowering.position_dtype(episodes) == np.float32))
  pool = lowering.lower_episodes(episodes, task, {'image': rends['image']}, max_sprites=3).assign_round_robin(1)
  eng = _emu(cfg, pool)
  it = (copy.deepcopy(e) for e in [episodes[0]] + episodes * 20)
  env = environment.Environment(task=task, action_space=aspace, renderers=rends, init_sprites=lambda: next(it),
                                keep_in_frame=True, max_episode_length=9)
  arng = np.random.RandomState(3)
  for t in range(40):
    if t % 4 == 2 and env._sprites and not env._reset_next_step:
      k = int(arng.randint(0, len(env._sprites)))
      attr, value = [('angle', 77.0), ('scale', 0.33), ('shape', 'star_5')][(t // 4) % 3]
      setattr(env._sprites[k], attr, value)
      eng.set_sprite_attr(0, k, {'shape': _abi.ATTR_SHAPE, 'angle': _abi.ATTR_ANGLE, 'scale': _abi.ATTR_SCALE}[attr],
                          shapes.shape_index(value) if attr == 'shape' else value)
    a = arng.uniform(0, 1, 4)
    ts = env.step(a)
    eng.step(a[None])
    got = eng.factors()[0]
    want = ts.observation['factors']
    assert len(want) == eng.state()['n_sprites'][0]
    for s, row in enumerate(want):
      assert [row[f] for f in sprite_lib.FACTOR_NAMES] == got[s].tolist(), (t, s)
    assert not got[len(want):].any()
    assert np.array_equal(ts.observation['image'], eng.outputs_host()['obs'][0]), t


@pytest.mark.skipif(not __import__('oracle.ref_harness', fromlist=['x']).reference_available(), reason='reference tree not present')
@pytest.mark.parametrize('module,mode', _reference_cases.CONFIGS)
def test_emulated_kernel_equals_the_unmodified_reference(module, mode):
  """Every shipped config in both modes: the UNMODIFIED reference `Environment` and the kernel source (emulated) stepped side
  by side in one process, no oracle in between (tests/_reference_cases.py)."""
  _reference_cases.side_by_side(_emu, module, mode, seed=33, n_eps=12, n_steps=100)


def test_emulated_results_do_not_depend_on_lane_order_or_lds_garbage():
  """The same parity tests with the lanes taking their turns in DESCENDING order between rendezvous and another garbage
  byte in the uninitialised LDS (both are read once per process: a subprocess).  A cross-lane hazard on LDS without a
  fence, or a read of LDS nothing wrote, would change a result."""
  import os
  import subprocess
  import sys
  env = dict(os.environ, SWB_EMU_LANE_ORDER='reverse', SWB_EMU_LDS_FILL='0x00')
  p = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-p', 'no:cacheprovider', '-k',
                      'equals_oracle and (cluster_s5 or embodied or f64_cluster or ragged_s16 or tiny or sorting) or setters and goal_s5'],
                     cwd=_util.ROOT, env=env, capture_output=True, text=True)
  assert p.returncode == 0 and ' passed' in p.stdout, p.stdout[-1500:]


# ---- the host-API bodies of tests/_surface_cases.py (the `-m gpu` tests of tests/test_env_spec_conformance.py,
# test_gym_wrapper.py, test_host_api.py) with the engine interface backed by the emulated library: the dm_env / gym surface over
# the kernel source
def test_emulated_environment_conforms_to_its_specs(monkeypatch):
  """tests/environment_test.py:30-51 (dm_env EnvironmentTestMixin), as re-expressed for the N = 1 Environment."""
  _patch_engine(monkeypatch)
  for make in (_surface_cases._reference_test_env, _surface_cases._rendered_env):
    _surface_cases.reset_and_step_protocol_case(make)
    _surface_cases.longer_action_sequence_case(make)
  _surface_cases.specs_are_specs_case()


def test_emulated_gym_wrapper_and_single_environment(monkeypatch):
  _patch_engine(monkeypatch)
  for embodied in (False, True):
    _surface_cases.reference_gym_wrapper_episode_pattern_case(embodied)
  _surface_cases.single_environment_run_loop_case()
  _surface_cases.sprite_factors_and_action_noise_case()


@pytest.mark.parametrize('f32', [True, False], ids=['f32pos', 'f64pos'])
@pytest.mark.parametrize('name', __import__('tests._position_cases', fromlist=['CASES']).CASES)
def test_emulated_kernel_tasks_that_filter_on_position(name, f32):
  cases.position_filter_case(_emu, name, f32, n_envs=5, min_flips=20)
