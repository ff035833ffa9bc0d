"""GPU parity: the HIP engine (through the C ABI) against the CPU oracle.

Both sides consume the same `SwbConfig`, the same pool arrays and the same
actions.  Bar (BASELINE.json north_star): sprite positions, step types,
discounts, success flags bit-exact; frames within +-1 LSB (we require +-0);
rewards bit-exact.
"""
import numpy as np
import pytest

from spriteworld_amd import workloads
from tests import _parity

pytestmark = pytest.mark.gpu


def _engine(cfg, pool):
  from spriteworld_amd import engine
  return engine.Engine(cfg, pool)


def _run(name, n_envs, steps, aa, seed=0):
  _parity.run(_engine, name, n_envs, steps, aa, seed=seed)


def test_goal_s5_aa5():
  _run('goal_s5', 256, 30, 5)


def test_cluster_s5_aa5():
  _run('cluster_s5', 256, 30, 5)


def test_goal_s5_aa1():
  _run('goal_s5', 256, 12, 1)


def test_embodied_s12_128():
  _run('embodied_s12', 64, 20, 5)


def test_sorting_meta():
  _run('sorting_s4', 128, 20, 5)


def test_f64_sprites_drag_and_drop_motion_cost():
  _run('f64_drag', 256, 40, 3)


def test_f64_sprites_clustering_three_clusters():
  _run('f64_cluster', 256, 40, 3)


def test_six_clusters_scalar_davies_bouldin_path():
  _run('cluster6_s12', 128, 25, 2)


def test_nine_clusters_ratio_matrix_in_two_passes():
  _run('cluster9_s16', 128, 25, 2)


@pytest.mark.parametrize('name', ['ragged_s16', 'ragged_s16_embodied'])
def test_ragged_sprite_counts_zero_to_sixteen(name):
  _run(name, 128, 20, 5)


def test_cluster_s5_aa1():
  _run('cluster_s5', 128, 10, 1)


def test_wide_sprites_chunked_scan_conversion():
  _run('wide_s4', 128, 12, 5)


def test_wide_sprites_aa1():
  _run('wide_s4', 128, 8, 1)


@pytest.mark.parametrize('n_vertices', [33, 40, 64])
@pytest.mark.parametrize('name,aa', [('cluster_s5', 5), ('goal_s5', 1), ('tiny_s6', 5)])
def test_shapes_of_33_to_64_edges(n_vertices, name, aa):
  """Shapes beyond 32 edges (the C ABI allows 64): one lane per edge in the edge-lane scatter -- ADVICE round 4 (every lane served
  edge 0).  The circle of the shape table is swapped for a regular n-gon on both sides."""
  from spriteworld_amd import shapes
  from tests import _util
  with _util.swapped_shape('circle', shapes.polygon(n_vertices)):
    _run(name, 128, 8, aa)


def test_ten_sprites_on_a_sixty_row_canvas_fit_their_run_lists():
  """Seed 2681 of tools/fuzz_sweep.py: the run-list capacity follows the sprite count (round 5; it was 4 units per canvas row and
  this scene, 4 - 8 visible spans in most rows, overflowed it: flagged, frame short of a batch of rows)."""
  _run('fuzz_2681', 64, 10, 5, seed=2681)


def test_tiny_sprites_degenerate_polygons():
  _run('tiny_s6', 256, 10, 5)


def test_tiny_sprites_aa1():
  _run('tiny_s6', 256, 6, 1)


@pytest.mark.parametrize('name,n_envs,aa', [('embodied_s12', 48, 5), ('ragged_s16', 96, 5), ('wide_s4', 64, 5), ('cluster_s5', 128, 1)])
def test_span_lists_spill_to_the_hbm_overflow_slots(monkeypatch, name, n_envs, aa):
  """Rows with more than three visible spans normally continue in LDS; with the LDS lists switched off
  (SWB_LDS_SPAN_CAP=0, read by swb_create) every such row takes the HBM overflow path: a slot from the
  bitmap on first use, given back at kernel end (so consecutive steps reuse the few slots)."""
  monkeypatch.setenv('SWB_LDS_SPAN_CAP', '0')
  _run(name, n_envs, 8, aa)


@pytest.mark.parametrize('name,aa', [('goal_s5_f32a', 5), ('cluster_s5_f32a', 5), ('f64_drag_f32a', 3),
                                     ('f64_cluster_f32a', 3), ('sorting_s4_f32a', 5)])
def test_float32_actions(name, aa):
  """Actions of the dtype action_spec() declares: float32 motion / click / cost arithmetic (NEP 50)."""
  _run(name, 192, 25, aa)


@pytest.mark.parametrize('geom,aa', [('96x48', 3), ('48x96', 2), ('256x64', 2), ('160x160', 4), ('128x128', 1),
                                     ('100x60', 3), ('64x256', 1), ('32x32', 8)])
def test_image_geometries(geom, aa):
  """Non-square and wide images: every kernel variant (canvas words x output columns x rows in flight)."""
  _run('geom_' + geom, 48, 6, aa)


@pytest.mark.parametrize('seed', range(24))
def test_randomised_configurations(seed):
  """Seeded random configurations: geometry x anti-aliasing x sprite counts x shapes x task x action space x dtype."""
  _run('fuzz_%d' % seed, 64, 10, 5, seed=seed)


# ---- the hand-off between the two kernels of a step (round 3)
@pytest.mark.parametrize('bands,band_tasks', [(1, 0), (2, 0), (2, 1), (4, 0), (4, 1), (8, 0), (8, 1)])
@pytest.mark.parametrize('name,n_envs,aa', [('cluster_s5', 64, 5), ('embodied_s12', 32, 5), ('geom_100x60', 32, 3), ('geom_64x256', 32, 1),
                                            ('cluster_s5', 64, 1)])
def test_any_number_of_bands(monkeypatch, bands, name, n_envs, aa, band_tasks):
  """Bands of output rows (one wave of the resample / fill kernel each; small batches use several): same frames, whether a task
  of the second kernel is a whole list or one band of it filed under its own cost (swb_params::band_tasks)."""
  monkeypatch.setenv('SWB_BANDS', str(bands))
  monkeypatch.setenv('SWB_BAND_TASKS', str(band_tasks))
  _run(name, n_envs, 3, aa)


@pytest.mark.parametrize('name,n_envs,aa', [('goal_s5', 1024, 5), ('cluster_s5', 2048, 5), ('geom_128x128', 1024, 1), ('embodied_s12', 700, 5)])
def test_small_batches_file_their_bands_as_tasks_of_their_own(name, n_envs, aa):
  """BASELINE configs[1]'s size and its neighbours: the engine picks 4 bands and files every band as a task (no switches set)."""
  _run(name, n_envs, 3, aa)


@pytest.mark.parametrize('n_envs', [1, 7, 9, 33, 1000])
def test_cost_ordered_dispatch_covers_every_environment(n_envs):
  """Batch sizes that do not divide by the eight shards of the cost buckets or the four waves of a resample block."""
  _run('cluster_s5', n_envs, 3, 5)
  _run('cluster_s5', n_envs, 2, 1)


@pytest.mark.parametrize('name,aa', [('embodied_s12', 5), ('geom_256x64', 2), ('geom_128x128', 1)])
@pytest.mark.parametrize('n_envs', [1, 7, 33, 250])
def test_cost_ordered_dispatch_files_every_column_group(name, aa, n_envs):
  """Images wider than 64 columns: every (environment, group of 64 columns) is a task of its own in the cost-ordered lists,
  filed under the length of that group's run list (2 and 4 groups; resample and fill kernels)."""
  _run(name, n_envs, 3, aa)


@pytest.mark.parametrize('name,n_envs,aa', [('cluster_s5', 33, 5), ('cluster_s5', 6000, 5), ('embodied_s12', 300, 5), ('ragged_s16', 257, 5),
                                            ('geom_128x128', 700, 1), ('sorting_s4', 1001, 5), ('cluster_s5', 6000, 1), ('tiny_s6', 333, 1)])
def test_cover_launches_in_cost_order(monkeypatch, name, n_envs, aa):
  """Launches of more than one round of cover waves (6000 environments here) take the environments in order of what their cover
  wave cost in the previous launch; SWB_COVER_ORDER asks for it at any batch size.  The order is only used after a launch that
  filed every environment (a step without an observation in between: one launch in plain order)."""
  from oracle import oracle
  from spriteworld_amd import engine
  monkeypatch.setenv('SWB_COVER_ORDER', '1')
  _run(name, n_envs, 4, aa)
  cfg, pool, sample = workloads.build(name, n_envs, episodes_per_env=3, seed=1, anti_aliasing=aa)
  ora, eng = oracle.Engine(cfg, pool), engine.Engine(cfg, pool)
  rng = np.random.default_rng(7)
  for t in range(6):
    a = sample(rng)
    want = ora.step(a)
    eng.step(a, render=(t != 2))                     # launch 2 renders nothing and files nothing
    if t == 2:
      continue
    got = eng.outputs_host()
    assert not got['error'].any()
    np.testing.assert_array_equal(got['step_type'], want['step_type'])
    np.testing.assert_array_equal(_parity.bits(eng.state()['x']), _parity.bits(ora.state()['x']))
    assert np.array_equal(got['obs'], want['obs']), t
  eng.close()


@pytest.mark.parametrize('shift', ['1', '2', '5'])
def test_cost_order_dealt_in_alternating_rounds(monkeypatch, shift):
  """The resample / fill blocks of a shard take its cost-ordered tasks in rounds of 2^deal_shift blocks (5: the 32 compute units of
  an XCD), odd rounds in ascending order; SWB_DEAL_SHIFT shortens the rounds.  Every task is served exactly once, whatever the
  number of rounds and the length of the last one."""
  monkeypatch.setenv('SWB_DEAL_SHIFT', shift)
  for n in (33, 97, 1500, 3000):
    _run('cluster_s5', n, 2, 5)
  _run('geom_256x64', 300, 2, 2)
  _run('geom_128x128', 700, 2, 1)


def test_without_cost_ordered_dispatch(monkeypatch):
  monkeypatch.setenv('SWB_NO_COST_ORDER', '1')
  _run('cluster_s5', 100, 4, 5)
  _run('geom_256x64', 9, 2, 2)


def test_run_list_overflow_is_flagged(monkeypatch):
  from spriteworld_amd import _abi, engine
  monkeypatch.setenv('SWB_RUN_CAP', '24')
  monkeypatch.setenv('SWB_ARENA_UNITS', '0')             # (no arena for an outgrown list to move to)
  cfg, pool, sample = workloads.build('cluster_s5', 64, episodes_per_env=2, seed=0, anti_aliasing=5)
  eng = engine.Engine(cfg, pool)
  eng.step(sample(np.random.default_rng(0)))
  assert (eng.outputs_host()['error'] & _abi.ENV_ERR_SPAN_OVERFLOW).all()
  eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('run_cap,bands', [(8, 1), (12, 4), (40, 2), (64, 8)])
def test_run_lists_that_outgrow_their_part_move_to_the_arena(monkeypatch, run_cap, bands):
  """Round 6: with an own part of 8 .. 64 units every run list outgrows it and moves to a segment of the shared arena (several
  times); nothing changes in what the step returns -- both second kernels (resample, fill), every band count, 12 sprites at
  128x128 included."""
  monkeypatch.setenv('SWB_RUN_CAP', str(run_cap))
  monkeypatch.setenv('SWB_ARENA_UNITS', str(1 << 22))
  monkeypatch.setenv('SWB_BANDS', str(bands))
  monkeypatch.setenv('SWB_BAND_TASKS', '1')         # (a moving list shifts the band starts it has recorded -- and their copy in LDS)
  _run('cluster_s5', 96, 4, 5)
  _run('embodied_s12', 24, 3, 5)
  monkeypatch.setenv('SWB_NO_PAINT_IN_COVER', '1')
  _run('geom_160x48', 33, 3, 1)


@pytest.mark.gpu
def test_run_lists_are_trimmed_after_the_third_rendering_launch():
  """The hand-off lists start with room for any scene of convex sprites and are cut to 1.25 x the longest list written (+ the
  arena) by the engine's third rendering step; frames stay exact across the cut (compared with the oracle every step)."""
  from oracle import oracle
  from spriteworld_amd import engine
  for name, n_envs in (('embodied_s12', 256), ('cluster_s5', 1024)):
    cfg, pool, sample = workloads.build(name, n_envs, episodes_per_env=3, seed=4, anti_aliasing=5)
    eng, ora = engine.Engine(cfg, pool), oracle.Engine(cfg, pool)
    rng = np.random.default_rng(8)
    sizes = []
    for t in range(6):
      a = sample(rng)
      want = ora.step(a)
      eng.step(a)
      got = eng.outputs_host()
      assert not got['error'].any()
      assert np.array_equal(got['obs'], want['obs']), (name, t)
      v = eng.variant()
      sizes.append((v['run_cap'], v['run_list_bytes']))
    worst = max(4, cfg.max_sprites + 1) * cfg.anti_aliasing * cfg.image_w + 1
    assert sizes[0][0] == sizes[1][0] == worst and sizes[2][0] < worst // 2 and sizes[-1] == sizes[2], sizes
    assert sizes[2][1] < sizes[1][1] // 2, sizes
    eng.close()


@pytest.mark.parametrize('name,n_envs', [('cluster_s5', 64), ('tiny_s6', 48), ('wide_s4', 32), ('ragged_s16', 96)])
def test_fill_kernel_for_narrow_images(monkeypatch, name, n_envs):
  """anti_aliasing = 1: images of up to 64 columns are painted by the cover kernel itself; SWB_NO_PAINT_IN_COVER sends them
  through the run lists and the fill kernel, the path wider images always take (test_image_geometries covers those)."""
  monkeypatch.setenv('SWB_NO_PAINT_IN_COVER', '1')
  _run(name, n_envs, 3, 1)


@pytest.mark.gpu
@pytest.mark.parametrize('f32', [True, False], ids=['f32pos', 'f64pos'])
@pytest.mark.parametrize('name', __import__('tests._position_cases', fromlist=['CASES']).CASES)
def test_tasks_that_filter_on_position(name, f32):
  """Round 6: task filters / cluster distributions keyed on x, y -- the reference re-evaluates `contains(sprite.factors)` at
  every step (tasks.py:134-137, 196-205); the kernel looks every sprite's label up in the cell of the task's position grid it
  stands in.  HIP engine against the oracle (which tests/test_oracle_vs_reference.py pins against the unmodified reference on
  these very cases; tests/golden/position_*.npz are the reference's own outputs, checked in tests/test_golden.py)."""
  from oracle import oracle
  from spriteworld_amd import engine, lowering
  from tests import _position_cases as pc
  ns = pc.namespace_of_mirrors()
  task, aspace, rends, keep, max_len = pc.environment_parts(ns, name)
  n_envs = 96
  episodes = pc.episodes_of(ns, name, f32, n_episodes=3 * n_envs)
  cfg = lowering.lower_config(task, aspace, rends, keep, max_len, n_envs, pc.N_SPRITES, pos_is_f32=f32)
  pool = lowering.lower_episodes(episodes, task, rends, max_sprites=pc.N_SPRITES).assign_round_robin(n_envs, 3)
  ora, eng = oracle.Engine(cfg, pool), engine.Engine(cfg, pool)
  rng = np.random.default_rng(11)
  sticky = np.zeros(n_envs, np.uint8)
  flips, prev = 0, None
  for t in range(40):
    a = rng.uniform(0.0, 1.0, size=(n_envs, 4))
    st = ora.state()
    for i in range(0, n_envs, 2):                      # click ON a sprite in every second environment
      k = int(rng.integers(0, max(int(st['n_sprites'][i]), 1)))
      a[i, 0], a[i, 1] = st['x'][i, k], st['y'][i, k]
    want = ora.step(a)
    eng.step(a)
    got = eng.outputs_host()
    np.testing.assert_array_equal(got['step_type'], want['step_type'])
    np.testing.assert_array_equal(got['success'], want['success'])
    assert np.array_equal(np.isnan(got['reward']), np.isnan(want['reward']))
    ok = ~np.isnan(want['reward'])
    np.testing.assert_array_equal(got['reward'][ok].view(np.uint64), want['reward'][ok].view(np.uint64))
    sticky |= want['error']
    np.testing.assert_array_equal(got['error'], sticky)
    np.testing.assert_array_equal(got['obs'], want['obs'])
    if prev is not None:
      flips += int((want['reward'] != prev).sum())
    prev = want['reward']
  assert flips > 200
  eng.close()
