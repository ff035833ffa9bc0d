"""GPU parity: the HIP engine (through the C ABI) against the CPU oracle.

Both sides consume the same `SwbConfig`, the same pool arrays and the same
actions.  Bar (BASELINE.json north_star): sprite positions, step types,
discounts, success flags bit-exact; frames within +-1 LSB (we require +-0);
rewards bit-exact.  The bar is tests/_parity.py; the scenarios that are more than one
`_parity.run` call are in tests/_kernel_cases.py, shared with tests/test_emulated_kernel.py.
"""
import numpy as np
import pytest

from tests import _kernel_cases as cases
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
  """6000 environments: more than one round of cover waves."""
  monkeypatch.setenv('SWB_COVER_ORDER', '1')
  cases.cover_cost_order_case(_engine, name, n_envs, aa)


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
  cases.run_list_overflow_case(_engine, monkeypatch, [('cluster_s5', 5)], run_cap=24, n_envs=64, steps=1, quantifier=np.all)


@pytest.mark.gpu
@pytest.mark.parametrize('run_cap,bands', [(8, 1), (12, 4), (40, 2), (64, 8)])
def test_run_lists_that_outgrow_their_part_move_to_the_arena(monkeypatch, run_cap, bands):
  """12 sprites at 128x128 included."""
  cases.arena_move_case(_engine, monkeypatch, [('cluster_s5', 96, 4, 5), ('embodied_s12', 24, 3, 5), ('geom_160x48', 33, 3, 1)], run_cap, bands,
                        1 << 22, episodes_per_env=3, seed=0, rng_seed=100)


@pytest.mark.gpu
def test_run_lists_are_trimmed_after_the_third_rendering_launch():
  cases.trim_case(_engine, [('embodied_s12', 256, 5), ('cluster_s5', 1024, 5)], seed=4, rng_seed=8, steps=6, total_halves=True)


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
  cases.position_filter_case(_engine, name, f32, n_envs=96, min_flips=200)
