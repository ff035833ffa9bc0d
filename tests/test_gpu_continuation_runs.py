"""Continuation runs of the hand-off lists on the GPU: the scenes of tests/_continuation_cases.py against the oracle -- positions,
rewards, step types bit for bit, frames +-0.  (tests/test_emulated_continuation_runs.py proves, through the emulator's counters,
that these scenes take the path.)"""
import pytest

from tests import _continuation_cases as cases

pytestmark = pytest.mark.gpu


def _gpu(cfg, pool):
  from spriteworld_amd import engine
  return engine.Engine(cfg, pool)


@pytest.mark.parametrize('n_envs', [8, 16, 64])
def test_square_crosses_the_forced_ends(n_envs):
  """One row pattern across about 19 forced run ends."""
  cases.run(_gpu, 'square', n_envs, 3, 5)


@pytest.mark.parametrize('bands,band_tasks', [(1, 0), (2, 1), (4, 1), (8, 0), (8, 1)])
def test_a_band_begins_inside_the_chain(monkeypatch, bands, band_tasks):
  """The first run of a band is never a continuation: the wave that starts there has no row yet -- every band count, bands as
  tasks of their own and as a grid dimension."""
  monkeypatch.setenv('SWB_BANDS', str(bands))
  monkeypatch.setenv('SWB_BAND_TASKS', str(band_tasks))
  cases.run(_gpu, 'square', 64, 3, 5)
  cases.run(_gpu, 'stack5', 16, 2, 5)


@pytest.mark.parametrize('case,n_envs,aa', [('square_wide', 16, 5), ('square_bg', 16, 5), ('stack5', 64, 5), ('square', 8, 2), ('stack5', 8, 3),
                                            ('square_wide', 8, 4)])
def test_column_groups_backgrounds_and_many_spans(case, n_envs, aa):
  cases.run(_gpu, case, n_envs, 3, aa)


@pytest.mark.parametrize('run_cap,bands', [(8, 1), (12, 4), (40, 2)])
def test_lists_that_move_to_the_arena_at_every_batch(monkeypatch, run_cap, bands):
  monkeypatch.setenv('SWB_RUN_CAP', str(run_cap))
  monkeypatch.setenv('SWB_ARENA_UNITS', str(1 << 22))
  monkeypatch.setenv('SWB_BANDS', str(bands))
  monkeypatch.setenv('SWB_BAND_TASKS', '1')
  for case in ('square', 'square_wide', 'stack5', 'square_bg'):
    cases.run(_gpu, case, 16, 2, 5)


def test_trimmed_lists():
  """The engine cuts the lists to 1.25 x the longest one after its third rendering step: the steps before and after the cut."""
  for case in ('square', 'stack5', 'square_wide'):
    cases.run(_gpu, case, 32, 5, 5)


@pytest.mark.parametrize('no_paint', [False, True], ids=['paint', 'fill'])
@pytest.mark.parametrize('case', cases.CASES)
def test_anti_aliasing_1_never_meets_a_continuation(monkeypatch, case, no_paint):
  """anti_aliasing = 1 has no forced ends; its two paths (the cover kernel paints / run lists + fill kernel) see lists as before."""
  if no_paint:
    monkeypatch.setenv('SWB_NO_PAINT_IN_COVER', '1')
  cases.run(_gpu, case, 16, 2, 1)
