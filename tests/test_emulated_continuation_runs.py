"""Continuation runs of the hand-off lists, on the emulated kernel (tests/emu, CPU): the scenes of tests/_continuation_cases.py
against the oracle -- positions, rewards, step types bit for bit, frames +-0 -- and, through the emulator's event counters, the
proof that the square scene does take the path."""
import ctypes

import pytest

from tests import _continuation_cases as cases


def _emu(cfg, pool):
  from tests import _emu_engine
  return _emu_engine.EmuEngine(cfg, pool)


@pytest.mark.parametrize('n_envs', [8, 16, 64])
def test_square_crosses_the_forced_ends(n_envs):
  """One row pattern across about 19 forced run ends, at the batch sizes whose band counts differ."""
  cases.run(_emu, 'square', n_envs, 2 if n_envs > 16 else 3, 5)


@pytest.mark.parametrize('bands', [2, 4, 8])
def test_a_band_begins_inside_the_chain(monkeypatch, bands):
  """The first run of a band is never a continuation: the wave that starts there has no row yet.  Every band is a task of its
  own, so each such wave does start at its band's first unit."""
  monkeypatch.setenv('SWB_BANDS', str(bands))
  monkeypatch.setenv('SWB_BAND_TASKS', '1')
  cases.run(_emu, 'square', 5, 3, 5)
  cases.run(_emu, 'stack5', 3, 2, 5)


@pytest.mark.parametrize('case,n_envs,aa', [('square_wide', 4, 5), ('square_bg', 4, 5), ('stack5', 4, 5), ('square', 3, 2), ('stack5', 3, 3),
                                            ('square_wide', 3, 4)])
def test_column_groups_backgrounds_and_many_spans(case, n_envs, aa):
  cases.run(_emu, case, n_envs, 3, aa)


@pytest.mark.parametrize('run_cap,bands', [(8, 1), (12, 4)])
def test_lists_that_move_to_the_arena_at_every_batch(monkeypatch, run_cap, bands):
  monkeypatch.setenv('SWB_RUN_CAP', str(run_cap))
  monkeypatch.setenv('SWB_ARENA_UNITS', str(1 << 20))
  monkeypatch.setenv('SWB_BANDS', str(bands))
  monkeypatch.setenv('SWB_BAND_TASKS', '1')
  for case in ('square', 'square_wide', 'stack5'):
    cases.run(_emu, case, 3, 2, 5)


def test_trimmed_lists():
  """The engine cuts the lists to 1.25 x the longest one after its third rendering step: the steps before and after the cut."""
  for case in ('square', 'stack5'):
    cases.run(_emu, case, 4, 5, 5)


@pytest.mark.parametrize('no_paint', [False, True], ids=['paint', 'fill'])
@pytest.mark.parametrize('case', cases.CASES)
def test_anti_aliasing_1_never_meets_a_continuation(monkeypatch, case, no_paint):
  """anti_aliasing = 1 has no forced ends; its two paths (the cover kernel paints / run lists + fill kernel) see lists as before."""
  if no_paint:
    monkeypatch.setenv('SWB_NO_PAINT_IN_COVER', '1')
  cases.run(_emu, case, 3, 2, 1)


def _counting_engine(monkeypatch):
  """_emu_engine over the build of the emulator that counts events, continuation runs among them (tests/_emu_counters.py: a
  library of its own beside the one the other tests share)."""
  from tests import _emu_counters, _emu_engine
  counting = _emu_counters.load()
  monkeypatch.setattr(_emu_engine, '_lib', None)
  monkeypatch.setattr(_emu_engine, 'build_emu', counting)
  lib = _emu_engine.lib()
  lib.emu_stats.restype = ctypes.c_long
  return lib, counting._COUNTERS


def test_the_square_scene_does_produce_continuations(monkeypatch):
  """96 canvas rows of one span, a forced end every 5 rows: all but two or three of the square's about 20 runs continue the run
  before them; at anti_aliasing = 1 none does.  The frames are compared as everywhere."""
  lib, counters = _counting_engine(monkeypatch)
  monkeypatch.setenv('SWB_BANDS', '1')                       # (bands overlap: their waves would count some runs twice)
  n_envs, steps = 4, 2
  for aa, case in ((5, 'square'), (5, 'square_bg'), (1, 'square')):
    if aa == 1:
      monkeypatch.setenv('SWB_NO_PAINT_IN_COVER', '1')       # (through the run lists and the fill kernel)
    lib.emu_stats(0, 1)
    cases.run(_emu, case, n_envs, steps, aa)
    per_frame = {c: lib.emu_stats(i, 0) / float(n_envs * steps) for i, c in enumerate(counters)}
    runs, cont = per_frame['p3_row_runs'], per_frame['p3_continuation_runs']
    if aa == 1:
      assert cont == 0, per_frame
    elif case == 'square':
      # rows [y0, y0 + 96) of the 320-row canvas, one span each, meet 19 or 20 forced ends; the row that begins the second
      # batch of 64 canvas rows heads a chain of its own, as the first row does
      assert 17 <= cont <= 20 and runs <= cont + 3, per_frame
      assert per_frame['p3_continuation_spans'] == cont, per_frame
    else:
      # all 320 rows are listed, in 64 windows of 5 rows; heads: the first row of each of the 5 batches, the square's first
      # row and the first one below it
      assert runs >= 64 and cont >= runs - 8, per_frame
      assert per_frame['p3_continuation_spans'] == cont, per_frame       # (a continuation of rows without spans counts one)
