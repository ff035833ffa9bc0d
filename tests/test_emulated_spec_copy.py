"""The speculative copies of the cover launch on the emulated kernel (tests/emu, CPU): tests/_spec_copy_cases.py under both
placements of the copy workgroups.  The emulator runs workgroups in index order, so `first` is the interleaving in which every
copy workgroup reads the word of the previous launch and `behind` the one in which it reads the word of this launch: the counts
of swb_spec_copy_stats are exact."""
import pytest

from tests import _masked_step_cases as masked
from tests import _spec_copy_cases as cases


def _emu(cfg, pool):
  from tests import _emu_engine
  return _emu_engine.EmuEngine(cfg, pool)


@pytest.mark.parametrize('order', cases.ORDERS)
def test_scripted_two_buffers(monkeypatch, order):
  cases.scripted(_emu, monkeypatch, 8, order, True)


@pytest.mark.parametrize('order', cases.ORDERS)
def test_thirteen_environments(monkeypatch, order):
  cases.scripted(_emu, monkeypatch, 13, order, True, steps=10)


@pytest.mark.parametrize('order', cases.ORDERS)
def test_stale_cache(monkeypatch, order):
  cases.stale_cache(_emu, monkeypatch, 8, order, True)


@pytest.mark.parametrize('order', cases.ORDERS)
@pytest.mark.parametrize('which', cases.GEOMETRIES)
def test_geometries(monkeypatch, which, order):
  cases.geometry(_emu, monkeypatch, 16 if which == 'band_tasks_8' else 8, which, order, True)


@pytest.mark.parametrize('order', cases.ORDERS)
@pytest.mark.parametrize('which', ('never', 'always'))
def test_split_bands(monkeypatch, which, order):
  cases.split_bands(_emu, monkeypatch, 8, which, order)


@pytest.mark.parametrize('order', cases.ORDERS)
@pytest.mark.parametrize('which', cases.BETWEEN)
def test_calls_between(monkeypatch, which, order):
  cases.call_between(_emu, monkeypatch, 8, which, order)


@pytest.mark.parametrize('order', cases.ORDERS)
def test_state_view(monkeypatch, order):
  cases.state_view(_emu, monkeypatch, 8, order, True)


@pytest.mark.parametrize('order', cases.ORDERS)
def test_load_state_between(monkeypatch, order):
  cases.load_state_between(_emu, monkeypatch, 12, order, True)


@pytest.mark.parametrize('order', cases.ORDERS)
def test_masked_steps_at_every_word(monkeypatch, order):
  cases.masked_words(_emu, monkeypatch, 8, order, True)


@pytest.mark.parametrize('order', cases.ORDERS)
def test_reset_envs_and_masked_steps(monkeypatch, order):
  from tests import _emu_engine
  cases.under(monkeypatch, order)
  masked.reset_envs(_emu, monkeypatch, 9, _emu_engine.EmuError)


@pytest.mark.parametrize('order', cases.ORDERS)
@pytest.mark.parametrize('which', ('no_frame_cache', 'anti_aliasing_1'))
def test_absent(monkeypatch, which, order):
  cases.absent(_emu, monkeypatch, 8, which, order)
