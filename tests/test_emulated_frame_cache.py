"""The frame cache on the emulated kernel (tests/emu, CPU): the scripts of tests/_frame_cache_cases.py against the oracle at every
step, with swb_frame_stats and swb_list_stats held to what a model of the header word implies.  A handful of environments each."""
import pytest

from tests import _frame_cache_cases as cases


def _emu(cfg, pool):
  from tests import _emu_engine
  return _emu_engine.EmuEngine(cfg, pool)


def test_never_hit(monkeypatch):
  cases.never_hit(_emu, monkeypatch, 4)


def test_hit_every_step(monkeypatch):
  cases.hit_every_step(_emu, monkeypatch, 3)


def test_scripted(monkeypatch):
  cases.scripted(_emu, monkeypatch, 7)


def test_episode_ends(monkeypatch):
  cases.episode_ends(_emu, monkeypatch, 3)


def test_caller_scribbles(monkeypatch):
  cases.scripted(_emu, monkeypatch, 5, what='caller_scribbles', scribble=True)


def test_alternating_buffers(monkeypatch):
  cases.alternating_buffers(_emu, monkeypatch, 5)


@pytest.mark.parametrize('which', cases.BETWEEN)
def test_calls_between(monkeypatch, which):
  cases.call_between(_emu, monkeypatch, 4, which)


@pytest.mark.parametrize('which', cases.GEOMETRIES)
def test_geometries(monkeypatch, which):
  cases.geometry(_emu, monkeypatch, 16 if which == 'band_tasks_8' else 5, which)


def test_switches(monkeypatch):
  cases.switches(_emu, monkeypatch, 5)


@pytest.mark.parametrize('paint', (False, True))
def test_anti_aliasing_1(monkeypatch, paint):
  cases.anti_aliasing_1(_emu, monkeypatch, 4, paint)
