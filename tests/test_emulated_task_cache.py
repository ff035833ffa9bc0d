"""The task cache on the emulated kernels (tests/emu, CPU): the scripts of tests/_task_cache_cases.py against the oracle at every
step, with swb_task_stats held to the oracle-driven model of the records.  Eight environments each."""
import pytest

from tests import _task_cache_cases as cases

N = 8


def _emu(cfg, pool):
  from tests import _emu_engine
  return _emu_engine.EmuEngine(cfg, pool)


def test_still_and_hits(monkeypatch):
  cases.still_and_hits(_emu, monkeypatch, N)


def test_mixed(monkeypatch):
  cases.mixed(_emu, monkeypatch, N)


def test_clipped_move(monkeypatch):
  cases.clipped_move(_emu, monkeypatch, N)


def test_velocities(monkeypatch):
  cases.velocities(_emu, monkeypatch, N)


@pytest.mark.parametrize('which', cases.BETWEEN)
def test_call_between(monkeypatch, which):
  cases.call_between(_emu, monkeypatch, N, which)


def test_reset_envs_between(monkeypatch):
  cases.reset_envs_between(_emu, monkeypatch, N)


def test_snapshots(monkeypatch):
  cases.snapshots(_emu, monkeypatch, N)


def test_masked(monkeypatch):
  cases.masked(_emu, monkeypatch, N)


def test_errors(monkeypatch):
  cases.errors(_emu, monkeypatch, N)


@pytest.mark.parametrize('which', cases.PATHS)
def test_paths(monkeypatch, which):
  cases.path(_emu, monkeypatch, N, which)


def test_switch_off(monkeypatch):
  cases.switch_off(_emu, monkeypatch, N)
