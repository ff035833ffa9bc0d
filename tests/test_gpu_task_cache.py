"""The task cache on the GPU: the scripts of tests/_task_cache_cases.py against the oracle at every step, with swb_task_stats held
to the oracle-driven model of the records.  64 environments each."""
import pytest

from tests import _task_cache_cases as cases

pytestmark = pytest.mark.gpu

N = 64


def _gpu(cfg, pool):
  from spriteworld_amd import engine
  return engine.Engine(cfg, pool)


def test_still_and_hits(monkeypatch):
  cases.still_and_hits(_gpu, monkeypatch, N)


def test_mixed(monkeypatch):
  cases.mixed(_gpu, monkeypatch, N)


def test_clipped_move(monkeypatch):
  cases.clipped_move(_gpu, monkeypatch, N)


def test_velocities(monkeypatch):
  cases.velocities(_gpu, monkeypatch, N)


@pytest.mark.parametrize('which', cases.BETWEEN)
def test_call_between(monkeypatch, which):
  cases.call_between(_gpu, monkeypatch, N, which)


def test_reset_envs_between(monkeypatch):
  cases.reset_envs_between(_gpu, monkeypatch, N)


def test_snapshots(monkeypatch):
  cases.snapshots(_gpu, monkeypatch, N)


def test_masked(monkeypatch):
  cases.masked(_gpu, monkeypatch, N)


def test_errors(monkeypatch):
  cases.errors(_gpu, monkeypatch, N)


@pytest.mark.parametrize('which', cases.PATHS)
def test_paths(monkeypatch, which):
  cases.path(_gpu, monkeypatch, N, which)


def test_switch_off(monkeypatch):
  cases.switch_off(_gpu, monkeypatch, N)
