"""Task sets on the GPU: the scripts of tests/_task_sets_cases.py against one oracle per set at every step."""
import pytest

from tests import _task_sets_cases as cases

pytestmark = pytest.mark.gpu


def _gpu(cfg, pool):
  from spriteworld_amd import engine
  return engine.Engine(cfg, pool)


def _error():
  from spriteworld_amd import _lib
  return _lib.SwbError


@pytest.mark.parametrize('which', sorted(cases.SCENES))
def test_against_the_oracles(monkeypatch, which):
  cases.against_the_oracles(_gpu, monkeypatch, which, gpu=True)


def test_with_a_live_setter(monkeypatch):
  cases.with_setter(_gpu, monkeypatch, gpu=True)


def test_with_an_active_mask(monkeypatch):
  cases.with_mask(_gpu, monkeypatch, gpu=True)


def test_null_steps_reuse_task_records(monkeypatch):
  cases.null_steps_reuse_records(_gpu, monkeypatch, gpu=True)


def test_one_set_equal_to_the_config_is_the_handle_without_sets(monkeypatch):
  cases.one_set_equals_no_sets(_gpu, monkeypatch, gpu=True)


def test_reassignment_in_the_middle_of_episodes(monkeypatch):
  cases.reassignment(_gpu, monkeypatch, gpu=True, emu_error=_error())


def test_snapshot_loaded_into_other_environments(monkeypatch):
  cases.snapshots(_gpu, monkeypatch, gpu=True)


def test_fork(monkeypatch):
  cases.fork(_gpu, monkeypatch, gpu=True)


def test_refusals(monkeypatch):
  cases.refusals(_gpu, monkeypatch, _error())
