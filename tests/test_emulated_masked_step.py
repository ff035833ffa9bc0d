"""Masked steps and partial resets on the emulated kernel (tests/emu, CPU): the scripts of tests/_masked_step_cases.py against the
oracle at every step.  A handful of environments each."""
import pytest

from tests import _masked_step_cases as cases


def _emu(cfg, pool):
  from tests import _emu_engine
  return _emu_engine.EmuEngine(cfg, pool)


@pytest.mark.parametrize('which', sorted(cases.WORKLOADS))
def test_against_the_oracle(monkeypatch, which):
  cases.against_the_oracle(_emu, monkeypatch, which, 5 if which in ('embodied_s12', 'cluster_s40') else 7)


def test_inactive_waves_take_the_cheap_path(monkeypatch):
  assert cases.cheap_path(_emu, monkeypatch, 7, masked=True) == cases.cheap_path(_emu, monkeypatch, 7, masked=False)


@pytest.mark.parametrize('which', ['goal_s5', 'cluster_s5_aa1', 'cluster_s40', 'goal_s5_large_frames'])
def test_nothing_of_an_inactive_environment_is_written(monkeypatch, which):
  cases.nothing_written(_emu, monkeypatch, which, 5 if which == 'cluster_s40' else 9)


def test_no_mask_all_ones_and_swb_step_are_the_same(monkeypatch):
  cases.three_ways_to_step_everything(_emu, monkeypatch, 7)


def test_reset_envs(monkeypatch):
  from tests import _emu_engine
  cases.reset_envs(_emu, monkeypatch, 9, _emu_engine.EmuError)


def test_with_load_state(monkeypatch):
  cases.with_load_state(_emu, monkeypatch, 6)


def test_with_set_positions(monkeypatch):
  cases.with_set_positions(_emu, monkeypatch, 5)


def test_with_sprite_setter(monkeypatch):
  cases.with_sprite_setter(_emu, monkeypatch, 5)
