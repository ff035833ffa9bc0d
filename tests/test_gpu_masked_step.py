"""Masked steps and partial resets on the GPU: the scripts of tests/_masked_step_cases.py against the oracle at every step."""
import pytest

from tests import _masked_step_cases as cases

pytestmark = pytest.mark.gpu


def _gpu(cfg, pool):
  from spriteworld_amd import engine
  return engine.Engine(cfg, pool)


@pytest.mark.parametrize('which', sorted(cases.WORKLOADS))
def test_against_the_oracle(monkeypatch, which):
  cases.against_the_oracle(_gpu, monkeypatch, which, 33 if which in ('embodied_s12', 'cluster_s40') else 67)


def test_inactive_waves_take_the_cheap_path(monkeypatch):
  assert cases.cheap_path(_gpu, monkeypatch, 67, masked=True) == cases.cheap_path(_gpu, monkeypatch, 67, masked=False)


@pytest.mark.parametrize('which', ['goal_s5', 'cluster_s5_aa1', 'cluster_s40', 'goal_s5_large_frames'])
def test_nothing_of_an_inactive_environment_is_written(monkeypatch, which):
  cases.nothing_written(_gpu, monkeypatch, which, 33 if which == 'cluster_s40' else 65)


def test_no_mask_all_ones_and_swb_step_are_the_same(monkeypatch):
  cases.three_ways_to_step_everything(_gpu, monkeypatch, 67)


def test_reset_envs(monkeypatch):
  from spriteworld_amd import _lib
  cases.reset_envs(_gpu, monkeypatch, 66, _lib.SwbError)


def test_with_load_state(monkeypatch):
  cases.with_load_state(_gpu, monkeypatch, 33)


def test_with_set_positions(monkeypatch):
  cases.with_set_positions(_gpu, monkeypatch, 33)


def test_with_sprite_setter(monkeypatch):
  cases.with_sprite_setter(_gpu, monkeypatch, 33)
