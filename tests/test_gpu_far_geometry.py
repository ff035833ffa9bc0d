"""Far, huge and non-finite sprites on the GPU: the cases of tests/_far_geometry_cases.py against the oracle at every step, on
every render path -- the crafted groups and the random scenes of a path in one batch."""
import pytest

from tests import _far_geometry_cases as cases

pytestmark = pytest.mark.gpu


def _gpu(cfg, pool):
  from spriteworld_amd import engine
  return engine.Engine(cfg, pool)


@pytest.mark.parametrize('path', cases.TUNED_PATHS + cases.LF_PATHS)
def test_inside_the_contract(monkeypatch, path):
  cases.family_a(_gpu, monkeypatch, path, 48)


@pytest.mark.parametrize('path', cases.LF_PATHS)
def test_inside_the_tuned_limit_on_the_large_frame_paths(monkeypatch, path):
  cases.family_a(_gpu, monkeypatch, path, 48, limit=cases.TUNED_LIMIT)


@pytest.mark.parametrize('path', cases.TUNED_PATHS)
def test_edge_of_the_limit(monkeypatch, path):
  cases.family_b(_gpu, monkeypatch, path, 32)


@pytest.mark.parametrize('path', cases.LF_EDGE_PATHS)
def test_edge_of_the_large_frame_limit(monkeypatch, path):
  cases.family_b(_gpu, monkeypatch, path, 32)


@pytest.mark.parametrize('path', cases.TUNED_PATHS + cases.LF_PATHS)
def test_far_beyond_and_non_finite_positions(monkeypatch, path):
  cases.family_c_positions(_gpu, monkeypatch, path, 40)


@pytest.mark.parametrize('keep_in_frame', (0, 1))
@pytest.mark.parametrize('path,name', cases.DRAG_SCENES)
def test_far_beyond_and_non_finite_drags(monkeypatch, path, name, keep_in_frame):
  cases.family_c_drags(_gpu, monkeypatch, path, 40, name, keep_in_frame=keep_in_frame)


def test_rollout_candidate_past_the_limit(monkeypatch):
  cases.rollout_case(_gpu, monkeypatch, n_envs=32)
