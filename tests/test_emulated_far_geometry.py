"""Far, huge and non-finite sprites on the emulated kernel (tests/emu, CPU): the cases of tests/_far_geometry_cases.py against the
oracle at every step, on every render path, a few environments each (one crafted group per test, so that every test stays
small); the emulator's out-of-bounds counter must stay at zero throughout."""
import pytest

from tests import _far_geometry_cases as cases


def _emu(cfg, pool):
  from tests import _emu_engine
  return _emu_engine.EmuEngine(cfg, pool)


def _n(path, tuned, large):
  """Environments: the large-frame and many-sprite paths are the slow ones to emulate."""
  return large if path in cases.LF_PATHS else tuned


@pytest.mark.parametrize('group', cases.GROUPS)
@pytest.mark.parametrize('path', cases.TUNED_PATHS + cases.LF_PATHS)
def test_inside_the_contract(monkeypatch, path, group):
  cases.family_a(_emu, monkeypatch, path, cases.GROUP_ENVS[group] + 2, groups=(group,), random_floor=False)


@pytest.mark.parametrize('path', cases.TUNED_PATHS + cases.LF_PATHS)
def test_random_far_scenes(monkeypatch, path):
  cases.family_a(_emu, monkeypatch, path, _n(path, 12, 6), groups=(), limit=cases.TUNED_LIMIT)


@pytest.mark.parametrize('path', cases.LF_PATHS)
def test_random_far_scenes_at_the_large_frame_limit(monkeypatch, path):
  cases.family_a(_emu, monkeypatch, path, 6, groups=())


@pytest.mark.parametrize('path', cases.TUNED_PATHS)
def test_edge_of_the_limit(monkeypatch, path):
  cases.family_b(_emu, monkeypatch, path, 10)


@pytest.mark.parametrize('path', cases.LF_EDGE_PATHS)
def test_edge_of_the_large_frame_limit(monkeypatch, path):
  cases.family_b(_emu, monkeypatch, path, 10)


@pytest.mark.parametrize('path', cases.TUNED_PATHS + cases.LF_PATHS)
def test_far_beyond_and_non_finite_positions(monkeypatch, path):
  cases.family_c_positions(_emu, monkeypatch, path, _n(path, 20, 8))


@pytest.mark.parametrize('keep_in_frame', (0, 1))
@pytest.mark.parametrize('path,name', cases.DRAG_SCENES)
def test_far_beyond_and_non_finite_drags(monkeypatch, path, name, keep_in_frame):
  cases.family_c_drags(_emu, monkeypatch, path, _n(path, 20, 10), name, keep_in_frame=keep_in_frame)


def test_rollout_candidate_past_the_limit(monkeypatch):
  cases.rollout_case(_emu, monkeypatch, n_envs=6)
