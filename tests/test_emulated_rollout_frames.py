"""swb_rollout_frames on the emulated library (the kernel source compiled for the host, tests/emu) against the oracle: the cases
of tests/_rollout_frames_cases.py, which tests/test_gpu_rollout_frames.py runs on the device.  TEST INFRASTRUCTURE: the emulator
proves the arithmetic and control flow of the kernel source, not its speed."""
import pytest

from tests import _rollout_frames_cases as cases


def _emu(cfg, pool):
  from tests import _emu_engine
  return _emu_engine.EmuEngine(cfg, pool)


@pytest.fixture
def emulated_environment(monkeypatch):
  from spriteworld_amd import environment
  from tests import _emu_engine
  monkeypatch.setattr(environment._engine, 'Engine', _emu_engine.EmuEngine)


@pytest.mark.parametrize('route', sorted(cases.ROUTES))
def test_emulated_rollout_frames_equal_oracle(monkeypatch, route):
  cases.route_case(_emu, monkeypatch, route)


@pytest.mark.parametrize('n_steps', (2, 3))
def test_emulated_rollout_frames_where_the_rollout_ends(n_steps):
  cases.ends_case(_emu, n_steps)


@pytest.mark.parametrize('which', sorted(cases.HANDLE))
def test_emulated_rollout_frames_leave_the_handle_as_it_was(which):
  cases.handle_case(_emu, which)


def test_emulated_rollout_frames_picked_candidates():
  cases.picked_case(_emu)


@pytest.mark.parametrize('which', cases.EDGES)
def test_emulated_rollout_frames_edges(which):
  cases.edge_case(_emu, which)


def test_emulated_rollout_frames_refusals():
  cases.refusals_case(_emu)


def test_emulated_rollout_frames_refusals_after_device_sampling(emulated_environment):
  cases.refusals_after_device_sampling_case()


def test_emulated_rollout_frames_python_surface(emulated_environment):
  cases.surface_case()
