"""GPU: swb_rollout_trajectory (swb_rollout_kernel<KEEP>) and swb_rollout_step_frames (the render path of the handle on a slot of
the trajectory block, and swb_rollout_pick_steps_kernel) against the CPU oracle -- the cases of
tests/_rollout_trajectory_cases.py, which tests/test_emulated_rollout_trajectory.py runs on the emulated library.  Positions and
rewards bit for bit, frames +-0; the live state, the caller's outputs and the pool untouched."""
import pytest

from tests import _rollout_trajectory_cases as cases

pytestmark = pytest.mark.gpu


def _gpu(cfg, pool):
  from spriteworld_amd import engine
  return engine.Engine(cfg, pool)


@pytest.mark.parametrize('name', cases.PARITY)
def test_gpu_rollout_trajectory_scores_and_states_equal_oracle(name):
  cases.parity_case(_gpu, name)


@pytest.mark.parametrize('route', sorted(cases.ROUTES))
def test_gpu_rollout_step_frames_equal_oracle(monkeypatch, route):
  cases.route_case(_gpu, monkeypatch, route)


def test_gpu_rollout_step_frames_picked_candidates():
  cases.picked_case(_gpu)


def test_gpu_rollout_trajectory_leaves_the_handle_as_it_was():
  cases.handle_case(_gpu)


@pytest.mark.parametrize('which', cases.EDGES)
def test_gpu_rollout_trajectory_edges(which):
  cases.edge_case(_gpu, which)


def test_gpu_rollout_trajectory_refusals():
  cases.refusals_case(_gpu)


def test_gpu_rollout_trajectory_refusals_after_device_sampling():
  cases.refusals_after_device_sampling_case()


def test_gpu_rollout_trajectory_python_surface():
  cases.surface_case()
