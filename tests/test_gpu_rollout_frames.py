"""GPU: swb_rollout_frames (the render path of the handle on a rollout's scratch state, and swb_rollout_pick_kernel) against the
CPU oracle -- the cases of tests/_rollout_frames_cases.py, which tests/test_emulated_rollout_frames.py runs on the emulated
library.  Frames +-0; the live state, the caller's outputs and the pool untouched."""
import pytest

from tests import _rollout_frames_cases as cases

pytestmark = pytest.mark.gpu


def _gpu(cfg, pool):
  from spriteworld_amd import engine
  return engine.Engine(cfg, pool)


@pytest.mark.parametrize('route', sorted(cases.ROUTES))
def test_gpu_rollout_frames_equal_oracle(monkeypatch, route):
  cases.route_case(_gpu, monkeypatch, route)


@pytest.mark.parametrize('n_steps', (2, 3))
def test_gpu_rollout_frames_where_the_rollout_ends(n_steps):
  cases.ends_case(_gpu, n_steps)


@pytest.mark.parametrize('which', sorted(cases.HANDLE))
def test_gpu_rollout_frames_leave_the_handle_as_it_was(which):
  cases.handle_case(_gpu, which)


def test_gpu_rollout_frames_picked_candidates():
  cases.picked_case(_gpu)


@pytest.mark.parametrize('which', cases.EDGES)
def test_gpu_rollout_frames_edges(which):
  cases.edge_case(_gpu, which)


def test_gpu_rollout_frames_refusals():
  cases.refusals_case(_gpu)


def test_gpu_rollout_frames_refusals_after_device_sampling():
  cases.refusals_after_device_sampling_case()


def test_gpu_rollout_frames_python_surface():
  cases.surface_case()
