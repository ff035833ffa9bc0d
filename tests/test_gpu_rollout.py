"""GPU: swb_rollout (swb_rollout_fork_kernel + swb_rollout_kernel) against the CPU oracle -- the cases of
tests/_rollout_cases.py, which tests/test_emulated_rollout.py runs on the emulated library.  Rewards, discounts and positions
bit-exact, step types, success flags and sprite counts equal; the live state untouched."""
import pytest

from tests import _rollout_cases as cases

pytestmark = pytest.mark.gpu


def _gpu(cfg, pool):
  from spriteworld_amd import engine
  return engine.Engine(cfg, pool)


@pytest.mark.parametrize('name', cases.PARITY)
def test_gpu_rollout_equals_oracle(name):
  cases.parity_case(_gpu, name)


def test_gpu_rollout_leaves_the_live_state_untouched():
  cases.live_state_case(_gpu)


@pytest.mark.parametrize('which', cases.EDGES)
def test_gpu_rollout_edges(which):
  cases.edge_case(_gpu, which)


def test_gpu_rollout_refusals():
  cases.refusals_case(_gpu)


def test_gpu_rollout_python_surface():
  cases.surface_case()
