"""GPU: swb_rollout_guided (swb_rollout_guided_kernel<KEEP>: the rollout kernel drawing its candidates from a plan distribution)
against the Python model of tests/_rollout_guided_model.py and the CPU oracle -- the cases of tests/_rollout_guided_cases.py,
which tests/test_emulated_rollout_guided.py runs on the emulated library.  Actions, sprites, tries, rewards and positions bit
for bit, frames +-0; the live state and the caller's outputs untouched."""
import pytest

from tests import _rollout_guided_cases as cases

pytestmark = pytest.mark.gpu


def _gpu(cfg, pool):
  from spriteworld_amd import engine
  return engine.Engine(cfg, pool)


@pytest.mark.parametrize('kind', cases.PLANS)
@pytest.mark.parametrize('name', cases.PARITY)
def test_gpu_rollout_guided_equals_model_and_oracle(name, kind):
  cases.parity_case(_gpu, name, kind)


@pytest.mark.parametrize('name', ('goal_s5', 'cluster_s5_f32a', 'embodied_s12', 'ragged_s64'))
def test_gpu_rollout_guided_actions_replay_through_swb_rollout(name):
  cases.replay_case(_gpu, name)


def test_gpu_rollout_guided_stream_properties():
  cases.stream_case(_gpu)


def test_gpu_rollout_guided_leaves_the_handle_as_it_was():
  cases.handle_case(_gpu)


def test_gpu_rollout_guided_frames():
  cases.frames_case(_gpu)


def test_gpu_rollout_guided_refusals():
  cases.refusals_case(_gpu)


def test_gpu_rollout_guided_python_surface():
  cases.surface_case()


def test_gpu_rollout_guided_global_env_offset():
  cases.offsets_case()


def test_gpu_rollout_guided_environment_groups():
  cases.groups_case()
