"""GPU: swb_rollout_sampled (swb_rollout_kernel<KEEP, SAMPLE>: the rollout kernel drawing its candidates' actions, uniform or as
clicks on sprites) against the Python model of tests/_rollout_random_model.py and the CPU oracle -- the cases of
tests/_rollout_random_cases.py, which tests/test_emulated_rollout_random.py runs on the emulated library.  Actions, sprites,
tries, rewards and positions bit for bit, frames +-0; the live state and the caller's outputs untouched."""
import pytest

from tests import _rollout_random_cases as cases

pytestmark = pytest.mark.gpu


def _gpu(cfg, pool):
  from spriteworld_amd import engine
  return engine.Engine(cfg, pool)


@pytest.mark.parametrize('mode', sorted(cases.MODES))
@pytest.mark.parametrize('name', cases.PARITY)
def test_gpu_rollout_sampled_equals_model_and_oracle(name, mode):
  cases.parity_case(_gpu, name, cases.MODES[mode])


@pytest.mark.parametrize('mode', sorted(cases.MODES))
@pytest.mark.parametrize('name', ('goal_s5', 'cluster_s5_f32a', 'embodied_s12', 'ragged_s64'))
def test_gpu_rollout_sampled_actions_replay_through_swb_rollout(name, mode):
  cases.replay_case(_gpu, name, cases.MODES[mode])


def test_gpu_rollout_sampled_stream_properties():
  cases.stream_case(_gpu)


def test_gpu_rollout_sampled_leaves_the_handle_as_it_was():
  cases.handle_case(_gpu)


def test_gpu_rollout_sampled_frames():
  cases.frames_case(_gpu)


def test_gpu_rollout_sampled_refusals():
  cases.refusals_case(_gpu)


def test_gpu_rollout_random_python_surface():
  cases.surface_case()


def test_gpu_rollout_random_global_env_offset():
  cases.offsets_case()


def test_gpu_rollout_random_environment_groups():
  cases.groups_case()
