"""GPU: Clustering rewards at every cluster count and degeneracy, error flags included, against the CPU oracle
(tests/_clustering_cases.py): the tuned state phase, swb_ms_state_kernel at 64 sprites and -- under SWB_MANY_SPRITES=1 -- at
16, swb_rollout_kernel and swb_evaluate, both position dtypes.  256 environments per scene, one geometry each, three steps."""
import pytest

from tests import _clustering_cases as cases

pytestmark = pytest.mark.gpu

N_ENVS = 256
DTYPES = [pytest.param(True, id='float32'), pytest.param(False, id='float64')]


def _gpu(cfg, pool):
  from spriteworld_amd import engine
  return engine.Engine(cfg, pool)


@pytest.mark.parametrize('f32', DTYPES)
@pytest.mark.parametrize('path', cases.PATHS)
def test_gpu_clustering_steps(path, f32):
  cases.step_case(_gpu, path, f32, N_ENVS)


@pytest.mark.parametrize('f32', DTYPES)
@pytest.mark.parametrize('path', ('tuned', 'many_s64'))
def test_gpu_clustering_rollout(path, f32):
  cases.rollout_case(_gpu, path, f32, N_ENVS)


@pytest.mark.parametrize('f32', DTYPES)
@pytest.mark.parametrize('path', cases.PATHS)
def test_gpu_clustering_evaluate(path, f32):
  cases.evaluate_case(_gpu, path, f32, N_ENVS)


@pytest.mark.parametrize('i', range(len(cases.META)))
def test_gpu_clustering_meta_aggregated(i):
  """2, 7 and 8 sub-tasks x sum, mean, max, min; the state paths and position dtypes in turn."""
  n_sub, aggregator = cases.META[i]
  cases.meta_case(_gpu, cases.PATHS[i % 3], i % 2 == 0, N_ENVS, n_sub, aggregator)
