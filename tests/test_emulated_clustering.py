"""Clustering rewards at every cluster count and degeneracy, error flags included, on the emulated library against the oracle
(tests/_clustering_cases.py): the tuned state phase, swb_ms_state_kernel at 64 sprites and -- under SWB_MANY_SPRITES=1 -- at
16, swb_rollout_kernel and swb_evaluate, both position dtypes.  One geometry per environment; the batch is the smallest that
holds one of each class.  TEST INFRASTRUCTURE: the emulator proves the arithmetic and control flow of the kernel source --
tests/test_gpu_clustering.py runs the real thing."""
import pytest

from tests import _clustering_cases as cases

DTYPES = [pytest.param(True, id='float32'), pytest.param(False, id='float64')]


def _emu(cfg, pool):
  from tests import _emu_engine
  return _emu_engine.EmuEngine(cfg, pool)


@pytest.mark.parametrize('f32', DTYPES)
@pytest.mark.parametrize('path', cases.PATHS)
def test_emulated_clustering_steps(path, f32):
  """(The float64 batches carry the recorded scenes whose score is exactly 0.0 through the regular path.)"""
  cases.step_case(_emu, path, f32, cases.min_envs(path, f32))


@pytest.mark.parametrize('f32', DTYPES)
@pytest.mark.parametrize('path', ('tuned', 'many_s64'))
def test_emulated_clustering_rollout(path, f32):
  cases.rollout_case(_emu, path, f32, cases.min_envs(path, f32))


@pytest.mark.parametrize('f32', DTYPES)
@pytest.mark.parametrize('path', cases.PATHS)
def test_emulated_clustering_evaluate(path, f32):
  cases.evaluate_case(_emu, path, f32, cases.min_envs(path, f32))


@pytest.mark.parametrize('i', range(len(cases.META)))
def test_emulated_clustering_meta_aggregated(i):
  """2, 7 and 8 sub-tasks x sum, mean, max, min; the state paths and position dtypes in turn."""
  n_sub, aggregator = cases.META[i]
  path, f32 = cases.PATHS[i % 3], i % 2 == 0
  cases.meta_case(_emu, path, f32, cases.min_envs(path, f32), n_sub, aggregator)
