"""GPU: BatchedEnvironment.plan_cem -- the cases of tests/_plan_cem_cases.py, which tests/test_plan_cem.py runs on the emulated
library -- and the planner under torch's synchronisation debug mode."""
import numpy as np
import pytest
import torch

from tests import _plan_cem_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', cases.NAMES)
def test_gpu_plan_cem_returns_what_its_plan_replays_to(name):
  cases.plan_case(name)


@pytest.mark.parametrize('name', cases.NAMES)
def test_gpu_plan_cem_refit_equals_numpy(name):
  cases.refit_case(name)


@pytest.mark.parametrize('name', cases.NAMES)
def test_gpu_plan_cem_warm_start(name):
  cases.warm_start_case(name)


@pytest.mark.parametrize('name', cases.NAMES)
def test_gpu_plan_cem_does_not_synchronise(name, monkeypatch):
  """plan_cem under torch.cuda.set_sync_debug_mode('error'): any torch operation that waits for the device raises; and no value
  of a tensor reaches Python (tests/_plan_cem_cases.no_host_reads)."""
  env = cases.started(name)
  env.plan_cem(cases.M, cases.K, iterations=1)            # (the scratch grows on the first rollout: the one blocking case)
  torch.cuda.synchronize()
  before = torch.cuda.get_sync_debug_mode()
  torch.cuda.set_sync_debug_mode('error')
  try:
    with cases.no_host_reads(monkeypatch):
      plan = env.plan_cem(cases.M, cases.K, iterations=cases.I)
  finally:
    torch.cuda.set_sync_debug_mode(before)
  assert (np.diff(plan.best_per_iteration.cpu().numpy(), axis=1) >= 0).all()
  env.close()
