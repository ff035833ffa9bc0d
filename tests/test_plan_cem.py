"""BatchedEnvironment.plan_cem on the emulated library (tests/emu): the cases of tests/_plan_cem_cases.py, which
tests/test_gpu_plan_cem.py runs on the device, and that the planner never waits for the device.  TEST INFRASTRUCTURE."""
import numpy as np
import pytest
import torch

from tests import _plan_cem_cases as cases


@pytest.fixture(autouse=True)
def emulated_environment(monkeypatch):
  from spriteworld_amd import environment
  from tests import _emu_engine
  monkeypatch.setattr(environment._engine, 'Engine', _emu_engine.EmuTorchEngine)


@pytest.mark.parametrize('name', cases.NAMES)
def test_emulated_plan_cem_returns_what_its_plan_replays_to(name):
  cases.plan_case(name)


@pytest.mark.parametrize('name', cases.NAMES)
def test_emulated_plan_cem_refit_equals_numpy(name):
  cases.refit_case(name)


@pytest.mark.parametrize('name', cases.NAMES)
def test_emulated_plan_cem_warm_start(name):
  cases.warm_start_case(name)


@pytest.mark.parametrize('name', cases.NAMES)
def test_emulated_plan_cem_does_not_synchronise(name, monkeypatch):
  """No host synchronisation inside plan_cem.  The emulated runtime counts neither launches nor synchronisations (its
  hipStreamSynchronize is an inline no-op), so the two things the Python layers could do are watched instead: the engine's own
  `_sync()` (what `state()`, `outputs_host()` and the readers call before they copy) is counted, and every way a tensor's value
  reaches Python (item, tolist, cpu, numpy, bool, int, float, index) raises.  The GPU suite runs the same call under torch's
  synchronisation debug mode."""
  from tests import _emu_engine
  env = cases.started(name)
  env.plan_cem(cases.M, cases.K, iterations=1)            # (the scratch grows on the first rollout: the one blocking case)
  syncs = []
  monkeypatch.setattr(_emu_engine.EmuEngine, '_sync', lambda self: syncs.append(1))
  with cases.no_host_reads(monkeypatch):
    plan = env.plan_cem(cases.M, cases.K, iterations=cases.I)
  assert not syncs, len(syncs)
  assert (np.diff(plan.best_per_iteration.numpy(), axis=1) >= 0).all()
  with cases.no_host_reads(monkeypatch):                  # (the watch itself works)
    with pytest.raises(AssertionError):
      plan.episode_return[0].item()
  env.close()


def test_cem_refit_std_bound_is_what_this_cpu_measures():
  """How STD_BOUND was obtained, kept as a test: torch's population deviation against numpy's over uniform triples and over
  triples within 1e-9 of each other, float64."""
  rng = np.random.default_rng(0)
  worst = 0.0
  for spread in (1.0, 1e-9):
    base = rng.uniform(0.0, 1.0, (200000, 1))
    a = np.clip(base + spread * rng.uniform(-0.5, 0.5, (200000, 3)), 0.0, 1.0) if spread < 1.0 else rng.uniform(0.0, 1.0, (200000, 3))
    got = torch.as_tensor(a).std(dim=1, unbiased=False).numpy()
    worst = max(worst, float(np.abs(got - a.std(axis=1)).max()))
  print('largest |torch std - numpy std| = %.3g' % worst)
  assert worst <= cases.STD_BOUND, worst
