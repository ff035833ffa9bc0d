"""swb_rollout_guided on the emulated library (the kernel source compiled for the host, tests/emu) against the Python model of
tests/_rollout_guided_model.py and the oracle -- the cases of tests/_rollout_guided_cases.py, which
tests/test_gpu_rollout_guided.py runs on the device -- and, on the model alone, the statistics of its motion draw.
TEST INFRASTRUCTURE: the emulator proves the arithmetic and control flow of the kernel source, not its speed."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from spriteworld_amd import _abi
from tests import _rollout_guided_cases as cases
from tests import _rollout_guided_model as model
from tests import _util


def _emu(cfg, pool):
  from tests import _emu_engine
  return _emu_engine.EmuEngine(cfg, pool)


@pytest.fixture
def emulated_environment(monkeypatch):
  from spriteworld_amd import environment
  from tests import _emu_engine
  monkeypatch.setattr(environment._engine, 'Engine', _emu_engine.EmuTorchEngine)


@pytest.mark.parametrize('kind', cases.PLANS)
@pytest.mark.parametrize('name', cases.PARITY)
def test_emulated_rollout_guided_equals_model_and_oracle(name, kind):
  cases.parity_case(_emu, name, kind)


@pytest.mark.parametrize('name', ('goal_s5', 'cluster_s5_f32a', 'embodied_s12', 'ragged_s64'))
def test_emulated_rollout_guided_actions_replay_through_swb_rollout(name):
  cases.replay_case(_emu, name)


def test_emulated_rollout_guided_stream_properties():
  cases.stream_case(_emu)


def test_emulated_rollout_guided_leaves_the_handle_as_it_was():
  cases.handle_case(_emu)


def test_emulated_rollout_guided_frames():
  cases.frames_case(_emu)


def test_emulated_rollout_guided_refusals():
  cases.refusals_case(_emu)


def test_emulated_rollout_guided_python_surface(emulated_environment):
  cases.surface_case()


def test_emulated_rollout_guided_global_env_offset(emulated_environment):
  cases.offsets_case()


def test_model_choice_rule():
  """Rule 3 on hand-made rows: zero weights are skipped at both ends and in the middle, u_c * total that rounds up to the total
  takes the last sprite WITH weight, rows without a positive finite total fall back."""
  cdf = np.cumsum([0.0, 2.0, 0.0, 1.0, 0.0])
  assert model.choose(0.0, 5, cdf, 5) == (1, model.WEIGHTED)
  assert model.choose(0.6666, 5, cdf, 5) == (1, model.WEIGHTED) and model.choose(0.6667, 5, cdf, 5) == (3, model.WEIGHTED)
  assert model.choose(1.0 - 2.0 ** -53, 5, cdf, 5) == (3, model.WEIGHTED)
  assert model.choose(0.999, 3, np.cumsum([0.0, 1e-300, 0.0]), 3) == (1, model.WEIGHTED)
  # t rounds up to the total (a subnormal total: for a normal one u_c * total stays below it): the first sprite that reaches it
  tiny = np.array([0.0, 5e-324, 5e-324])
  assert 0.75 * 5e-324 == 5e-324 and model.choose(0.75, 3, tiny, 3) == (1, model.WEIGHTED_ROUNDED_UP)
  assert model.choose(0.5, 4, cdf, 5) == (1, model.WEIGHTED)                  # n < W: the first n running sums
  assert model.choose(0.99, 2, cdf, 5) == (1, model.WEIGHTED)
  assert model.choose(0.99, 1, cdf, 5) == (0, model.FALLBACK_TOTAL)           # (the only sprite there has weight 0)
  assert model.choose(0.99, 7, cdf, 5) == (3, model.WEIGHTED)                 # W < n: sprites 5, 6 are never chosen
  for bad in ([0.0, 0.0, 0.0], [1.0, np.nan, np.nan], [1.0, np.inf, np.inf], [-1.0, -2.0, -3.0]):
    assert model.choose(0.75, 3, np.array(bad), 3) == (2, model.FALLBACK_TOTAL), bad
  assert model.choose(0.75, 3, None, 3) == (2, model.FALLBACK_NO_CDF)
  assert model.choose(1.0 - 2.0 ** -53, 3, None, 3) == (2, model.FALLBACK_NO_CDF)    # ((int)(u_c * n) == n is clamped)


def test_model_motion_draw_is_standardised():
  """10^5 values of z (Irwin-Hall, n = 4, centred and scaled) from the model's own stream: the mean within 5 / sqrt(10^5) =
  0.016 of 0 (five standard errors of a unit-variance mean); the variance within 0.02 of 1 -- the standard error of a sample
  variance is sqrt((kurtosis - 1) / n) = sqrt(1.7 / 10^5) = 0.0041 for kurtosis 2.7, five of them; every value within
  +-2 sqrt(3)."""
  n = 100000
  rng = model.CandidateStream(cases.SEED, 3, 1)
  z = np.array([model.irwin_hall_z(rng) for _ in range(n)])
  assert abs(z.mean()) <= 5.0 / math.sqrt(n), z.mean()
  assert abs(z.var() - 1.0) <= 0.02, z.var()
  assert (np.abs(z) <= 2.0 * math.sqrt(3.0)).all(), np.abs(z).max()
  assert np.abs(z).max() > 2.5                            # (a bell with tails, not a clipped uniform)


def test_rollout_plan_struct_matches_the_header(tmp_path):
  """sizeof(swb_rollout_plan) and the offsets of its fields against the ctypes mirror, the way tests/test_abi.py checks the
  other structs."""
  src = tmp_path / 'sizes.c'
  src.write_text('''
#include <stdio.h>
#include <stddef.h>
#include "swb.h"
int main(void) {
  printf("%zu %zu %zu %zu\\n", sizeof(swb_rollout_plan), offsetof(swb_rollout_plan, width), offsetof(swb_rollout_plan, motion_mean),
         offsetof(swb_rollout_plan, motion_std));
  return 0;
}''')
  exe = tmp_path / 'sizes'
  subprocess.check_call(['gcc', '-I', os.path.join(_util.ROOT, 'include'), '-o', str(exe), str(src)])
  out = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
  assert out == [ctypes.sizeof(_abi.SwbRolloutPlan), _abi.SwbRolloutPlan.width.offset, _abi.SwbRolloutPlan.motion_mean.offset,
                 _abi.SwbRolloutPlan.motion_std.offset]
