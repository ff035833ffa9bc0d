"""swb_rollout_trajectory and swb_rollout_step_frames on the emulated library (the kernel source compiled for the host, tests/emu)
against the oracle: the cases of tests/_rollout_trajectory_cases.py, which tests/test_gpu_rollout_trajectory.py runs on the
device.  TEST INFRASTRUCTURE: the emulator proves the arithmetic and control flow of the kernel source, not its speed."""
import ctypes
import os
import subprocess
import sys

import pytest

from spriteworld_amd import _abi
from tests import _rollout_trajectory_cases as cases
from tests import _util


def _emu(cfg, pool):
  from tests import _emu_engine
  return _emu_engine.EmuEngine(cfg, pool)


@pytest.fixture
def emulated_environment(monkeypatch):
  from spriteworld_amd import environment
  from tests import _emu_engine
  monkeypatch.setattr(environment._engine, 'Engine', _emu_engine.EmuEngine)


@pytest.mark.parametrize('name', cases.PARITY)
def test_emulated_rollout_trajectory_scores_and_states_equal_oracle(name):
  cases.parity_case(_emu, name)


@pytest.mark.parametrize('route', sorted(cases.ROUTES))
def test_emulated_rollout_step_frames_equal_oracle(monkeypatch, route):
  cases.route_case(_emu, monkeypatch, route)


def test_emulated_rollout_step_frames_picked_candidates():
  cases.picked_case(_emu)


def test_emulated_rollout_trajectory_leaves_the_handle_as_it_was():
  cases.handle_case(_emu)


@pytest.mark.parametrize('which', cases.EDGES)
def test_emulated_rollout_trajectory_edges(which):
  cases.edge_case(_emu, which)


def test_emulated_rollout_trajectory_refusals():
  cases.refusals_case(_emu)


def test_emulated_rollout_trajectory_refusals_after_device_sampling(emulated_environment):
  cases.refusals_after_device_sampling_case()


def test_emulated_rollout_trajectory_python_surface(emulated_environment):
  cases.surface_case()


def test_rollout_step_outputs_struct_matches_the_header(tmp_path):
  """sizeof(swb_rollout_step_outputs), the offset of its last field and SWB_ALL_STEPS against the ctypes mirror, the way
  tests/test_abi.py checks the other structs."""
  src = tmp_path / 'sizes.c'
  src.write_text('''
#include <stdio.h>
#include <stddef.h>
#include "swb.h"
int main(void) {
  printf("%zu %zu %d\\n", sizeof(swb_rollout_step_outputs), offsetof(swb_rollout_step_outputs, n_sprites), SWB_ALL_STEPS);
  return 0;
}''')
  exe = tmp_path / 'sizes'
  subprocess.check_call(['gcc', '-I', os.path.join(_util.ROOT, 'include'), '-o', str(exe), str(src)])
  out = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
  assert out == [ctypes.sizeof(_abi.SwbRolloutStepOutputs), _abi.SwbRolloutStepOutputs.n_sprites.offset, _abi.SWB_ALL_STEPS]


def test_emulated_rollout_trajectory_does_not_depend_on_lane_order():
  """One parity case with the lanes taking their turns in DESCENDING order between rendezvous (read once per process: a
  subprocess, as tests/test_emulated_rollout.py does for the plain kernel).  The keeping build stores slot k before the
  wave_sync() that ends the iteration, from registers, and the next iteration re-reads what lane 0 and lanes < S stored behind
  it: the kept states and the scores must not depend on which lane runs first."""
  env = dict(os.environ, SWB_EMU_LANE_ORDER='reverse', SWB_EMU_LDS_FILL='0x00')
  p = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-p', 'no:cacheprovider', '-k',
                      'scores_and_states_equal_oracle and goal_s5'], cwd=_util.ROOT, env=env, capture_output=True, text=True)
  assert p.returncode == 0 and ' passed' in p.stdout, p.stdout[-1500:]
