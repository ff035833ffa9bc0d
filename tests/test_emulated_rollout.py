"""swb_rollout on the emulated library (the kernel source compiled for the host, tests/emu) against the oracle: the cases of
tests/_rollout_cases.py, which tests/test_gpu_rollout.py runs on the device.  TEST INFRASTRUCTURE: the emulator proves the
arithmetic and control flow of the kernel source, not its speed."""
import ctypes
import os
import subprocess
import sys

import pytest

from spriteworld_amd import _abi
from tests import _rollout_cases as cases
from tests import _util


def _emu(cfg, pool):
  from tests import _emu_engine
  return _emu_engine.EmuEngine(cfg, pool)


@pytest.mark.parametrize('name', cases.PARITY)
def test_emulated_rollout_equals_oracle(name):
  cases.parity_case(_emu, name)


def test_emulated_rollout_leaves_the_live_state_untouched():
  cases.live_state_case(_emu)


@pytest.mark.parametrize('which', cases.EDGES)
def test_emulated_rollout_edges(which):
  cases.edge_case(_emu, which)


def test_emulated_rollout_refusals():
  cases.refusals_case(_emu)


def test_emulated_rollout_python_surface(monkeypatch):
  """BatchedEnvironment.rollout, the Rollout tuple and episode_return() over the emulated library.  The engine patched in is
  engine.Engine over that library, so the argument checks, dtype conversion and allocation of Engine.rollout run here too
  (with the permuted, non-contiguous view BatchedEnvironment hands it), as in tests/test_gpu_rollout.py on the device."""
  import numpy as np
  from spriteworld_amd import environment
  from tests import _emu_engine
  monkeypatch.setattr(environment._engine, 'Engine', _emu_engine.EmuEngine)
  cases.surface_case()
  cfg, pool, _ = cases.built('goal_s5')
  eng = _emu(cfg, pool)
  for shape in ((cases.K, cases.N_ENVS, cases.M), (cases.K, cases.N_ENVS + 1, cases.M, 4), (cases.K, cases.N_ENVS, cases.M, 2)):
    with pytest.raises(ValueError, match='rollout actions must be'):
      eng.rollout(np.zeros(shape))
  eng.close()


def test_rollout_outputs_struct_matches_the_header(tmp_path):
  """sizeof(swb_rollout_outputs) and the offset of its last field against the ctypes mirror, the way tests/test_abi.py checks
  the other structs."""
  src = tmp_path / 'sizes.c'
  src.write_text('''
#include <stdio.h>
#include <stddef.h>
#include "swb.h"
int main(void) {
  printf("%zu %zu %zu\\n", sizeof(swb_rollout_outputs), offsetof(swb_rollout_outputs, error), offsetof(swb_rollout_outputs, n_sprites));
  return 0;
}''')
  exe = tmp_path / 'sizes'
  subprocess.check_call(['gcc', '-I', os.path.join(_util.ROOT, 'include'), '-o', str(exe), str(src)])
  out = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
  assert out == [ctypes.sizeof(_abi.SwbRolloutOutputs), _abi.SwbRolloutOutputs.error.offset, _abi.SwbRolloutOutputs.n_sprites.offset]


def test_emulated_rollout_does_not_depend_on_lane_order():
  """One parity case with the lanes taking their turns in DESCENDING order between rendezvous (read once per process: a
  subprocess, as tests/test_emulated_kernel.py does).  Between two iterations every lane re-reads what lane 0 and lanes < S
  stored: without the wave_sync() there, the high lanes would load the next step's state before it is written."""
  env = dict(os.environ, SWB_EMU_LANE_ORDER='reverse', SWB_EMU_LDS_FILL='0x00')
  p = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-p', 'no:cacheprovider', '-k',
                      'equals_oracle and goal_s5'], cwd=_util.ROOT, env=env, capture_output=True, text=True)
  assert p.returncode == 0 and ' passed' in p.stdout, p.stdout[-1500:]
