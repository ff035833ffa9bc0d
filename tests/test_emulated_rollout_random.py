"""swb_rollout_sampled on the emulated library (the kernel source compiled for the host, tests/emu) against the Python model of
tests/_rollout_random_model.py and the oracle -- the cases of tests/_rollout_random_cases.py, which
tests/test_gpu_rollout_random.py runs on the device.  TEST INFRASTRUCTURE: the emulator proves the arithmetic and control flow
of the kernel source, not its speed."""
import ctypes
import os
import subprocess
import sys

import pytest

from spriteworld_amd import _abi
from tests import _rollout_random_cases as cases
from tests import _util


def _emu(cfg, pool):
  from tests import _emu_engine
  return _emu_engine.EmuEngine(cfg, pool)


@pytest.fixture
def emulated_environment(monkeypatch):
  from spriteworld_amd import environment
  from tests import _emu_engine
  monkeypatch.setattr(environment._engine, 'Engine', _emu_engine.EmuTorchEngine)


@pytest.mark.parametrize('mode', sorted(cases.MODES))
@pytest.mark.parametrize('name', cases.PARITY)
def test_emulated_rollout_sampled_equals_model_and_oracle(name, mode):
  cases.parity_case(_emu, name, cases.MODES[mode])


@pytest.mark.parametrize('mode', sorted(cases.MODES))
@pytest.mark.parametrize('name', ('goal_s5', 'cluster_s5_f32a', 'embodied_s12', 'ragged_s64'))
def test_emulated_rollout_sampled_actions_replay_through_swb_rollout(name, mode):
  cases.replay_case(_emu, name, cases.MODES[mode])


@pytest.mark.parametrize('name', cases.CONTAINED)
def test_model_clicks_are_inside_the_chosen_sprites(name):
  cases.containment_case(name)


def test_emulated_rollout_sampled_stream_properties():
  cases.stream_case(_emu)


def test_emulated_rollout_sampled_leaves_the_handle_as_it_was():
  cases.handle_case(_emu)


def test_emulated_rollout_sampled_frames():
  cases.frames_case(_emu)


def test_emulated_rollout_sampled_refusals():
  cases.refusals_case(_emu)


def test_emulated_rollout_sampled_gives_up_at_the_cap():
  cases.cap_case(_emu)


def test_emulated_rollout_random_python_surface(emulated_environment):
  cases.surface_case()


def test_emulated_rollout_random_global_env_offset(emulated_environment):
  cases.offsets_case()


def test_rollout_sampled_outputs_struct_matches_the_header(tmp_path):
  """sizeof(swb_rollout_sampled_outputs) and the offset of its last field against the ctypes mirror, the way tests/test_abi.py
  checks the other structs."""
  src = tmp_path / 'sizes.c'
  src.write_text('''
#include <stdio.h>
#include <stddef.h>
#include "swb.h"
int main(void) {
  printf("%zu %zu %zu\\n", sizeof(swb_rollout_sampled_outputs), offsetof(swb_rollout_sampled_outputs, sprite),
         offsetof(swb_rollout_sampled_outputs, tries));
  return 0;
}''')
  exe = tmp_path / 'sizes'
  subprocess.check_call(['gcc', '-I', os.path.join(_util.ROOT, 'include'), '-o', str(exe), str(src)])
  out = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
  assert out == [ctypes.sizeof(_abi.SwbRolloutSampledOutputs), _abi.SwbRolloutSampledOutputs.sprite.offset,
                 _abi.SwbRolloutSampledOutputs.tries.offset]


def test_emulated_rollout_sampled_does_not_depend_on_lane_order():
  """One parity case with the lanes taking their turns in DESCENDING order between rendezvous (read once per process: a
  subprocess, as tests/test_emulated_rollout.py does for the plain kernel).  The draw writes the chosen sprite's path into the
  buffer the hit test reuses, and lanes 0..3 store the action other lanes drew alongside: neither may depend on which lane
  runs first."""
  env = dict(os.environ, SWB_EMU_LANE_ORDER='reverse', SWB_EMU_LDS_FILL='0x00')
  p = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-p', 'no:cacheprovider', '-k',
                      'equals_model_and_oracle and goal_s5 and sprite'], cwd=_util.ROOT, env=env, capture_output=True, text=True)
  assert p.returncode == 0 and ' passed' in p.stdout, p.stdout[-1500:]
