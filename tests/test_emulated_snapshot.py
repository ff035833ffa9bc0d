"""Snapshots (swb_save_state, swb_load_state, swb_copy_pool) on the emulated library (the kernel source compiled for the host,
tests/emu) against the oracle: the cases of tests/_snapshot_cases.py, which tests/test_gpu_snapshot.py runs on the device.
TEST INFRASTRUCTURE: the emulator proves the arithmetic and control flow of the kernel source, not its speed."""
import ctypes
import os
import subprocess
import sys

import pytest

from spriteworld_amd import _abi
from tests import _snapshot_cases as cases
from tests import _util


def _emu(cfg, pool):
  from tests import _emu_engine
  return _emu_engine.EmuEngine(cfg, pool)


@pytest.fixture
def emulated_environment(monkeypatch):
  from spriteworld_amd import environment
  from tests import _emu_engine
  monkeypatch.setattr(environment._engine, 'Engine', _emu_engine.EmuEngine)


@pytest.mark.parametrize('name,aa,expect', cases.ROUND_TRIP, ids=['%s-aa%d' % (n, a) for n, a, _ in cases.ROUND_TRIP])
def test_emulated_snapshot_round_trip(name, aa, expect):
  cases.round_trip_case(_emu, name, aa, expect)


def test_emulated_snapshot_permuted_and_partial_load():
  cases.permuted_case(_emu)


def test_emulated_snapshot_does_not_depend_on_lane_order():
  """The permuted load with the lanes taking their turns in DESCENDING order between rendezvous (read once per process: a
  subprocess, as tests/test_emulated_rollout.py does)."""
  env = dict(os.environ, SWB_EMU_LANE_ORDER='reverse', SWB_EMU_LDS_FILL='0x00')
  p = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-p', 'no:cacheprovider', '-k',
                      'permuted_and_partial_load'], cwd=_util.ROOT, env=env, capture_output=True, text=True)
  assert p.returncode == 0 and ' passed' in p.stdout, p.stdout[-1500:]


def test_emulated_snapshot_load_drops_only_the_loaded_lists(monkeypatch):
  cases.stale_list_case(_emu, monkeypatch)


def test_emulated_snapshot_rollout_end_states():
  cases.rollout_end_case(_emu)


def test_emulated_snapshot_fork(emulated_environment):
  cases.fork_case()


def test_emulated_snapshot_copy_pool_between_unlike_handles():
  cases.unlike_handles_case(_emu)


def test_emulated_snapshot_pool_identity_and_host_round_trip():
  cases.pool_identity_case(_emu)


def test_emulated_snapshot_is_refused_after_a_pool_refresh(emulated_environment):
  cases.refresh_refuses_case()


def test_emulated_snapshot_guards():
  cases.guards_case(_emu)


def test_snapshot_struct_matches_the_header(tmp_path):
  """sizeof(swb_snapshot), the offsets of two fields and the source enum against the ctypes mirror, the way tests/test_abi.py
  checks the other structs."""
  src = tmp_path / 'sizes.c'
  src.write_text('''
#include <stdio.h>
#include <stddef.h>
#include "swb.h"
int main(void) {
  printf("%zu %zu %zu %d %d\\n", sizeof(swb_snapshot), offsetof(swb_snapshot, pool_base), offsetof(swb_snapshot, reset_next),
         (int)SWB_STATE_LIVE, (int)SWB_STATE_ROLLOUT_END);
  return 0;
}''')
  exe = tmp_path / 'sizes'
  subprocess.check_call(['gcc', '-I', os.path.join(_util.ROOT, 'include'), '-o', str(exe), str(src)])
  out = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
  assert out == [ctypes.sizeof(_abi.SwbSnapshot), _abi.SwbSnapshot.pool_base.offset, _abi.SwbSnapshot.reset_next.offset,
                 _abi.STATE_LIVE, _abi.STATE_ROLLOUT_END]
