"""The snapshot calls of the host side (spriteworld_amd/csrc/swb.hip: swb_pool_id, swb_save_state, swb_load_state, swb_copy_pool)
under AddressSanitizer, leak detection on.

tests/host_snapshot_lifecycle.cc -- a program of its own, no Python in the process -- creates two handles, copies the pool of
each into the other, saves and loads states between them (the end states of a rollout included), makes swb_copy_pool fail
half-way before and after the destination has a pool, and destroys the handles in either order; here it is compiled together
with the sources the emulator build leaves under tests/emu/_build/src/csrc (the host code as shipped, the kernels rewritten for
x86) and tests/emu/emu_runtime.cc, and run, in the manner of tests/test_host_lifecycle.py.  Every pool array a copy makes must
be freed exactly once, whichever handle ends up owning it: any sanitizer report fails.

CPU only: sanitizer builds are not run where a GPU is visible.
"""
import os
import subprocess

import pytest

from tests.conftest import _has_gpu
from tests.emu import build_emu

HERE = os.path.dirname(os.path.abspath(__file__))
UNITS = ('swb.hip', 'swb_wide.hip')


def test_host_snapshot_lifecycle_is_clean_under_address_sanitizer():
  if _has_gpu():
    pytest.skip('a GPU is visible: sanitizer builds run on CPU-only machines')
  build_emu.build()
  src_dir = os.path.join(build_emu.OUT_DIR, 'src', 'csrc')
  out_dir = os.path.join(build_emu.OUT_DIR, 'host_snapshot_lifecycle_asan')
  os.makedirs(out_dir, exist_ok=True)
  flags = build_emu.FLAGS + ['-I', os.path.join(build_emu.OUT_DIR, 'include'), '-fsanitize=address', '-fno-omit-frame-pointer']
  sources = [os.path.join(src_dir, u) for u in UNITS] + [os.path.join(build_emu.HERE, 'emu_runtime.cc'),
                                                         os.path.join(HERE, 'host_snapshot_lifecycle.cc')]
  objs, procs = [], []
  for path in sources:                                  # the four units compile in parallel
    obj = os.path.join(out_dir, os.path.basename(path) + '.o')
    procs.append(subprocess.Popen([build_emu.CLANG] + flags + ['-c', '-o', obj, path]))
    objs.append(obj)
  assert [p.wait() for p in procs] == [0] * len(procs), 'sanitizer build failed'
  exe = os.path.join(out_dir, 'host_snapshot_lifecycle')
  subprocess.check_call([build_emu.CLANG, '-fsanitize=address', '-o', exe] + objs + ['-lm'])
  env = {k: v for k, v in os.environ.items() if k not in ('LD_PRELOAD', 'ASAN_OPTIONS', 'LSAN_OPTIONS') and not k.startswith('SWB_')}
  env['ASAN_OPTIONS'] = 'detect_leaks=1'
  run = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600)
  print(run.stdout + run.stderr)
  assert run.returncode == 0, run.stderr[-4000:]
  assert 'Sanitizer' not in run.stderr, run.stderr[-4000:]
  assert run.stderr.rstrip().endswith('ok'), run.stderr[-4000:]
