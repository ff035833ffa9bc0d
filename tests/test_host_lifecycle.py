"""The host side of the engine (spriteworld_amd/csrc/swb.hip) under AddressSanitizer, leak detection on.

tests/host_lifecycle.cc -- a program of its own, no Python in the process -- takes six kinds of handle through creation,
uploads, steps with and without an observation, trimming and restoring the run lists, a sprite setter, two rollouts that
regrow their scratch and three refusals that return after part of the set-up; here it is compiled together with the sources
the emulator build leaves under tests/emu/_build/src/csrc (the host code as shipped, the kernels rewritten for x86) and
tests/emu/emu_runtime.cc, and run.  Every device buffer a handle makes must be freed exactly once: any sanitizer report fails.

CPU only: sanitizer builds are not run where a GPU is visible.

Measured: about 80 s to compile on 8 cores, 2.5 s to run (profiles/r10_host_refactor.md).
"""
import os
import subprocess

import pytest

from tests.conftest import _has_gpu
from tests.emu import build_emu

HERE = os.path.dirname(os.path.abspath(__file__))
UNITS = ('swb.hip', 'swb_wide.hip')


def test_host_lifecycle_is_clean_under_address_sanitizer():
  if _has_gpu():
    pytest.skip('a GPU is visible: sanitizer builds run on CPU-only machines')
  build_emu.build()
  src_dir = os.path.join(build_emu.OUT_DIR, 'src', 'csrc')
  out_dir = os.path.join(build_emu.OUT_DIR, 'host_lifecycle_asan')
  os.makedirs(out_dir, exist_ok=True)
  flags = build_emu.FLAGS + ['-I', os.path.join(build_emu.OUT_DIR, 'include'), '-fsanitize=address', '-fno-omit-frame-pointer']
  sources = [os.path.join(src_dir, u) for u in UNITS] + [os.path.join(build_emu.HERE, 'emu_runtime.cc'), os.path.join(HERE, 'host_lifecycle.cc')]
  objs, procs = [], []
  for path in sources:                                  # the four units compile in parallel
    obj = os.path.join(out_dir, os.path.basename(path) + '.o')
    procs.append(subprocess.Popen([build_emu.CLANG] + flags + ['-c', '-o', obj, path]))
    objs.append(obj)
  assert [p.wait() for p in procs] == [0] * len(procs), 'sanitizer build failed'
  exe = os.path.join(out_dir, 'host_lifecycle')
  subprocess.check_call([build_emu.CLANG, '-fsanitize=address', '-o', exe] + objs + ['-lm'])
  env = {k: v for k, v in os.environ.items() if k not in ('LD_PRELOAD', 'ASAN_OPTIONS', 'LSAN_OPTIONS') and not k.startswith('SWB_')}
  env['ASAN_OPTIONS'] = 'detect_leaks=1'
  run = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600)
  print(run.stdout + run.stderr)
  assert run.returncode == 0, run.stderr[-4000:]
  assert 'Sanitizer' not in run.stderr, run.stderr[-4000:]
  assert run.stderr.rstrip().endswith('ok'), run.stderr[-4000:]
