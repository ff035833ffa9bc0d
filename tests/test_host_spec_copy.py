"""The host side of the speculative copies of the cover launch (spriteworld_amd/csrc/swb.hip: the condition, the grown grid, the
switch SWB_SPEC_COPY and its refusal, the seventh counter) under AddressSanitizer (leak detection on) and under
UndefinedBehaviorSanitizer.

tests/host_spec_copy.cc -- a program of its own, no Python in the process -- walks create -> steps -> swb_set_positions -> steps
-> trim -> steps -> render -> destroy under `first` and under `behind` and holds swb_frame_stats and swb_spec_copy_stats at every
stage; here it is compiled together with the sources the emulator build leaves under tests/emu/_build/src/csrc (the host code as
shipped, the kernels rewritten for x86) and tests/emu/emu_runtime.cc, and run.

CPU only: sanitizer builds are not run where a GPU is visible.
"""
import os
import subprocess

import pytest

from tests.conftest import _has_gpu
from tests.emu import build_emu

HERE = os.path.dirname(os.path.abspath(__file__))
UNITS = ('swb.hip', 'swb_wide.hip')
# One program per sanitizer (see tests/test_host_kept_lists.py).
SANITIZERS = ('address', 'undefined')


def test_host_side_of_speculative_copies_is_clean_under_sanitizers():
  if _has_gpu():
    pytest.skip('a GPU is visible: sanitizer builds run on CPU-only machines')
  build_emu.build()
  src_dir = os.path.join(build_emu.OUT_DIR, 'src', 'csrc')
  sources = [os.path.join(src_dir, u) for u in UNITS] + [os.path.join(build_emu.HERE, 'emu_runtime.cc'), os.path.join(HERE, 'host_spec_copy.cc')]
  objs, procs = {}, []
  for san in SANITIZERS:
    out_dir = os.path.join(build_emu.OUT_DIR, 'host_spec_copy_' + san)
    os.makedirs(out_dir, exist_ok=True)
    flags = build_emu.FLAGS + ['-I', os.path.join(build_emu.OUT_DIR, 'include'), '-fsanitize=' + san, '-fno-omit-frame-pointer']
    if san == 'undefined':
      # (alignment: the emulator's allocator aligns to 16 bytes what hipMalloc aligns to 256, and the emulated resample kernel
      # loads 32-byte vectors from such a table -- a property of the emulation, not of the host code under test)
      flags += ['-fno-sanitize=alignment', '-fno-sanitize-recover=undefined']
    for path in sources:
      obj = os.path.join(out_dir, os.path.basename(path) + '.o')
      procs.append(subprocess.Popen([build_emu.CLANG] + flags + ['-c', '-o', obj, path]))
      objs.setdefault(san, []).append(obj)
  assert [p.wait() for p in procs] == [0] * len(procs), 'sanitizer build failed'
  env = {k: v for k, v in os.environ.items() if k not in ('LD_PRELOAD', 'ASAN_OPTIONS', 'LSAN_OPTIONS', 'UBSAN_OPTIONS') and not k.startswith('SWB_')}
  env['ASAN_OPTIONS'] = 'detect_leaks=1'
  env['UBSAN_OPTIONS'] = 'print_stacktrace=1'
  for san in SANITIZERS:
    exe = os.path.join(build_emu.OUT_DIR, 'host_spec_copy_' + san, 'host_spec_copy')
    subprocess.check_call([build_emu.CLANG, '-fsanitize=' + san, '-o', exe] + objs[san] + ['-lm'])
    run = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600)
    print(run.stdout + run.stderr)
    assert run.returncode == 0, (san, run.stderr[-4000:])
    assert 'Sanitizer' not in run.stderr and 'runtime error' not in run.stderr, (san, run.stderr[-4000:])
    assert run.stderr.rstrip().endswith('ok'), (san, run.stderr[-4000:])
