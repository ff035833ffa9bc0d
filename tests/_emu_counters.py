"""The counting build of the emulator (tests/emu/build_emu.py under SWB_EMU_STATS) with two more event counters, for the
continuation runs of the hand-off lists (TEST INFRASTRUCTURE ONLY; used by tests/test_emulated_continuation_runs.py and
tools/emu_stats.py):

  p3_continuation_runs   runs the resample kernel walks that continue the run before them (SWB_RUN_CONTINUES)
  p3_continuation_spans  the spans whose horizontal pass those runs skip (a continuation's spans field repeats its head's, so
                         p3_spans counts what it counted before there were continuations)

build_emu.py decides where it builds, and whether it counts, when it is imported: `load()` executes a second copy of the module
with SWB_EMU_STATS set, appends the counters and their hook to that copy and gives it a build directory of its own, so the
library the other tests share and the plain counting build stay what they are.
"""
import hashlib
import importlib.util
import os

from tests.emu import build_emu

EXTRA = ('p3_continuation_runs', 'p3_continuation_spans')
_ANCHOR = '      while ((int)(rec.x & 0xffffu) <= next_end) {'
_module = None


def load():
  """The counting copy of build_emu (its `_COUNTERS` end with EXTRA; `build()` returns the library)."""
  global _module
  if _module is not None:
    return _module
  spec = importlib.util.spec_from_file_location('tests.emu.build_emu_continuation_counters', build_emu.__file__)
  mod = importlib.util.module_from_spec(spec)
  before = os.environ.get('SWB_EMU_STATS')
  os.environ['SWB_EMU_STATS'] = '1'
  try:
    spec.loader.exec_module(mod)
    first = len(mod._COUNTERS)
    mod._COUNTERS = tuple(mod._COUNTERS) + EXTRA
    mod.OUT_DIR = os.path.join(mod.OUT_DIR, 'continuation')
    mod.LIB = os.path.join(mod.OUT_DIR, 'libswb_emu.so')
    instrument, source_hash = mod._instrument, mod.source_hash

    def _instrument(text):
      text = instrument(text)
      assert text.count(_ANCHOR) == 1, _ANCHOR
      return text.replace(_ANCHOR, _ANCHOR + ' if (rec.x & SWB_RUN_CONTINUES) { emu_count(%d, 1); emu_count(%d, (long)(rec.x >> 24)); }'
                          % (first, first + 1))

    def _source_hash():
      with open(os.path.abspath(__file__), 'rb') as f:
        return hashlib.sha256(source_hash().encode() + f.read()).hexdigest()

    mod._instrument, mod.source_hash = _instrument, _source_hash
    mod.build()                 # (reads SWB_EMU_STATS while it rewrites the sources)
  finally:
    if before is None:
      del os.environ['SWB_EMU_STATS']
    else:
      os.environ['SWB_EMU_STATS'] = before
  _module = mod
  return mod
