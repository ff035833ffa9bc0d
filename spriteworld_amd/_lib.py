"""Loader of the HIP engine (spriteworld_amd/csrc/libswb.so, C ABI of include/swb.h).

There is no CPU fallback: if the library is missing or no gfx950 device is
usable, the engine raises.  Build with `python __graft_entry__.py` (or
`spriteworld_amd.build.build()`).
"""
import ctypes as C
import os

from spriteworld_amd import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# SWB_LIBRARY: an alternative build of the same ABI (experiments, integrators' own install path)
LIB_PATH = os.environ.get('SWB_LIBRARY') or os.path.join(_HERE, 'csrc', 'libswb.so')

# Every symbol include/swb.h declares (tests check the header against it, and that the library exports them all).
EXPORTS = tuple(_abi.PROTOTYPES)

_lib = None


class SwbError(RuntimeError):
  pass


def load():
  """Returns the ctypes handle of libswb.so (raises SwbError when it is not built)."""
  global _lib
  if _lib is not None:
    return _lib
  if not os.path.exists(LIB_PATH):
    raise SwbError('HIP engine not built: %s is missing (run `python __graft_entry__.py`)' %
                   LIB_PATH)
  # PyTorch bundles its own HIP runtime; it must be the first (and only) one loaded in the
  # process, otherwise a second runtime initialised later sees no devices.
  import torch
  if torch.cuda.is_available():
    torch.cuda.init()
  # (an A/B build of an older revision, named by SWB_LIBRARY, may lack the newer calls)
  lib = _abi.declare(C.CDLL(LIB_PATH), tolerate_missing=bool(os.environ.get('SWB_LIBRARY')))
  _lib = lib
  return lib


def check(rc):
  if rc != 0:
    raise SwbError('swb error %d: %s' % (rc, load().swb_last_error().decode()))
