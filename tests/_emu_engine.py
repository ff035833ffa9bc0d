"""`engine.Engine` itself over tests/emu/_build/libswb_emu.so (TEST INFRASTRUCTURE ONLY).

libswb_emu.so is the source of spriteworld_amd/csrc -- the C-ABI host side AND the fused step kernel -- compiled for the
host against an emulation of the HIP runtime and of the wave-level builtins (tests/emu): every work-item is a fibre,
cross-lane operations are rendezvous of the 64 lanes.  "Device" buffers are CPU torch tensors.  It exists so that the CPU
test suite can execute the kernel source, and the product's Python binding above it, against the oracle where no GPU is
available; the product never loads it (spriteworld_amd/_lib.py loads csrc/libswb.so, built by hipcc for gfx950, and raises
when it is missing).  The seam is the handful of members `Engine` keeps for what depends on where the library runs.
"""
import contextlib
import ctypes as C
import os

import torch

from spriteworld_amd import _abi
from spriteworld_amd import engine
from tests.emu import build_emu

_lib = None


class EmuError(RuntimeError):
  pass


def lib():
  global _lib
  if _lib is None:      # (SWB_EMU_CSRC: an older copy of the sources may lack the newer calls)
    _lib = _abi.declare(C.CDLL(build_emu.build()), tolerate_missing=bool(os.environ.get('SWB_EMU_CSRC')))
  return _lib


def check(rc):
  if rc != 0:
    raise EmuError('swb error %d: %s' % (rc, lib().swb_last_error().decode()))


class EmuEngine(engine.Engine):
  """N environments stepped by the emulated kernel (`cfg`: _abi.SwbConfig, `pool`: lowering.Pool or None)."""

  _check = staticmethod(check)

  def __init__(self, cfg, pool, device=0):
    super().__init__(cfg, pool, device)
    self.obs.fill_(0x5A)      # garbage: every byte must be written

  def _open(self, device):
    return lib(), torch.device('cpu')

  def _device_scope(self):
    return contextlib.nullcontext()

  def _sync(self):
    pass

  def _stream(self):
    return None


EmuTorchEngine = EmuEngine      # (the name the environment-level tests and the bench dry run patch in)
