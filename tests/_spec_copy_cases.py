"""Scenes for the speculative copies of the cover launch (tests/test_emulated_spec_copy.py, tests/test_gpu_spec_copy.py;
DESIGN.md section 29).

A rendering launch on the live state of a handle with a frame cache has one more workgroup per (environment, column group) in
its cover grid.  Such a workgroup reads the environment's header word while the environment's own cover wave may be writing it,
and copies the cached frame if the word is not 0 -- before anyone knows whether the environment keeps its lists.  Whichever value
it reads, the frame must be right: an environment that keeps for the second time files no resample task and its frame IS the
copy; any other has every byte rewritten by the resample kernel.

Every case runs under SWB_SPEC_COPY=first (the copy workgroups in front: each reads the word the PREVIOUS launch left) and under
`behind` (the default; on the emulator, which runs workgroups in index order, each reads the word THIS launch wrote): the two
extremes of the race, deterministically.  The scene, the script and the model of the word are tests/_frame_cache_cases.py's; the
frames are held to oracle.Engine through the bar of tests/_parity.py at every step, +-0, with SWB_LIST_STATS set and the caller's
buffer filled with 0xA5 before every launch.  swb_list_stats, swb_frame_stats and swb_split_stats are held to the model the
parent's tests hold them to (the keeping wave now adds what its resample tasks used to count), swb_spec_copy_stats to the number
of copy workgroups that must have copied: exactly on the emulator, between the two extremes on the GPU.
"""
import numpy as np
import torch

from spriteworld_amd import _abi
from tests import _frame_cache_cases as fc
from tests import _masked_step_cases as masked
from tests import _parity
from tests import _snapshot_cases as sn
from tests import _split_bands_cases as sb

ORDERS = ('first', 'behind')
BETWEEN = ('render', 'step_without_frame', 'set_positions', 'sprite_setter', 'trim', 'upload_tables', 'rollout_frames')
GEOMETRIES = ('narrow_last_group', 'wide_build', 'band_tasks_8', 'background')


def under(monkeypatch, order):
  assert order in ORDERS
  monkeypatch.setenv('SWB_SPEC_COPY', order)


class Pair(fc.Pair):
  """tests/_frame_cache_cases.py's pair with the copy workgroups: `groups` is how many of them copied so far.  One that reads the
  old word copies where it is not 0 (`first`), one that reads the new word where that is not 0 (`behind`, in index order)."""

  def __init__(self, make_engine, monkeypatch, cfg, pool, what, order, exact, env=(), **kw):
    under(monkeypatch, order)
    fc.Pair.__init__(self, make_engine, monkeypatch, cfg, pool, '%s [%s]' % (what, order), env, **kw)
    self.order, self.exact = order, exact
    self.ncg = self.eng.variant()['n_column_groups']
    self.lo = self.hi = 0
    self.scribble = True

  def launch(self, keeps):
    old = self.word.copy()
    fc.Pair.launch(self, keeps)
    new = self.word
    if self.cache and self.cfg.anti_aliasing != 1:
      if self.exact:
        n = int(((old if self.order == 'first' else new) != 0).sum())
        self.lo += self.ncg * n
        self.hi += self.ncg * n
      else:
        self.lo += self.ncg * int(((old != 0) & (new != 0)).sum())
        self.hi += self.ncg * int(((old != 0) | (new != 0)).sum())
    self.check_groups()

  def check_groups(self):
    got = self.eng.spec_copy_stats()
    assert self.lo <= got <= self.hi, (self.what, self.t, got, self.lo, self.hi)

  def step(self, hit, keeps=None, render=True):
    want = fc.Pair.step(self, hit, keeps, render)
    if render:
      self.held = want
    return want

  def step_masked(self, hit, active):
    """swb_step_masked: the oracle steps the runs of active environments, an inactive one keeps the outputs of its last active
    step and the frame of its unchanged state, and its wave keeps its lists whatever its last step type was."""
    hit = np.broadcast_to(np.asarray(hit, dtype=bool), (self.N,)) & active
    a = fc.actions(self.ora.state(), hit)
    want = {k: v.copy() for k, v in self.held.items()}
    for i0, i1 in masked.runs_of(active):
      out = self.ora.step(a, render=True, env_range=(i0, i1))
      for k in want:
        if k == 'error':
          want[k][i0:i1] |= out[k][i0:i1]
        else:
          want[k][i0:i1] = out[k][i0:i1]
    self.eng.obs.fill_(0xA5)
    self.eng.step(masked.poison(self.cfg, a, active), active=active)
    got = self.eng.outputs_host()
    _parity.compare(self.t, self.ora, self.eng, want, got, frames=True, what=self.what)
    self.held = want
    self.frames.append(got['obs'].copy())
    self.launch(~active | ((want['step_type'] != _abi.STEP_FIRST) & ~hit))
    self.t += 1
    return want


def scripted(make_engine, monkeypatch, n_envs, order, exact, steps=14):
  """SCRIPT -- build, fill, move, fill, move, fill, copy, copy, move, fill -- every environment at its own point of it, so that
  keepers, fillers and builders share every launch; the steps alternate between two observation buffers of the caller's."""
  cfg, pool = fc.build(n_envs)
  p = Pair(make_engine, monkeypatch, cfg, pool, 'scripted', order, exact)
  eng = p.eng
  shape, nbytes = tuple(eng.obs.shape), eng.obs.numel()
  raw = [torch.zeros(nbytes + 16, dtype=torch.uint8, device=eng.device) for _ in range(2)]
  bufs = [r[(-r.data_ptr()) % 16:][:nbytes].view(shape) for r in raw]
  for t in range(steps):
    eng.obs = bufs[t % 2]
    eng._outs.obs = eng.obs.data_ptr()
    p.step(fc.scripted_hits(n_envs, t))
  assert p.copied > 0 and p.filled > p.tasks * n_envs and p.resampled > p.tasks * n_envs
  assert p.hi > p.copied // p.tasks * p.ncg       # (some copies were overwritten: the speculation was wrong there)
  p.close()


def stale_cache(make_engine, monkeypatch, n_envs, order, exact):
  """kept (the cache holds frame A), moved (builds: word 0, the cache still holds A), kept (word 1), kept (word 2).  The third
  launch's copy workgroup that reads 1 copies A -- the fill must overwrite it; the fourth's that reads 1 must copy."""
  cfg, pool = fc.build(n_envs)
  p = Pair(make_engine, monkeypatch, cfg, pool, 'stale_cache', order, exact)
  for _ in range(3):
    p.step(False)
  assert p.word.tolist() == [2] * n_envs
  p.step(True)
  assert (p.frames[-1] != p.frames[-2]).any() and p.word.tolist() == [0] * n_envs
  p.step(False)
  assert p.word.tolist() == [1] * n_envs and p.frames[-1].tobytes() == p.frames[-2].tobytes()
  p.step(False)
  assert p.word.tolist() == [2] * n_envs and p.frames[-1].tobytes() == p.frames[-2].tobytes()
  T = p.tasks * n_envs
  assert (p.copied, p.filled, p.resampled) == (2 * T, 2 * T, 2 * T)
  if exact:       # first: launches 3, 4 (old word 2), 6 (old 1); behind: launches 2, 3 (new 1, 2), 5, 6
    assert p.lo == p.hi == p.ncg * n_envs * (3 if order == 'first' else 4)
  p.close()


def geometry(make_engine, monkeypatch, n_envs, which, order, exact):
  """SCRIPT on the other shapes of a copy workgroup's rectangle and of the counts a keeping wave adds."""
  env, size, bg = (), (64, 64), (0, 0, 0)
  if which == 'narrow_last_group':    # 72 columns: two groups, the second 8 columns wide, rows of 216 bytes -- the dword mover
    size = (72, 64)
  elif which == 'wide_build':         # 128x128: the cover build of the wide translation unit, two groups of 192-byte segments
    size = (128, 128)
  elif which == 'band_tasks_8':       # every band a task: a keeping wave counts eight copies per column group
    env = (('SWB_BANDS', '8'), ('SWB_BAND_TASKS', '1'))
  elif which == 'background':
    bg = (7, 30, 110)
  else:
    raise ValueError(which)
  cfg, pool = fc.build(n_envs, size=size, bg=bg)
  p = Pair(make_engine, monkeypatch, cfg, pool, which, order, exact, env)
  v = p.eng.variant()
  if which == 'narrow_last_group':
    assert v['n_column_groups'] == 2 and tuple(p.eng.obs.shape)[1:] == (64, 72, 3)
  if which == 'wide_build':
    assert v['n_column_groups'] == 2 and '<20' in v['cover_kernel'], v
  if which == 'band_tasks_8':
    assert v['n_bands'] == 8 and p.tasks == 8
  for t in range(10):
    p.step(fc.scripted_hits(n_envs, t))
  assert p.copied > 0 and p.filled > 0
  p.close()


def split_bands(make_engine, monkeypatch, n_envs, which, order):
  """Split bands forced (SWB_SPLIT_BANDS=8; SWB_SPLIT_WHEN 0 / huge): swb_split_stats' whole copies are the keeping waves' now."""
  under(monkeypatch, order)
  sb.thresholds(make_engine, monkeypatch, n_envs, 8, which, what='split %s [%s]' % (which, order))


def call_between(make_engine, monkeypatch, n_envs, which, order):
  """Two kept steps, the call, three more steps: tests/_frame_cache_cases.py's own case, whose counts are the parent's model."""
  under(monkeypatch, order)

  base = fc.Pair

  class Scribbling(base):         # (the parent's case scribbles from the call on: here from the first launch)
    def __init__(self, *args, **kw):
      base.__init__(self, *args, **kw)
      self.scribble = True

  monkeypatch.setattr(fc, 'Pair', Scribbling)
  fc.call_between(make_engine, monkeypatch, n_envs, which)


def state_view(make_engine, monkeypatch, n_envs, order, exact):
  """Frames of rollout states between two kept steps.  The launches on the state views have no copy workgroups -- they build and
  resample every candidate's frame through the engine's own lists and headers, which makes the live lists and cached frames
  stale: the next step builds and resamples, the one after fills, the third copies, and no stale frame is ever shown."""
  cfg, pool = fc.build(n_envs)
  p = Pair(make_engine, monkeypatch, cfg, pool, 'state_view', order, exact)
  for _ in range(3):
    p.step(False)
  before = p.eng.spec_copy_stats()
  M = 2
  acts = np.stack([fc.actions(p.ora.state(), np.ones(n_envs, bool), motion=(0.9, 0.1 + 0.2 * m)) for m in range(M)], axis=1)[None]
  p.eng.rollout(acts)
  cand = p.eng.rollout_frames()['obs'].cpu().numpy()
  assert all((cand[:, m] != p.frames[-1]).any() for m in range(M))
  assert p.eng.spec_copy_stats() == before
  p.built += M * n_envs
  p.resampled += M * n_envs * p.tasks
  p.check_counts()
  p.word[:] = 0                      # (the view launches built through the live headers: the words in memory are 0 as well)
  p.step(False, keeps=False)
  p.step(False)
  p.step(False)
  assert p.word.tolist() == [2] * n_envs and p.filled == 2 * p.tasks * n_envs
  assert p.frames[-1].tobytes() == p.frames[-4].tobytes()
  p.close()


def masked_words(make_engine, monkeypatch, n_envs, order, exact):
  """step(active=mask) with inactive environments at word 0, 1 and 2: after three misses every word is 2; a hit on the
  environments e % 3 == 0, then one on e % 3 == 1 leaves the classes at 1, 0 and 2.  Then environments 0, 1 and 2 -- one of each
  -- sit out two steps (their waves keep, their frames are the unchanged state's), and everyone takes a last one."""
  cfg, pool = fc.build(n_envs)
  p = Pair(make_engine, monkeypatch, cfg, pool, 'masked_words', order, exact)
  e = np.arange(n_envs)
  for _ in range(3):
    p.step(False)
  p.step(e % 3 == 0)
  p.step(e % 3 == 1)
  active = e >= 3
  assert sorted(p.word[~active].tolist()) == [0, 1, 2] and set(p.word[active].tolist()) == {0, 1, 2}
  p.step_masked(e % 2 == 0, active)
  assert p.word[~active].tolist() == [2, 1, 2]
  p.step_masked(False, active)
  assert p.word[~active].tolist() == [2, 2, 2]
  p.step(False)
  assert p.copied > 0 and p.filled > 0
  p.close()


class Counts(object):
  """The model of the word and of the copy workgroups for a case that does not step through Pair (tests/_snapshot_cases.py's pair
  with its lineage of oracles): as Pair.launch, on a handle with a cache at anti_aliasing > 1."""

  def __init__(self, eng, what, order, exact):
    v = eng.variant()
    assert v['frame_cache_bytes'] > 0 and not v['paint_in_cover'], v
    self.eng, self.what, self.order, self.exact = eng, '%s [%s]' % (what, order), order, exact
    self.N, self.ncg, self.tasks = eng.obs.shape[0], v['n_column_groups'], v['n_bands'] * v['n_column_groups']
    self.word = np.zeros(self.N, np.int64)
    self.kept = self.built = self.copied = self.filled = self.resampled = self.lo = self.hi = 0

  def launch(self, keeps):
    old = self.word.copy()
    self.kept += int(keeps.sum())
    self.built += int((~keeps).sum())
    self.word = np.where(keeps, np.minimum(self.word + 1, 2), 0)
    self.copied += self.tasks * int((self.word == 2).sum())
    self.filled += self.tasks * int((self.word == 1).sum())
    self.resampled += self.tasks * int((self.word == 0).sum())
    if self.exact:
      n = int(((old if self.order == 'first' else self.word) != 0).sum())
      self.lo += self.ncg * n
      self.hi += self.ncg * n
    else:
      self.lo += self.ncg * int(((old != 0) & (self.word != 0)).sum())
      self.hi += self.ncg * int(((old != 0) | (self.word != 0)).sum())
    got = self.eng.list_stats(), self.eng.frame_stats()
    want = (self.kept, self.built), (self.copied, self.filled, self.resampled)
    assert got == want, (self.what, got, want)
    g = self.eng.spec_copy_stats()
    assert self.lo <= g <= self.hi, (self.what, g, self.lo, self.hi)


def load_state_between(make_engine, monkeypatch, n_envs, order, exact):
  """Two kept steps (every frame is a copy), load_state of every fourth environment with a state whose sprites stand elsewhere,
  three more steps: only the loaded environments build, then fill, then copy -- the others go on copying --, every frame is the
  oracle's of the environment's lineage, and every count the model's.  (swb_load_state makes the loaded environments' lists stale
  and leaves their words: under `first` their copy workgroups copy the stale frames, which the resample waves overwrite.)"""
  under(monkeypatch, order)
  monkeypatch.setenv('SWB_LIST_STATS', '1')
  cfg, pool, sample = sn.built('goal_s5', 5, n_envs=n_envs, seed=2, max_len=50)
  p = sn.Pair(make_engine, cfg, pool, 'load_state_between [%s]' % order, {'paint_in_cover': 0, 'large_frames': 0})
  p.eng.TRIM_AFTER = 0
  c = Counts(p.eng, 'load_state_between', order, exact)
  bits = lambda v: np.ascontiguousarray(v).view(np.uint64)

  def step(a):
    before = p.ora.state()
    p.eng.obs.fill_(0xA5)
    want = p.step(a)
    after = p.ora.state()
    moved = ((bits(before['x']) != bits(after['x'])) | (bits(before['y']) != bits(after['y']))).any(axis=1)
    c.launch((want['step_type'] != _abi.STEP_FIRST) & ~moved & ~loaded)
    loaded[:] = False

  loaded = np.zeros(n_envs, bool)      # environments whose lists a load made stale since the last launch
  rng = np.random.default_rng(102)
  null = sn.still_actions(cfg)
  step(null)
  elsewhere = p.save()
  there = p.ora.state()
  for _ in range(2):
    now, a = p.ora.state(), sample(rng)
    top = now['n_sprites'] - 1                                         # a click on the top sprite: it moves
    a[:, 0], a[:, 1] = now['x'][np.arange(n_envs), top], now['y'][np.arange(n_envs), top]
    step(a)
  here = p.ora.state()
  differ = ((bits(there['x']) != bits(here['x'])) | (bits(there['y']) != bits(here['y']))).any(axis=1)
  chosen = differ & (np.arange(n_envs) % 4 == 0)
  assert chosen.sum() >= 2, chosen
  for _ in range(3):                                                   # fill, copy, copy: two kept steps behind the fill
    step(null)
  assert c.word.tolist() == [2] * n_envs
  p.load(elsewhere, [int(n) if chosen[n] else -1 for n in range(n_envs)])
  loaded |= chosen
  frames = []
  for _ in range(3):
    step(null)
    frames.append(p.outs[-1]['obs'].copy())
  assert c.word.tolist() == [2] * n_envs
  k = int(chosen.sum())
  assert c.built == 3 * n_envs + k and c.filled == c.tasks * (n_envs + k)
  assert frames[0].tobytes() == frames[1].tobytes() == frames[2].tobytes()
  assert (frames[0][chosen] != p.outs[-4]['obs'][chosen]).any() and (frames[0][~chosen] == p.outs[-4]['obs'][~chosen]).all()
  p.close()


def absent(make_engine, monkeypatch, n_envs, which, order):
  """A handle without a frame cache (SWB_NO_FRAME_CACHE) and an anti_aliasing 1 handle: no copy workgroup ever copies, the
  frames are the oracle's, the counts the parent's."""
  if which == 'no_frame_cache':
    cfg, pool = fc.build(n_envs)
    env = (('SWB_NO_FRAME_CACHE', '1'),)
  elif which == 'anti_aliasing_1':
    cfg, pool = fc.build(n_envs, aa=1, size=(128, 64))
    env = ()
  else:
    raise ValueError(which)
  p = Pair(make_engine, monkeypatch, cfg, pool, which, order, True, env, cache=False)
  assert p.eng.variant()['frame_cache_bytes'] == 0
  for t in range(6):
    p.step(fc.scripted_hits(n_envs, t))
  assert (p.copied, p.filled) == (0, 0) and p.eng.spec_copy_stats() == 0 and p.kept > 0
  p.close()
