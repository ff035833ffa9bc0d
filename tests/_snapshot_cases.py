"""Scenarios of snapshots (swb_save_state, swb_load_state, swb_copy_pool), written against an engine
factory so that the emulated suite (tests/test_emulated_snapshot.py) and the GPU suite (tests/test_gpu_snapshot.py) run the
same checks.  TEST INFRASTRUCTURE ONLY.

The oracle has no set_state and gets none.  What a loaded environment must do from its next step on is what ANOTHER oracle.Engine
does: one whose pool is a copy with pool_base / pool_len gathered by the load's slot map and which has been stepped, from its
reset, through the action history of the source environments, gathered the same way.  `Lineage` keeps that book: for every live
environment the environment whose pool range it resets through and the (global step, action row) pairs it has taken.  Its
`oracle()` builds one oracle per group of environments that took the same number of steps and merges them behind the interface
tests/_parity.compare expects; from there on every step goes through `compare`: state, rewards and step types bit for bit,
frames +-0.
"""
import copy
import ctypes as C

import numpy as np
import torch

from spriteworld_amd import _abi
from spriteworld_amd import workloads
from tests import _parity

N = 12
MAX_LEN = 4
_bits = _parity.bits
# case 1: (workload, anti_aliasing, what variant() must say)
ROUND_TRIP = (('goal_s5', 5, {'large_frames': 0, 'paint_in_cover': 0}), ('f64_drag', 5, {}), ('embodied_s12', 2, {}),
              ('pos:goal_x_lt_half', 2, {}), ('cluster_s40', 2, {'many_sprites': 1}), ('goal_s5', 1, {'paint_in_cover': 1}))


def built(name, aa=5, n_envs=N, seed=0, max_len=MAX_LEN, episodes_per_env=3):
  """(cfg, pool, sample) with episodes of at most `max_len` steps; 'pos:<case>' as in tests/_rollout_cases.py."""
  if name.startswith('pos:'):
    from tests import _rollout_cases
    return _rollout_cases.built(name, n_envs=n_envs, seed=seed, max_len=max_len, episodes_per_env=episodes_per_env)
  cfg, pool, sample = workloads.build(name, n_envs, episodes_per_env=episodes_per_env, seed=seed, anti_aliasing=aa)
  cfg.max_episode_length = max_len
  return cfg, pool, sample


def null_actions(cfg, n=None):
  n = cfg.n_envs if n is None else n
  return np.zeros((n, 2), np.int32) if cfg.action_space == _abi.ACTION_EMBODIED else np.zeros((n, 4))


def still_actions(cfg):
  """SelectMove / DragAndDrop: a click in the middle with a motion of exactly zero -- whatever it hits stays where it is."""
  assert cfg.action_space != _abi.ACTION_EMBODIED
  return np.full((cfg.n_envs, 4), 0.5)


def violations(eng):
  """Bounds violations the emulated kernels counted since the last call (0 on the device: it has no such counter)."""
  if not hasattr(eng.lib, 'emu_violations'):
    return 0
  eng.lib.emu_violations.restype = C.c_long
  return eng.lib.emu_violations(1)


class _Merged(object):
  """Environment n is environment n of oracle parts[k][0] where parts[k][1][n]: what _parity.compare calls `ora`."""

  def __init__(self, parts):
    self.parts = parts

  def _merge(self, dicts):
    out = {}
    for key, first in dicts[0].items():
      if first is None:
        out[key] = None
        continue
      out[key] = first.copy()
      for d, (_, mask) in zip(dicts, self.parts):
        out[key][mask] = d[key][mask]
    return out

  def step(self, actions, render=True):
    return self._merge([o.step(actions, render=render) for o, _ in self.parts])

  def state(self):
    return self._merge([o.state() for o, _ in self.parts])


class Lineage(object):
  """Who every live environment is: root[n], the environment of the ORIGINAL batch whose pool range it resets through, and
  hist[n], the (global step, action row) pairs it has taken since its reset.  `log` is the actions of every global step."""

  def __init__(self, cfg, pool, log=None):
    self.cfg, self.pool = cfg, pool
    self.log = [] if log is None else log
    self.root = list(range(cfg.n_envs))
    self.hist = [[] for _ in range(cfg.n_envs)]

  def took(self, actions):
    self.log.append(np.array(actions))
    t = len(self.log) - 1
    for n, h in enumerate(self.hist):
      h.append((t, n))

  def saved(self, index=None):
    index = range(len(self.root)) if index is None else index
    return [(self.root[e], list(self.hist[e])) for e in index]

  def loaded(self, saved, slots=None):
    slots = range(len(self.root)) if slots is None else slots
    for n, c in enumerate(slots):
      if 0 <= c < len(saved):
        self.root[n], self.hist[n] = saved[c][0], list(saved[c][1])

  def forked(self, copies):
    cfg = type(self.cfg).from_buffer_copy(self.cfg)
    cfg.n_envs = self.cfg.n_envs * copies
    child = Lineage(cfg, self.pool)
    child.root = [self.root[n // copies] for n in range(cfg.n_envs)]
    child.log = [np.repeat(a, copies, axis=0) for a in self.log]      # (row r of the parent is rows r * copies ... of the child)
    child.hist = [[(t, row * copies) for t, row in self.hist[n // copies]] for n in range(cfg.n_envs)]
    return child

  def oracle(self):
    from oracle import oracle
    n_envs = len(self.root)
    pool = copy.copy(self.pool)
    pool.pool_base = np.ascontiguousarray(np.asarray(self.pool.pool_base)[self.root], dtype=np.int32)
    pool.pool_len = np.ascontiguousarray(np.asarray(self.pool.pool_len)[self.root], dtype=np.int32)
    cfg = type(self.cfg).from_buffer_copy(self.cfg)
    cfg.n_envs = n_envs
    parts = []
    for length in sorted(set(len(h) for h in self.hist)):
      mask = np.array([len(h) == length for h in self.hist])
      ora = oracle.Engine(cfg, pool)
      for i in range(length):
        a = null_actions(cfg, n_envs).astype(self.log[0].dtype)
        for n in np.flatnonzero(mask):
          t, row = self.hist[n][i]
          a[n] = self.log[t][row]
        ora.step(a, render=False)
      parts.append((ora, mask))
    return _Merged(parts)


class Pair(object):
  """An engine and the oracle of its lineage side by side; every step through _parity.compare."""

  def __init__(self, make_engine, cfg, pool, what, expect=None):
    self.cfg, self.pool, self.what = cfg, pool, what
    self.eng = make_engine(cfg, pool)
    v = self.eng.variant()
    for k, value in (expect or {}).items():
      assert v[k] == value, (what, k, v)
    self.line = Lineage(cfg, pool)
    self.ora = self.line.oracle()
    self.t = 0
    self.outs = []

  def step(self, actions, frame_envs=None):
    want = self.ora.step(actions)
    self.eng.step(actions)
    got = self.eng.outputs_host()
    _parity.compare(self.t, self.ora, self.eng, want, got, what=self.what, frame_envs=frame_envs)
    self.line.took(actions)
    self.t += 1
    self.outs.append(got)
    return want

  def save(self, index=None):
    return self.eng.save_state(index), self.line.saved(index)

  def load(self, saved, slots=None, **kw):
    snap, book = saved
    self.eng.load_state(snap, slots, **kw)
    self.line.loaded(book, slots)
    self.ora = self.line.oracle()
    assert_same_state(self.eng.state(), self.ora.state(), self.what + ' straight after the load')

  def close(self):
    assert violations(self.eng) == 0
    self.eng.close()


def assert_same_state(a, b, what=''):
  for k in ('x', 'y'):
    np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=k + ' ' + what)
  for k in ('n_sprites', 'pool_entry', 'step_count', 'reset_next', 'episode'):
    np.testing.assert_array_equal(a[k], b[k], err_msg=k + ' ' + what)


def desynchronised(make_engine, name, aa, seed, expect=None, **kw):
  """A Pair whose environments are at different points of their episodes (every workload ends its episodes by the step limit,
  all environments at once): two steps, a snapshot, one more step, and the even environments go back to the snapshot."""
  cfg, pool, sample = built(name, aa, seed=seed, **kw)
  p = Pair(make_engine, cfg, pool, '%s aa=%d' % (name, aa), expect)
  rng = np.random.default_rng(seed + 100)
  p.step(sample(rng))
  p.step(sample(rng))
  early = p.save()
  p.step(sample(rng))
  p.load(early, [n if n % 2 == 0 else -1 for n in range(cfg.n_envs)])
  return p, sample, rng


# ---------------------------------------------------------------------------------------------------------------------
def round_trip_case(make_engine, name, aa, expect=None, seed=0, k=5):
  """1. Step to a point at which some environments have just returned LAST (reset_next set) and others are inside an episode,
  save, step k more, load the snapshot back, step the same k actions again."""
  p, sample, rng = desynchronised(make_engine, name, aa, seed, expect)
  for _ in range(2 * MAX_LEN):
    if p.ora.state()['reset_next'].any():
      break
    p.step(sample(rng))
  at_save = p.ora.state()
  pending = at_save['reset_next'].astype(bool)
  assert pending.any() and not pending.all(), (name, pending)       # coverage, on the oracle: chosen seeds
  saved = p.save()
  np.testing.assert_array_equal(saved[0].reset_next.cpu().numpy(), at_save['reset_next'])
  acts = [sample(rng) for _ in range(k)]
  first = [p.step(a) for a in acts]
  mark = len(p.outs)
  p.load(saved)
  again = [p.step(a) for a in acts]
  types = np.stack([w['step_type'] for w in again])                  # [k, N]
  assert (types[0][pending] == _abi.STEP_FIRST).all()                # the restored reset_next
  mid = ~pending
  for n in np.flatnonzero(mid):                                      # the restored step_count runs into the step limit
    last_at = MAX_LEN - int(at_save['step_count'][n]) - 1
    assert 0 <= last_at < k - 1, (n, last_at)
    assert types[last_at, n] == _abi.STEP_LAST and types[last_at + 1, n] == _abi.STEP_FIRST, (name, n, types[:, n])
  for a, b in zip(first, again):                                     # the same k steps twice
    assert a['obs'].tobytes() == b['obs'].tobytes() and a['step_type'].tobytes() == b['step_type'].tobytes()
    np.testing.assert_array_equal(_bits(np.nan_to_num(a['reward'])), _bits(np.nan_to_num(b['reward'])))
  for a, b in zip(p.outs[mark - k:mark], p.outs[mark:]):
    assert a['obs'].tobytes() == b['obs'].tobytes()
  p.close()


def permuted_case(make_engine, name='goal_s5', aa=5, seed=1):
  """2. The slot map is a permutation with repeats and three -1: untouched environments continue their own oracle, loaded ones
  their source's -- the source's entry sequence across two auto-resets included."""
  cfg, pool, sample = built(name, aa, seed=seed)
  p = Pair(make_engine, cfg, pool, 'permuted ' + name)
  rng = np.random.default_rng(seed + 100)
  for _ in range(3):
    p.step(sample(rng))
  index = [4, 9, 1, 11, 0, 6, 7, 2]                                  # slot c holds environment index[c]
  saved = p.save(index)
  for _ in range(2):
    p.step(sample(rng))
  slots = [3, 3, 0, -1, 7, 1, -1, 5, 2, 6, -1, 4]
  assert sorted(set(slots) - {-1}) == list(range(8)) and slots.count(-1) == 3 and slots.count(3) == 2
  before = p.eng.state()
  p.load(saved, slots)
  after = p.eng.state()
  for n in (3, 6, 10):                                               # -1: exactly as it was
    for key in after:
      assert after[key][n].tobytes() == before[key][n].tobytes(), (key, n)
  source = [index[c] if c >= 0 else n for n, c in enumerate(slots)]
  base, length = np.asarray(pool.pool_base), np.asarray(pool.pool_len)
  firsts = np.zeros(cfg.n_envs, int)
  for _ in range(2 * MAX_LEN + 3):
    want = p.step(sample(rng))
    firsts += want['step_type'] == _abi.STEP_FIRST
    entry = p.ora.state()['pool_entry']
    for n, s in enumerate(source):                                   # the entries are the source's
      assert base[s] <= entry[n] < base[s] + length[s], (n, s, entry[n])
  moved = [n for n, s in enumerate(source) if s != n]
  assert len(moved) >= 8 and (firsts[moved] >= 2).all(), firsts
  p.close()


def stale_list_case(make_engine, monkeypatch, seed=2):
  """3. The trap: every environment stands still until its lists are kept and its frame is copied from the cache; three are
  then loaded with states whose sprites are elsewhere and stand still again.  Only their lists may be built, only their
  frames resampled."""
  monkeypatch.setenv('SWB_LIST_STATS', '1')
  cfg, pool, sample = built('goal_s5', 5, seed=seed, max_len=50)
  p = Pair(make_engine, cfg, pool, 'stale lists', {'paint_in_cover': 0, 'large_frames': 0})
  eng = p.eng
  v = eng.variant()
  assert v['frame_cache_bytes'] > 0
  tasks = v['n_bands'] * v['n_column_groups']
  rng = np.random.default_rng(seed + 100)
  null = still_actions(cfg)
  p.step(null)
  p.step(sample(rng))
  elsewhere = p.save()
  there = p.ora.state()
  for _ in range(3):                                                 # (the third rendering launch: the engine trims its lists)
    now, a = p.ora.state(), sample(rng)
    top = now['n_sprites'] - 1                                       # a click on the top sprite: it moves
    a[:, 0], a[:, 1] = now['x'][np.arange(N), top], now['y'][np.arange(N), top]
    p.step(a)
  here = p.ora.state()
  differ = np.flatnonzero(((_bits(there['x']) != _bits(here['x'])) | (_bits(there['y']) != _bits(here['y']))).any(axis=1))
  assert len(differ) >= 3, differ                                    # coverage, on the oracle: chosen seed
  chosen = [int(n) for n in differ[:3]]
  for _ in range(4):                                                 # build, fill, copy, copy
    p.step(null)
  kept0, built0 = eng.list_stats()
  copied0, filled0, resampled0 = eng.frame_stats()
  p.step(null)
  assert eng.list_stats() == (kept0 + N, built0) and eng.frame_stats() == (copied0 + N * tasks, filled0, resampled0)
  p.load(elsewhere, [n if n in chosen else -1 for n in range(N)])
  p.step(null)
  assert eng.list_stats() == (kept0 + N + 9, built0 + 3), (eng.list_stats(), kept0, built0)
  assert eng.frame_stats() == (copied0 + (N + 9) * tasks, filled0, resampled0 + 3 * tasks), (eng.frame_stats(), copied0, filled0, resampled0)
  p.step(null)                                                       # the three fill, the nine copy
  assert eng.list_stats() == (kept0 + 2 * N + 9, built0 + 3)
  assert eng.frame_stats() == (copied0 + (N + 18) * tasks, filled0 + 3 * tasks, resampled0 + 3 * tasks), eng.frame_stats()
  p.step(null)                                                       # all twelve copy
  assert eng.frame_stats() == (copied0 + (2 * N + 18) * tasks, filled0 + 3 * tasks, resampled0 + 3 * tasks), eng.frame_stats()
  p.close()


def rollout_end_case(make_engine, seed=3, n_cand=4, n_steps=5):
  """4. load_state(the end states of the picked candidates) leaves what K real steps with actions[:, n, best[n]] leave."""
  cfg, pool, sample = built('goal_s5', 5, seed=seed)
  p = Pair(make_engine, cfg, pool, 'rollout end states')
  twin = make_engine(cfg, pool)
  rng = np.random.default_rng(seed + 100)
  with_no_rollout = 'no rollout has run'
  try:
    p.eng.save_state(source='rollout')
    raise AssertionError('a handle without a rollout saved its end states')
  except RuntimeError as e:
    assert with_no_rollout in str(e), e
  for _ in range(3):
    a = sample(rng)
    p.step(a)
    twin.step(a)
  acts = np.ascontiguousarray(np.stack([np.stack([sample(rng) for _ in range(n_cand)], axis=1) for _ in range(n_steps)], axis=0))
  res = p.eng.rollout(acts)
  types = res['step_type'].cpu().numpy()
  best = rng.integers(0, n_cand, size=N)
  picked = types[:, np.arange(N), best]
  assert (picked[:-1] == _abi.STEP_LAST).any(), 'no picked candidate crosses a LAST'       # coverage
  before = p.eng.state()
  snap = p.eng.save_state(np.arange(N) * n_cand + best, source='rollout')
  everything = p.eng.save_state(source='rollout')
  assert len(snap) == N and len(everything) == N * n_cand
  for key in snap.FIELDS:
    np.testing.assert_array_equal(getattr(everything, key).cpu().numpy()[np.arange(N) * n_cand + best], getattr(snap, key).cpu().numpy(), err_msg=key)
  assert_same_state(p.eng.state(), before, 'saving the end states')
  for k in range(n_steps):                                           # what the plan does, step by step: the twin engine, the oracle
    a = acts[k, np.arange(N), best]
    twin.step(a)
    p.ora.step(a, render=False)
    p.line.took(a)
  p.eng.load_state(snap)
  assert_same_state(p.eng.state(), twin.state(), 'against the engine that took the steps')
  assert_same_state(p.eng.state(), p.ora.state(), 'against the oracle')
  for _ in range(2):
    a = sample(rng)
    p.step(a)
    twin.step(a)
    out = twin.outputs_host()
    assert out['obs'].tobytes() == p.outs[-1]['obs'].tobytes() and out['step_type'].tobytes() == p.outs[-1]['step_type'].tobytes()
  p.eng.rollout(acts)
  p.eng.set_pool(pool)                                               # a stale pool
  try:
    p.eng.save_state(source='rollout')
    raise AssertionError('the end states of a rollout were saved under a new pool')
  except RuntimeError as e:
    assert 'the pool has changed since the last rollout' in str(e), e
  twin.close()
  p.close()


def _environment(n_envs=N, refresh_every=0):
  """A BatchedEnvironment of four sprites on 64x64 frames, episodes of at most MAX_LEN steps, drawn on the device."""
  from spriteworld_amd import action_spaces, environment, renderers, sprite_generators, tasks
  from spriteworld_amd import factor_distributions as distribs
  common = [distribs.Continuous('x', 0.1, 0.9), distribs.Continuous('y', 0.1, 0.9),
            distribs.Discrete('shape', ['square', 'triangle', 'circle']), distribs.Discrete('scale', [0.2]),
            distribs.Continuous('c1', 0.3, 1.), distribs.Continuous('c2', 0.9, 1.)]
  gen = sprite_generators.chain_generators(
      sprite_generators.generate_sprites(distribs.Product(common + [distribs.Continuous('c0', 0., 0.4)]), num_sprites=2),
      sprite_generators.generate_sprites(distribs.Product(common + [distribs.Continuous('c0', 0.5, 0.9)]), num_sprites=2))
  task = tasks.FindGoalPosition(filter_distrib=distribs.Continuous('c0', 0., 0.4), terminate_distance=0.2)
  rend = {'image': renderers.PILRenderer(image_size=(64, 64), anti_aliasing=5, color_to_rgb=renderers.color_maps.hsv_to_rgb)}
  return environment.BatchedEnvironment(task=task, action_space=action_spaces.SelectMove(scale=0.25), renderers=rend,
                                        init_sprites=gen, max_episode_length=MAX_LEN, num_envs=n_envs, episodes_per_env=3,
                                        refresh_every=refresh_every, seed=5)


def _env_step(env, line, ora, actions, t, what):
  want = ora.step(actions)
  env.step(torch.as_tensor(actions))
  _parity.compare(t, ora, env.engine, want, env.engine.outputs_host(), what=what)
  line.took(actions)
  return want


def fork_case(copies=3):
  """5. fork(3) of a batch inside its episodes: 36 environments that step and render against an oracle of 36 from their first
  step, the parent untouched.  The engine class is environment._engine.Engine: the caller has patched the emulated one in, or
  runs on the GPU."""
  from spriteworld_amd import environment
  env = _environment()
  env.reset()
  cfg, pool = env.engine.cfg, env.engine.get_pool()
  line = Lineage(cfg, pool)
  line.took(np.zeros((N, 4)))
  ora = line.oracle()
  rng = np.random.default_rng(11)
  for t in range(2):
    _env_step(env, line, ora, rng.uniform(0., 1., size=(N, 4)), t + 1, 'parent')
  marks = (np.arange(N) % 3 == 0).astype(np.uint8) * 0x40            # a caller's unread flags (no bit the engine sets)
  env.engine.error.copy_(torch.as_tensor(marks))
  before = env.state()
  assert not before['reset_next'].any() and (before['step_count'] == 2).all()
  child = env.fork(copies)
  assert isinstance(child, environment.BatchedEnvironment) and child.num_envs == N * copies
  assert child.engine.pool_id() == env.engine.pool_id() != 0
  st = child.state()
  for key in before:
    np.testing.assert_array_equal(st[key], np.repeat(before[key], copies, axis=0), err_msg=key)
  assert_same_state(env.state(), before, 'the parent after the fork')
  np.testing.assert_array_equal(env.engine.outputs_host()['error'], marks)
  env.engine.error.zero_()
  child_line = line.forked(copies)
  child_ora = child_line.oracle()
  firsts = 0
  for t in range(MAX_LEN + 2):                                       # every copy its own actions: the copies part ways
    want = _env_step(child, child_line, child_ora, rng.uniform(0., 1., size=(N * copies, 4)), t, 'fork')
    firsts += int((want['step_type'] == _abi.STEP_FIRST).sum())
  assert firsts >= N * copies
  x = child.state()['x'].reshape(N, copies, -1)
  assert (_bits(x[:, 0]) != _bits(x[:, 1])).any()
  for t in range(3):                                                 # the parent's next real steps
    _env_step(env, line, ora, rng.uniform(0., 1., size=(N, 4)), 3 + t, 'parent after the fork')
  child.check()
  with np.testing.assert_raises(Exception):
    child.refresh_pool()
  # the chosen plans of a rollout adopted in one launch; then bad slot values: counted, and check() raises
  twin = child.fork(1)
  plans = rng.uniform(0., 1., size=(N * copies, 2, 3, 4))
  ret = child.rollout(torch.as_tensor(plans))
  pick = ret.episode_return().argmax(1)
  child.load_state(child.rollout_snapshot(pick))
  assert len(child.rollout_snapshot()) == N * copies * 2
  for k in range(3):
    twin.step(torch.as_tensor(plans[np.arange(N * copies), pick.cpu().numpy(), k]))
  assert_same_state(child.state(), twin.state(), 'the adopted plans')
  held = child.state()
  slots = np.arange(N * copies)
  slots[[1, 5]] = [N * copies, -2]
  child.load_state(twin.save_state(), slots)
  assert_same_state(child.state(), held, 'rejected slots')
  with np.testing.assert_raises(IndexError):
    child.check()
  child.check()                                                      # (read and cleared)
  twin.close()
  child.close()
  env.close()


def unlike_handles_case(make_engine):
  """5b. swb_copy_pool between handles that differ is refused; so is a handle without a pool as the source."""
  cfg, pool, _ = built('goal_s5', 5)
  other_cfg, other_pool, _ = built('embodied_s12', 2)
  a, b, empty = make_engine(cfg, pool), make_engine(other_cfg, other_pool), make_engine(cfg, None)
  base, length = np.asarray(pool.pool_base), np.asarray(pool.pool_len)
  for dst, src, code, text in ((b, a, -1, 'swb_copy_pool: the handles differ'), (a, empty, -4, 'swb_copy_pool: src has no pool'),
                               (a, a, -1, 'the same handle')):
    rc = a.lib.swb_copy_pool(dst._h, src._h, base.ctypes.data, length.ctypes.data, None)
    assert rc == code and text in a.lib.swb_last_error().decode(), (rc, a.lib.swb_last_error())
  bad = base + pool.n_entries
  rc = a.lib.swb_copy_pool(empty._h, a._h, bad.ctypes.data, length.ctypes.data, None)
  assert rc == -1 and 'outside the pool' in a.lib.swb_last_error().decode()
  assert empty.pool_id() == 0
  empty.copy_pool_from(a, base, length)
  assert empty.pool_id() == a.pool_id()
  for e in (a, b, empty):
    e.close()


def pool_identity_case(make_engine, seed=4):
  """6. A snapshot is refused once the pool has been replaced, unless the caller vouches for it; Snapshot.cpu() and get_pool()
  put into a brand-new engine continue bit for bit."""
  cfg, pool, sample = built('goal_s5', 5, seed=seed)
  p = Pair(make_engine, cfg, pool, 'pool identity')
  rng = np.random.default_rng(seed + 100)
  ids = [p.eng.pool_id()]
  for _ in range(3):
    p.step(sample(rng))
  saved = p.save()
  assert saved[0].pool_id == ids[0] != 0
  host = saved[0].cpu()
  assert host.device.type == 'cpu' and len(host) == N and host.pool_id == ids[0]
  pool_host = p.eng.get_pool()
  p.step(sample(rng))
  # a brand-new engine (a restart): the pool from the host, the state from the host copy
  fresh = Pair(make_engine, cfg, pool_host, 'resumed')
  ids.append(fresh.eng.pool_id())
  try:
    fresh.eng.load_state(host)
    raise AssertionError('a snapshot of another pool was loaded')
  except RuntimeError as e:
    assert 'swb_load_state: the snapshot was saved under pool' in str(e), e
  fresh.line.log = list(p.line.log)
  fresh.load((host, saved[1]), check_pool=False)
  assert fresh.eng.state()['episode'].tobytes() == saved[0].episode.cpu().numpy().tobytes()
  fresh.t = 3
  for _ in range(2 * MAX_LEN):
    fresh.step(sample(rng))
  fresh.close()
  # the same engine after set_pool: refused, then accepted on the caller's word
  p.eng.set_pool(pool)
  ids.append(p.eng.pool_id())
  assert len(set(ids)) == 3 and 0 not in ids, ids
  try:
    p.eng.load_state(saved[0])
    raise AssertionError('a snapshot of the pool before set_pool was loaded')
  except RuntimeError as e:
    assert 'swb_load_state: the snapshot was saved under pool' in str(e), e
  p.line = Lineage(cfg, pool, log=p.line.log)
  p.load(saved, check_pool=False)
  for _ in range(3):
    p.step(sample(rng))
  p.close()


def refresh_refuses_case():
  """6b. BatchedEnvironment: refresh_pool() redraws entries a snapshot may play; the snapshot is refused afterwards."""
  env = _environment()
  env.reset()
  snap = env.save_state([0, 1])
  assert len(snap) == 2
  env.refresh_pool()
  with np.testing.assert_raises_regex(RuntimeError, 'saved under pool'):
    env.load_state(snap, [0, 1] + [-1] * (N - 2))
  env.close()


def _snapshot_struct(snap, **replace):
  s = snap.as_struct()
  for k, v in replace.items():
    setattr(s, k, v)
  return s


def guards_case(make_engine):
  """7. Every refusal, with its message; slot values out of range leave the environment alone and are counted."""
  cfg, pool, sample = built('goal_s5', 5)
  eng = make_engine(cfg, pool)
  rng = np.random.default_rng(5)
  for _ in range(2):
    eng.step(sample(rng))
  lib, h = eng.lib, eng._h
  snap = eng.save_state()
  cs = snap.as_struct()
  idx = torch.zeros(N, dtype=torch.int32, device=eng.device)
  ip = C.c_void_p(idx.data_ptr())
  err = lambda: lib.swb_last_error().decode()
  pid = snap.pool_id
  calls = (
      (lambda: lib.swb_save_state(None, 0, None, N, C.byref(cs), None), -1, 'swb_save_state: null handle'),
      (lambda: lib.swb_load_state(None, C.byref(cs), N, None, pid, None, None), -1, 'swb_load_state: null handle'),
      (lambda: lib.swb_save_state(h, 0, None, N, None, None), -1, 'swb_save_state: snapshot is NULL'),
      (lambda: lib.swb_load_state(h, None, N, None, pid, None, None), -1, 'swb_load_state: snapshot is NULL'),
      (lambda: lib.swb_save_state(h, 0, None, N, C.byref(_snapshot_struct(snap, episode=None)), None), -1,
       'swb_save_state: a pointer of the snapshot is NULL'),
      (lambda: lib.swb_load_state(h, C.byref(_snapshot_struct(snap, reset_next=None)), N, None, pid, None, None), -1,
       'swb_load_state: a pointer of the snapshot is NULL'),
      (lambda: lib.swb_save_state(h, 0, ip, 0, C.byref(cs), None), -1, 'swb_save_state: C must be positive'),
      (lambda: lib.swb_load_state(h, C.byref(cs), -3, ip, pid, None, None), -1, 'swb_load_state: C must be positive'),
      (lambda: lib.swb_save_state(h, 0, ip, 2**31 - 1, C.byref(cs), None), -1, 'swb_save_state: C x max_sprites'),
      (lambda: lib.swb_load_state(h, C.byref(cs), 2**31 - 1, ip, pid, None, None), -1, 'swb_load_state: C x max_sprites'),
      (lambda: lib.swb_save_state(h, 2, None, N, C.byref(cs), None), -1, 'swb_save_state: unknown source 2'),
      (lambda: lib.swb_save_state(h, 0, None, N - 1, C.byref(cs), None), -1, 'swb_save_state: index is NULL'),
      (lambda: lib.swb_load_state(h, C.byref(cs), N + 1, None, pid, None, None), -1, 'swb_load_state: slot is NULL'),
      (lambda: lib.swb_load_state(h, C.byref(cs), N, None, pid + 12345, None, None), -4, 'swb_load_state: the snapshot was saved under pool'),
      (lambda: lib.swb_save_state(h, 1, None, N, C.byref(cs), None), -4, 'swb_save_state: no rollout has run'),
      (lambda: lib.swb_pool_id(None, None), -1, 'swb_pool_id: null argument'),
      (lambda: lib.swb_copy_pool(None, h, None, None, None), -1, 'swb_copy_pool: null argument'),
  )
  held = eng.state()
  for call, code, text in calls:
    rc = call()
    assert rc == code and text in err(), (rc, err(), text)
  assert_same_state(eng.state(), held, 'after the refusals')
  # slot values out of range
  eng.step(sample(rng))
  held = eng.state()
  slots = [-1] * N
  slots[2], slots[7], slots[8] = N, -2, 2**31 - 1
  eng.load_state(snap, slots)
  assert_same_state(eng.state(), held, 'rejected slots')
  assert eng.load_rejected() == 3 and eng.load_rejected() == 0
  out_of_range = eng.save_state([0, N, -1, 3])                       # slots 1 and 2 stay as Snapshot.empty made them
  assert out_of_range.pool_len.cpu().tolist()[1:3] == [1, 1] and out_of_range.reset_next.cpu().tolist() == [int(held['reset_next'][0]), 1, 1, int(held['reset_next'][3])]
  np.testing.assert_array_equal(_bits(out_of_range.x.cpu().numpy()[[0, 3]]), _bits(held['x'][[0, 3]]))
  with np.testing.assert_raises(ValueError):
    eng.save_state(source='nowhere')
  with np.testing.assert_raises(ValueError):
    eng.load_state(snap, [0] * (N - 1))
  # the setters: overrides belong to an environment slot, not to a state
  other = make_engine(cfg, pool)
  env = int(np.flatnonzero(eng.state()['reset_next'] == 0)[0])
  eng.set_sprite_attr(env, 0, _abi.ATTR_ANGLE, 45.0)
  base, length = np.ascontiguousarray(pool.pool_base, np.int32), np.ascontiguousarray(pool.pool_len, np.int32)
  for call, name in ((lambda: lib.swb_save_state(h, 0, None, N, C.byref(cs), None), 'swb_save_state'),
                     (lambda: lib.swb_load_state(h, C.byref(cs), N, None, pid, None, None), 'swb_load_state'),
                     (lambda: lib.swb_copy_pool(other._h, h, base.ctypes.data, length.ctypes.data, None), 'swb_copy_pool'),
                     (lambda: lib.swb_copy_pool(h, other._h, base.ctypes.data, length.ctypes.data, None), 'swb_copy_pool')):
    rc = call()
    assert rc == -4 and name + ': sprite setters have been called' in err(), (rc, err())
  assert violations(eng) == 0
  other.close()
  eng.close()
