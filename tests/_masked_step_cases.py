"""Scenes for stepping and resetting subsets of the batch (tests/test_emulated_masked_step.py, tests/test_gpu_masked_step.py;
DESIGN.md section 27): swb_step_masked and swb_reset_envs.

An environment whose byte of the active mask is 0 takes no part in a step: nothing of its state and none of its output entries
changes, a pending reset stays pending, its action row is never read, and its frame is drawn from the state as it is.  Every step
of every case goes through the bar of tests/_parity.py -- state arrays, rewards, step types, discounts and flags bit for bit,
frames +-0 -- against the oracle, which needs no mask: `oracle.Engine.step(a, env_range=(i0, i1))` steps a contiguous range and
writes only those entries, so a masked step is one call per run of active environments, merged into the outputs held from the
step before (`Runner`).  For partial resets every environment has an oracle of its own (`Bank`): oracle i stands for environment
i only, and `reset_all()` on it is that environment's reset.

The action rows of inactive environments are NaN (0x7fffffff for Embodied) and the frame buffer is filled with 0x5A before every
launch: every byte of every frame must be written, and nothing may be read from such a row.

The emulated file runs the same scripts on fewer environments.
"""
import ctypes as C

import numpy as np

from spriteworld_amd import _abi
from spriteworld_amd import workloads
from tests import _kept_lists_cases as kept_scene
from tests import _parity

# (name, anti_aliasing, environment of the engine, entries of variant() that must hold)
WORKLOADS = {
    'goal_s5': ('goal_s5', 5, (), {'large_frames': 0, 'many_sprites': 0, 'paint_in_cover': 0}),
    'goal_s5_large_frames': ('goal_s5', 5, (('SWB_LARGE_FRAMES', '1'),), {'large_frames': 1, 'many_sprites': 0}),
    'cluster_s5_aa1': ('cluster_s5', 1, (), {'paint_in_cover': 1}),
    'embodied_s12': ('embodied_s12', 5, (), {'large_frames': 0, 'many_sprites': 0}),
    'cluster_s40': ('cluster_s40', 2, (), {'many_sprites': 1}),
    'f64_drag': ('f64_drag', 3, (), {'large_frames': 0, 'many_sprites': 0}),
}
STEPS = 40
ALL_INACTIVE_AT, ALL_ACTIVE_AT = 9, 23
# Episodes of 50 (cluster_s5, embodied_s12) and 30 steps (cluster_s40) cannot end inside 40 steps of which 60 % are taken, and
# each case must see resets held pending: those workloads run with episodes of 12 steps (goal_s5: its own 20, f64_drag: its 15).
SHORT_EPISODES = 12

SENTINELS = {'reward': -123.25, 'discount': 0.375, 'step_type': 77, 'success': 99, 'error': 0x40}


def runs_of(active):
  """[(i0, i1)]: the maximal runs of set entries."""
  idx = np.flatnonzero(active)
  if idx.size == 0:
    return []
  cuts = np.flatnonzero(np.diff(idx) > 1)
  starts = np.concatenate(([idx[0]], idx[cuts + 1]))
  ends = np.concatenate((idx[cuts], [idx[-1]])) + 1
  return list(zip(starts.tolist(), ends.tolist()))


def poison(cfg, a, active):
  """`a` with the rows of inactive environments made unreadable."""
  a = np.array(a)
  if active is not None:
    a[~active] = 0x7fffffff if cfg.action_space == _abi.ACTION_EMBODIED else np.nan
  return a


class Bank(object):
  """One oracle.Engine per environment behind the surface of one: oracle i is stepped, reset and read for environment i only."""

  def __init__(self, cfg, pool):
    from oracle import oracle
    self.N = cfg.n_envs
    self.oras = [oracle.Engine(cfg, pool) for _ in range(self.N)]

  def step(self, a, render=True, env_range=None):
    i0, i1 = env_range
    outs = [self.oras[i].step(a, render=render, env_range=(i, i + 1)) for i in range(i0, i1)]
    res = {k: (None if outs[0][k] is None else np.zeros_like(outs[0][k])) for k in outs[0]}
    for i, o in zip(range(i0, i1), outs):
      for k in res:
        if res[k] is not None:
          res[k][i] = o[k][i]
    return res

  def reset(self, mask):
    for i in np.flatnonzero(mask):
      self.oras[i].reset_all()

  def state(self):
    sts = [o.state() for o in self.oras]
    return {k: np.stack([sts[i][k][i] for i in range(self.N)]) for k in sts[0]}


class Runner(object):
  """The engine beside the oracle; `held`: the outputs as the caller's buffers must hold them -- every entry that of the
  environment's last active step, every frame that of its current state.  With `stats` the counts of swb_list_stats and
  swb_frame_stats are held to the model of tests/_frame_cache_cases.py: a rendering launch in which a wave keeps its lists moves
  the environment's frame word to min(word + 1, 2) -- 1: its tasks fill the cache, 2: they copy from it --, any other to 0."""

  def __init__(self, make_engine, monkeypatch, cfg, pool, what, env=(), stats=False, bank=False, expect=None):
    from oracle import oracle
    for k, v in env:
      monkeypatch.setenv(k, v)
    if stats:
      monkeypatch.setenv('SWB_LIST_STATS', '1')
    self.cfg, self.what, self.t, self.N = cfg, what, 0, cfg.n_envs
    self.ora = Bank(cfg, pool) if bank else oracle.Engine(cfg, pool)
    self.eng = make_engine(cfg, pool)
    v = self.eng.variant()
    for k, value in (expect or {}).items():
      assert v[k] == value, (what, k, v)
    self.stats = stats
    if stats:
      self.eng.TRIM_AFTER = 0          # (the reallocation would rebuild every list once, in the middle of the counts)
      self.tasks = v['n_bands'] * v['n_column_groups']
      self.word = np.zeros(self.N, np.int64)
      self.kept = self.built = self.copied = self.filled = self.resampled = 0
    self.held = None
    # what the run has seen (see `assert_saw_everything`)
    self.pending_for = np.zeros(self.N, np.int64)      # steps the environment has been inactive with a reset pending
    self.was_inactive = np.zeros(self.N, bool)
    self.saw_inactive_pending = self.saw_first_after_hold = self.saw_inactive_twice = False

  def expected(self, a, active, render=True):
    """The oracle's step: all of it, or one call per run of active environments merged into the held outputs."""
    if active is None:
      active = np.ones(self.N, bool)
    if self.held is None:
      assert active.all(), 'the first step of a run takes every environment (the frame of one that never had a FIRST step is unspecified)'
    pending = self.ora.state()['reset_next'] != 0
    want = None if self.held is None else {k: (None if v is None else v.copy()) for k, v in self.held.items()}
    for i0, i1 in runs_of(active):
      out = self.ora.step(a, render=render, env_range=(i0, i1))
      if want is None:
        assert (i0, i1) == (0, self.N)
        want = out
        continue
      for k in want:
        if k == 'error':
          want[k][i0:i1] |= out[k][i0:i1]      # (sticky)
        elif out[k] is not None:
          if want[k] is None:
            want[k] = out[k].copy()
          want[k][i0:i1] = out[k][i0:i1]
    if not render:
      want['obs'] = None
    first = active & (want['step_type'] == _abi.STEP_FIRST)
    self.saw_inactive_pending |= bool((~active & pending).any())
    self.saw_first_after_hold |= bool((first & (self.pending_for > 0)).any())
    self.saw_inactive_twice |= bool((~active & self.was_inactive).any())
    self.pending_for = np.where(~active & pending, self.pending_for + 1, np.where(active, 0, self.pending_for))
    self.was_inactive = ~active
    return want

  def step(self, a, active=None, render=True, keeps=None, sentinels=False, call=None):
    """One step of both through _parity.compare.  `active`: None or bool[N]; `keeps` (stats): bool[N], the environments whose
    wave must keep its lists; `sentinels`: the output entries of the inactive environments are overwritten before the launch and
    must be untouched after it; `call(engine, actions)`: another way to the same step than `Engine.step`."""
    want = self.expected(a, active, render)
    eng = self.eng
    if render:
      eng.obs.fill_(0x5A)
    saved = {}
    idle = None if active is None else np.flatnonzero(~active)
    if sentinels and idle is not None and idle.size:
      for k, s in SENTINELS.items():
        buf = getattr(eng, k)
        saved[k] = buf[idle].clone()
        buf[idle] = s
    if call is not None:
      call(eng, poison(self.cfg, a, active))
    else:
      eng.step(poison(self.cfg, a, active), render=render, active=active)
    got = eng.outputs_host()
    for k, s in saved.items():
      assert (got[k][idle] == np.array(SENTINELS[k], dtype=got[k].dtype)).all(), ('%s of an inactive environment was written' % k, self.what, self.t)
      getattr(eng, k)[idle] = saved[k]
      got[k][idle] = saved[k].cpu().numpy()
    _parity.compare(self.t, self.ora, eng, want, got, frames=render, what=self.what)
    self.held = want if want['obs'] is not None or self.held is None else dict(want, obs=self.held['obs'])
    if self.stats and render:
      self.count(np.broadcast_to(np.asarray(keeps, dtype=bool), (self.N,)))
    self.t += 1
    return want, got

  def count(self, keeps):
    self.kept += int(keeps.sum())
    self.built += int((~keeps).sum())
    self.word = np.where(keeps, np.minimum(self.word + 1, 2), 0)
    self.copied += self.tasks * int((self.word == 2).sum())
    self.filled += self.tasks * int((self.word == 1).sum())
    self.resampled += self.tasks * int((self.word == 0).sum())
    got = self.eng.list_stats(), self.eng.frame_stats()
    want = (self.kept, self.built), (self.copied, self.filled, self.resampled)
    assert got == want, (self.what, self.t, got, want)

  def assert_saw_everything(self):
    assert self.saw_inactive_pending, self.what + ': no environment was inactive while its reset was pending'
    assert self.saw_first_after_hold, self.what + ': no FIRST step of an environment that had been held pending'
    assert self.saw_inactive_twice, self.what + ': no environment was inactive on consecutive steps'

  def close(self):
    self.eng.close()


def masks(n_envs, steps, seed):
  """Step 0 all active, then Bernoulli(0.6) per environment and step; one step all inactive, one all active."""
  rng = np.random.default_rng(seed)
  m = rng.random((steps, n_envs)) < 0.6
  m[0] = True
  m[ALL_INACTIVE_AT] = False
  m[ALL_ACTIVE_AT] = True
  return m


def against_the_oracle(make_engine, monkeypatch, which, n_envs, seed=0):
  """STEPS masked steps of a workload on its render path."""
  name, aa, env, expect = WORKLOADS[which]
  cfg, pool, sample = workloads.build(name, n_envs, episodes_per_env=4, seed=seed, anti_aliasing=aa)
  if cfg.max_episode_length > 20:
    cfg.max_episode_length = SHORT_EPISODES
  r = Runner(make_engine, monkeypatch, cfg, pool, which, env, expect=expect)
  rng = np.random.default_rng(seed + 100)
  m = masks(n_envs, STEPS, seed + 200)
  for t in range(STEPS):
    r.step(sample(rng), m[t])
  r.assert_saw_everything()
  r.close()


def cheap_path(make_engine, monkeypatch, n_envs, masked):
  """The scene of tests/_kept_lists_cases.py: FIRST, one step in which every environment hits, then five in which the even ones
  hit and the odd ones are inactive (`masked`) or miss (else).  Either way the odd waves keep their lists -- fill the frame cache
  once, then copy from it -- and the even ones build: the same counts."""
  cfg, pool = kept_scene.build(n_envs)
  r = Runner(make_engine, monkeypatch, cfg, pool, 'cheap_path masked=%s' % masked, stats=True)
  odd = (np.arange(n_envs) % 2) == 1
  r.step(kept_scene.actions(r.ora.state(), np.zeros(n_envs, bool)), keeps=False)
  r.step(kept_scene.actions(r.ora.state(), np.ones(n_envs, bool)), keeps=False)
  for _ in range(5):
    a = kept_scene.actions(r.ora.state(), ~odd)
    r.step(a, active=~odd if masked else None, keeps=odd)
  n_odd, T = int(odd.sum()), r.tasks
  assert (r.kept, r.built) == (5 * n_odd, 2 * n_envs + 5 * (n_envs - n_odd))
  assert (r.copied, r.filled) == (4 * n_odd * T, n_odd * T)
  counts = (r.kept, r.built, r.copied, r.filled, r.resampled)
  r.close()
  return counts


def nothing_written(make_engine, monkeypatch, which, n_envs, steps=12, seed=3):
  """The caller's reward, discount, step_type, success and error entries of inactive environments carry sentinels into every
  launch and out of it; the frame buffer goes in as 0x5A and comes out right everywhere."""
  name, aa, env, expect = WORKLOADS[which]
  cfg, pool, sample = workloads.build(name, n_envs, episodes_per_env=4, seed=seed, anti_aliasing=aa)
  cfg.max_episode_length = 4
  r = Runner(make_engine, monkeypatch, cfg, pool, 'nothing_written ' + which, env, expect=expect)
  rng = np.random.default_rng(seed + 100)
  m = np.random.default_rng(seed + 200).random((steps, n_envs)) < 0.5
  m[:5] = True           # (FIRST and four steps: every episode has ended ...)
  m[5] = False           # (... and every environment is inactive with its reset pending)
  for t in range(steps):
    r.step(sample(rng), m[t], sentinels=True)
  assert r.saw_inactive_pending
  r.close()


def three_ways_to_step_everything(make_engine, monkeypatch, n_envs):
  """swb_step, swb_step_masked without a mask and swb_step_masked with a mask of ones: ten steps of three engines (odd
  environments hit, episodes of four steps), the same outputs, state, list and frame statistics."""
  cfg, pool = kept_scene.build(n_envs, max_episode_length=4)

  def no_mask(eng, a):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(a), device=eng.device)
    eng._last_actions = t            # keep alive until the launch is consumed
    eng._check(eng.lib.swb_step_masked(eng._h, C.c_void_p(t.data_ptr()), None, C.byref(eng._outs), eng._stream()))

  ways = {'swb_step': dict(), 'no_mask': dict(call=no_mask), 'ones': dict(active=np.ones(n_envs, bool))}
  runners = {k: Runner(make_engine, monkeypatch, cfg, pool, 'three_ways ' + k, stats=True) for k in ways}
  odd = (np.arange(n_envs) % 2) == 1
  for t in range(10):
    res = {}
    for k, r in runners.items():
      pending = r.ora.state()['reset_next'] != 0
      _, got = r.step(kept_scene.actions(r.ora.state(), odd), keeps=~odd & ~pending, **ways[k])
      res[k] = (got, r.eng.state(), r.eng.list_stats() + r.eng.frame_stats())
    for k in ('no_mask', 'ones'):
      for i in (0, 1):
        for name, v in res[k][i].items():
          assert v.tobytes() == res['swb_step'][i][name].tobytes(), (k, name, t)
      assert res[k][2] == res['swb_step'][2], (k, t)
  assert runners['ones'].kept > 0 and runners['ones'].copied > 0
  for r in runners.values():
    r.close()


def reset_envs(make_engine, monkeypatch, n_envs, emu_error):
  """Five steps; a third of the environments are marked (swb_reset_envs); in the next masked step half of the marked ones are
  inactive -- still pending, the old frame, the old episode number -- and the other half start their next pool entry with FIRST,
  while the unmarked ones go on MID and KEEP their lists (the epoch did not move); then ten more masked steps."""
  cfg, pool = kept_scene.build(n_envs)
  r = Runner(make_engine, monkeypatch, cfg, pool, 'reset_envs', stats=True, bank=True)
  none = np.zeros(n_envs, bool)
  r.step(kept_scene.actions(r.ora.state(), none), keeps=False)
  for t in range(4):
    hit = (np.arange(n_envs) + t) % 2 == 0
    r.step(kept_scene.actions(r.ora.state(), hit), keeps=~hit)
  marked = (np.arange(n_envs) % 3) == 0
  held_back = marked & ((np.arange(n_envs) % 6) == 0)
  before = r.ora.state()
  frames_before = r.held['obs'].copy()
  r.ora.reset(marked)
  r.eng.reset_envs(marked)
  assert (r.eng.state()['reset_next'] != 0).tolist() == marked.tolist()
  want, got = r.step(kept_scene.actions(r.ora.state(), none), active=~held_back, keeps=~(marked & ~held_back))
  st = r.eng.state()
  assert (st['reset_next'][held_back] == 1).all() and (st['episode'][held_back] == before['episode'][held_back]).all()
  assert (got['obs'][held_back] == frames_before[held_back]).all()
  started = marked & ~held_back
  assert (got['step_type'][started] == _abi.STEP_FIRST).all() and (got['step_type'][~marked] == _abi.STEP_MID).all()
  assert (st['episode'][started] == before['episode'][started] + 1).all()
  assert (st['pool_entry'][started] == pool.pool_base[started] + before['episode'][started] % pool.pool_len[started]).all()
  rng = np.random.default_rng(11)
  for t in range(10):
    active = rng.random(n_envs) < 0.6
    if t == 0:
      active |= held_back              # (the environments held back start now)
    hit = rng.random(n_envs) < 0.5
    pending = r.ora.state()['reset_next'] != 0
    r.step(kept_scene.actions(r.ora.state(), hit), active=active, keeps=~active | (~hit & ~pending))
  assert r.saw_first_after_hold and r.saw_inactive_pending
  with np.testing.assert_raises_regex(emu_error, 'mask is NULL'):
    r.eng._check(r.eng.lib.swb_reset_envs(r.eng._h, None, r.eng._stream()))
  r.close()


def with_load_state(make_engine, monkeypatch, n_envs, a_env=1, b_env=4):
  """Environment a's snapshot loaded into b, then a step with both inactive: b shows a's frame, and both what render() gives."""
  cfg, pool, sample = workloads.build('goal_s5', n_envs, episodes_per_env=4, seed=1, anti_aliasing=5)
  r = Runner(make_engine, monkeypatch, cfg, pool, 'with_load_state')
  rng = np.random.default_rng(5)
  for _ in range(3):
    r.step(sample(rng))
  eng = r.eng
  slots = np.full(n_envs, -1, np.int32)
  slots[b_env] = 0
  eng.load_state(eng.save_state(np.array([a_env], np.int32)), slots, check_pool=False)
  active = np.ones(n_envs, bool)
  active[[a_env, b_env]] = False
  eng.obs.fill_(0x5A)
  eng.step(poison(cfg, sample(rng), active), active=active)
  obs = eng.outputs_host()['obs']
  assert obs[b_env].tobytes() == obs[a_env].tobytes()
  assert (obs[a_env] == r.held['obs'][a_env]).all()
  rendered = eng.render().cpu().numpy()
  assert rendered.tobytes() == obs.tobytes()
  r.close()


def with_set_positions(make_engine, monkeypatch, n_envs):
  """set_positions, then a step with everything inactive: the frames are the oracle's set_positions + render."""
  cfg, pool, sample = workloads.build('goal_s5', n_envs, episodes_per_env=4, seed=1, anti_aliasing=5)
  r = Runner(make_engine, monkeypatch, cfg, pool, 'with_set_positions')
  rng = np.random.default_rng(5)
  for _ in range(3):
    r.step(sample(rng))
  st = r.ora.state()
  x, y = st['x'].copy(), st['y'].copy()
  y[:, 0] = np.where(y[:, 0] < 0.5, y[:, 0] + 0.2, y[:, 0] - 0.2)
  r.ora.set_positions(x, y)
  r.eng.set_positions(x, y)
  r.held['obs'] = r.ora.render()
  r.step(sample(rng), active=np.zeros(n_envs, bool))
  r.step(sample(rng))
  r.close()


def with_sprite_setter(make_engine, monkeypatch, n_envs):
  """A sprite setter on an environment that is then inactive shows in its frame."""
  cfg, pool, sample = workloads.build('goal_s5', n_envs, episodes_per_env=4, seed=1, anti_aliasing=5)
  r = Runner(make_engine, monkeypatch, cfg, pool, 'with_sprite_setter')
  rng = np.random.default_rng(5)
  for _ in range(3):
    r.step(sample(rng))
  changed = (np.arange(n_envs) % 2) == 0
  for e in np.flatnonzero(changed):
    r.ora.set_sprite_attr(int(e), 1, _abi.ATTR_SCALE, 0.3)
    r.eng.set_sprite_attr(int(e), 1, _abi.ATTR_SCALE, 0.3)
  before = r.held['obs'].copy()
  r.held['obs'] = r.ora.render()
  assert all((r.held['obs'][e] != before[e]).any() for e in np.flatnonzero(changed))
  r.step(sample(rng), active=~changed)
  r.step(sample(rng))
  r.close()
