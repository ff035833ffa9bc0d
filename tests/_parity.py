"""The bar every engine-against-oracle test holds a step to (TEST INFRASTRUCTURE ONLY): sprite positions, the state arrays,
step types, success flags, discounts and rewards bit-exact (rewards with the same NaN pattern), frames +-0, no error flag -- or,
for scenes the reference raises on, exactly the flags the caller expects.
The emulated suites and the `-m gpu` suites call the same three functions with an engine factory of their own."""
import numpy as np

from spriteworld_amd import workloads


def bits(a):
  return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def compare(t, ora, eng, want, got, frames=True, reward_ulp=0, what='', errors=None, nan_positions=False, frame_envs=None):
  """One step's outputs (`want`: the oracle's, `got`: the engine's, on the host) and the state after it; returns the
  engine's state.  reward_ulp: a bound in units of the last place in place of bit-equal rewards; `what`: the caller's case, put
  in front of the step in every message; `errors`: the error buffer expected in place of an empty one (the engine's flags are sticky:
  the OR of the oracle's per-step flags so far).  nan_positions: a position the oracle holds as NaN must be NaN in the engine
  (sign and payload differ between x86 and the GPU) -- every other position stays bit-equal; off, NaN positions are compared bit
  for bit like the rest.  frame_envs: bool[N], the environments whose frames are compared (None: all)."""
  at = '%st=%d' % (what and what + ', ', t)
  st_o, st_g = ora.state(), eng.state()
  if errors is None:
    assert not got['error'].any(), ('error flags ' + at, np.flatnonzero(got['error'])[:8])
  else:
    np.testing.assert_array_equal(got['error'], errors, err_msg='error flags ' + at)
  np.testing.assert_array_equal(got['step_type'], want['step_type'], err_msg='step_type ' + at)
  for k in ('x', 'y'):
    pg, po = st_g[k], st_o[k]
    if nan_positions:
      nan = np.isnan(po)
      np.testing.assert_array_equal(np.isnan(pg), nan, err_msg=k + ' NaN pattern ' + at)
      pg, po = np.where(nan, 0.0, pg), np.where(nan, 0.0, po)
    np.testing.assert_array_equal(bits(pg), bits(po), err_msg=k + ' ' + at)
  for k in ('step_count', 'reset_next', 'episode', 'pool_entry', 'n_sprites'):
    np.testing.assert_array_equal(st_g[k], st_o[k], err_msg=k + ' ' + at)
  np.testing.assert_array_equal(got['success'], want['success'], err_msg='success ' + at)
  np.testing.assert_array_equal(got['discount'].view(np.uint32), want['discount'].view(np.uint32), err_msg='discount ' + at)
  assert_rewards_equal(got['reward'], want['reward'], at, reward_ulp)
  if frames:
    diff = np.abs(got['obs'].astype(np.int16) - want['obs'].astype(np.int16))
    if frame_envs is not None:      # (the frames left out compare as equal)
      diff[~np.asarray(frame_envs, dtype=bool)] = 0
    assert diff.max() == 0, ('frame diff', int(diff.max()), int((diff > 0).sum()), at, np.argwhere(diff > 0)[:5].tolist())
  return st_g


def assert_rewards_equal(gr, wr, what, reward_ulp=0):
  """NaN where the oracle has NaN (a FIRST step has no reward), bit-equal -- or within `reward_ulp` -- elsewhere."""
  assert np.array_equal(np.isnan(gr), np.isnan(wr)), 'reward NaN pattern ' + what
  ok = ~np.isnan(wr)
  if reward_ulp == 0:
    np.testing.assert_array_equal(bits(gr[ok]), bits(wr[ok]), err_msg='reward ' + what)
  elif ok.any():
    d = np.abs(bits(gr[ok]).astype(np.int64) - bits(wr[ok]).astype(np.int64))
    assert d.max() <= reward_ulp, ('reward ulp', d.max(), what)


def run(make_engine, name, n_envs, steps, aa, seed=0, episodes_per_env=3, frame_every=1, expect=None):
  """Steps workload `name` on `make_engine(cfg, pool)` and the oracle, every step through compare(); `expect`: entries of
  variant() that must hold (large_frames, many_sprites).  Returns (FIRST steps seen, the most sprites an episode had)."""
  from oracle import oracle
  cfg, pool, sample = workloads.build(name, n_envs, episodes_per_env=episodes_per_env, seed=seed, anti_aliasing=aa)
  ora, eng = oracle.Engine(cfg, pool), make_engine(cfg, pool)
  v = eng.variant()
  for k, value in (expect or {}).items():
    assert v[k] == value, (k, v)
  rng = np.random.default_rng(seed + 100)
  firsts, most = 0, 0
  for t in range(steps):
    a = sample(rng)
    want = ora.step(a)
    eng.step(a)
    st = compare(t, ora, eng, want, eng.outputs_host(), frames=(t % frame_every == 0))
    firsts += int((want['step_type'] == 0).sum())
    most = max(most, int(st['n_sprites'].max()))
  eng.close()
  return firsts, most
