"""The step-kernel scenarios that are more than one `_parity.run` call (TEST INFRASTRUCTURE ONLY), written against an engine
FACTORY: tests/test_emulated_kernel.py runs them on the emulated library, tests/test_gpu_parity.py on the HIP engine.  The
sizes (workloads, environment counts, steps, seeds, capacities) are the callers'; what is asserted is the same on both.  A case
that takes `monkeypatch` sets the SWB_* switches that make its scenario, the same on both backends; the others are the caller's."""
import ctypes as C

import numpy as np

from spriteworld_amd import _abi, workloads
from tests import _parity


def _violations(eng):
  """Run-record reads outside a list's own part and the arena since the last call, which only the emulated build counts
  (tests/emu/emu_runtime.cc); 0 on a library without the counter."""
  if not hasattr(eng.lib, 'emu_violations'):
    return 0
  eng.lib.emu_violations.restype = C.c_long
  return eng.lib.emu_violations(1)


def _build(make_engine, monkeypatch, name, n_envs, aa, episodes_per_env, seed):
  from oracle import oracle
  if aa == 1:
    monkeypatch.setenv('SWB_NO_PAINT_IN_COVER', '1')       # (through the run lists and the fill kernel)
  cfg, pool, sample = workloads.build(name, n_envs, episodes_per_env=episodes_per_env, seed=seed, anti_aliasing=aa)
  eng = make_engine(cfg, pool)
  _violations(eng)
  return cfg, pool, sample, oracle.Engine(cfg, pool), eng


def cover_cost_order_case(make_engine, name, n_envs, aa):
  """Launches of more than one round of cover waves take the environments in order of what their cover wave cost in the previous
  launch (cycle counts filed per environment, heavy scenes first); SWB_COVER_ORDER, the caller's, asks for it at any batch size.
  The order is only used after a launch that filed every environment: a step without an observation in between falls back to the
  plain order for one launch.  State, rewards and frames do not depend on any of it."""
  from oracle import oracle
  _parity.run(make_engine, name, n_envs, 4, aa)
  cfg, pool, sample = workloads.build(name, n_envs, episodes_per_env=3, seed=1, anti_aliasing=aa)
  ora, eng = oracle.Engine(cfg, pool), make_engine(cfg, pool)
  rng = np.random.default_rng(7)
  for t in range(6):
    a = sample(rng)
    want = ora.step(a)
    eng.step(a, render=(t != 2))                     # launch 2 renders nothing and files nothing
    if t == 2:
      continue
    got = eng.outputs_host()
    assert not got['error'].any()
    np.testing.assert_array_equal(got['step_type'], want['step_type'])
    np.testing.assert_array_equal(_parity.bits(eng.state()['x']), _parity.bits(ora.state()['x']))
    assert np.array_equal(got['obs'], want['obs']), t
  eng.close()


def run_list_overflow_case(make_engine, monkeypatch, workload_list, run_cap, n_envs, steps, quantifier):
  """A run list that does not fit its capacity (swb_params::run_cap; SWB_RUN_CAP lowers it) and has no arena to continue in flags
  the environment (SWB_ENV_ERR_SPAN_OVERFLOW) instead of writing past it -- `quantifier` (np.any, np.all) of the environments
  after `steps` steps -- and the second kernel never READS past it either: every band of an overflowed list starts inside the
  written part (with SWB_RUN_CAP=8, SWB_BANDS=4 a band header pointed 114 units beyond an 8-unit list).
  workload_list: (name, anti_aliasing)."""
  monkeypatch.setenv('SWB_RUN_CAP', str(run_cap))
  monkeypatch.setenv('SWB_ARENA_UNITS', '0')
  for name, aa in workload_list:
    _, _, sample, _, eng = _build(make_engine, monkeypatch, name, n_envs, aa, episodes_per_env=2, seed=0)
    rng = np.random.default_rng(0)
    for _ in range(steps):
      eng.step(sample(rng))
    assert quantifier(eng.outputs_host()['error'] & _abi.ENV_ERR_SPAN_OVERFLOW)
    assert _violations(eng) == 0
    eng.close()


def arena_move_case(make_engine, monkeypatch, workload_list, run_cap, bands, arena, episodes_per_env, seed, rng_seed, exhausted_by=None):
  """A run list owns a part of its own and MOVES to a segment of a shared arena, twice (four times ...) as large, when it
  outgrows it (the wave copies what it wrote; positions in the header are counted from the own part, so the second kernels know
  nothing of it).  With an own part of `run_cap` = 8 .. 64 units EVERY list moves, several times: every step is held to the bar
  on both second kernels (resample; fill: anti_aliasing 1 on a wide image) for every band count, and no run record is read
  outside the list's own part or the arena.  With an arena too small for workload `exhausted_by` the environments that find it
  exhausted are FLAGGED, that workload flags some, and every other frame is still exact.
  workload_list: (name, n_envs, steps, anti_aliasing)."""
  monkeypatch.setenv('SWB_RUN_CAP', str(run_cap))
  monkeypatch.setenv('SWB_ARENA_UNITS', str(arena))
  monkeypatch.setenv('SWB_BANDS', str(bands))
  monkeypatch.setenv('SWB_BAND_TASKS', '1')         # (a moving list shifts the band starts it has recorded -- and their copy in LDS)
  for name, n_envs, steps, aa in workload_list:
    _, _, sample, ora, eng = _build(make_engine, monkeypatch, name, n_envs, aa, episodes_per_env, seed)
    rng = np.random.default_rng(rng_seed)
    flagged_any = False
    for t in range(steps):
      a = sample(rng)
      want = ora.step(a)
      eng.step(a)
      got = eng.outputs_host()
      if exhausted_by is None:
        _parity.compare(t, ora, eng, want, got, what=name)
        continue
      flagged = (got['error'] & _abi.ENV_ERR_SPAN_OVERFLOW) != 0
      flagged_any |= bool(flagged.any())
      assert np.array_equal(got['obs'][~flagged], want['obs'][~flagged])
      assert np.array_equal(got['step_type'], want['step_type'])
      _parity.assert_rewards_equal(got['reward'], want['reward'], '%s, t=%d' % (name, t))
    if name == exhausted_by:
      assert flagged_any
    assert _violations(eng) == 0
    v = eng.variant()
    assert v['run_cap'] == run_cap and v['arena_units'] == arena and v['run_list_bytes'] > 0
    eng.close()


def trim_case(make_engine, workload_list, seed, rng_seed, steps, total_halves):
  """The lists start with room for any scene of convex sprites (max(4, S + 1) units per canvas row); after the third rendering
  launch the engine cuts them to 1.25 x the longest list written + a shared arena (swb_trim_run_lists), once.  Frames stay exact
  before, at and after the cut; a new pool restores the reservation.  workload_list: (name, n_envs, anti_aliasing).
  total_halves: the batch is large enough for the lists' own parts to dwarf the arena's floor of sixteen worst-case lists, so the
  cut halves the whole allocation too."""
  from oracle import oracle
  for name, n_envs, aa in workload_list:
    cfg, pool, sample = workloads.build(name, n_envs, episodes_per_env=3, seed=seed, anti_aliasing=aa)
    eng, ora = make_engine(cfg, pool), oracle.Engine(cfg, pool)
    rng = np.random.default_rng(rng_seed)
    sizes = []
    for t in range(steps):
      a = sample(rng)
      want = ora.step(a)
      eng.step(a)
      got = eng.outputs_host()
      assert not got['error'].any()
      assert np.array_equal(got['obs'], want['obs']), (name, t)
      v = eng.variant()
      sizes.append((v['run_cap'], v['arena_units'], v['run_list_bytes']))
    worst = max(4, cfg.max_sprites + 1) * cfg.anti_aliasing * cfg.image_w + 1
    assert sizes[0][0] == sizes[1][0] == worst                     # the start-up reservation ...
    assert sizes[2][0] < worst // 2 and sizes[2][2] < sizes[1][2], sizes           # ... cut at the third launch
    fixed_before, fixed_after = sizes[1][2] - 8 * sizes[1][1], sizes[2][2] - 8 * sizes[2][1]
    assert fixed_after < fixed_before // 2, sizes                  # (the lists' own parts; the arena has a floor)
    if total_halves:
      assert sizes[2][2] < sizes[1][2] // 2, sizes
    assert sizes[-1] == sizes[2]                                   # once
    assert sizes[2][1] >= 16 * worst                               # the arena: at least sixteen worst-case lists
    assert eng.trim() == sizes[2][0]                               # (calling it again changes nothing)
    eng.set_pool(pool)                                             # a new pool: the full reservation again
    eng.step(sample(rng))
    assert eng.variant()['run_cap'] == worst
    eng.close()


def position_filter_case(make_engine, name, f32, n_envs, min_flips):
  """Task filters / cluster distributions keyed on x, y (tests/_position_cases.py; pinned against the unmodified reference
  through the oracle in tests/test_oracle_vs_reference.py and through tests/golden/position_*.npz): the reference re-evaluates
  `contains(sprite.factors)` at every step (tasks.py:134-137, 196-205), the kernel looks every sprite's label up in the cell of
  the task's position grid it stands in.  Rewards must change more than `min_flips` times over the forty steps."""
  from oracle import oracle
  from spriteworld_amd import lowering
  from tests import _position_cases as pc
  ns = pc.namespace_of_mirrors()
  task, aspace, rends, keep, max_len = pc.environment_parts(ns, name)
  episodes = pc.episodes_of(ns, name, f32, n_episodes=3 * n_envs)
  cfg = lowering.lower_config(task, aspace, rends, keep, max_len, n_envs, pc.N_SPRITES, pos_is_f32=f32)
  pool = lowering.lower_episodes(episodes, task, rends, max_sprites=pc.N_SPRITES).assign_round_robin(n_envs, 3)
  assert pool.cell_label is not None
  ora, eng = oracle.Engine(cfg, pool), make_engine(cfg, pool)
  rng = np.random.default_rng(11)
  sticky = np.zeros(n_envs, np.uint8)
  flips, prev = 0, None
  for t in range(40):
    a = rng.uniform(0.0, 1.0, size=(n_envs, 4))
    st = ora.state()
    for i in range(0, n_envs, 2):                      # click ON a sprite in every second environment
      k = int(rng.integers(0, max(int(st['n_sprites'][i]), 1)))
      a[i, 0], a[i, 1] = st['x'][i, k], st['y'][i, k]
    want = ora.step(a)
    eng.step(a)
    got = eng.outputs_host()
    np.testing.assert_array_equal(got['step_type'], want['step_type'])
    np.testing.assert_array_equal(got['success'], want['success'])
    _parity.assert_rewards_equal(got['reward'], want['reward'], 't=%d' % t)
    sticky |= want['error']                            # (the engine's error flags are sticky; the oracle's are per step)
    np.testing.assert_array_equal(got['error'], sticky)
    np.testing.assert_array_equal(got['obs'], want['obs'])
    if prev is not None:
      flips += int((want['reward'] != prev).sum())
    prev = want['reward']
  assert flips > min_flips
  eng.close()
