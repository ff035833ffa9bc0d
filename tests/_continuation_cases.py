"""Scenes for the continuation runs of the hand-off lists (tests/test_emulated_continuation_runs.py, tests/test_gpu_continuation_runs.py).

At anti_aliasing > 1 the cover kernel ends a run at every canvas row that ends an output row's window.  Rows below such a forced
end that have the spans of the run before them become a CONTINUATION run: one unit without spans, for which the resample kernel
keeps the horizontal pass it has.  The scenes are the smallest in which that can go wrong:

  square       one axis-aligned square of scale 0.3 (96 canvas rows of one span at anti_aliasing 5: about 19 forced ends)
  square_bg    the same on a non-black background: the rows without spans are listed too and continue one another
  square_wide  a 128x64 image, the square across the boundary between the two groups of 64 output columns (a row changes, or
               leaves, one group's list and continues in the other's)
  stack5       five overlapping squares, staggered: rows of one to five spans (beyond three: overflow units, never folded)
"""
import numpy as np

from spriteworld_amd import action_spaces
from spriteworld_amd import lowering
from spriteworld_amd import renderers
from spriteworld_amd import synthetic
from spriteworld_amd import tasks
from tests import _parity

CASES = ('square', 'square_bg', 'square_wide', 'stack5')


def build(case, n_envs, aa, episodes_per_env=2, seed=0):
  """(SwbConfig, Pool, sample_actions(rng)) of `case`."""
  rng = np.random.default_rng(seed)
  P = n_envs * episodes_per_env
  n = 5 if case == 'stack5' else 1
  size = (128, 64) if case == 'square_wide' else (64, 64)
  bg = (7, 30, 110) if case == 'square_bg' else (0, 0, 0)
  rend = {'image': renderers.PILRenderer(image_size=size, anti_aliasing=aa, bg_color=bg, color_to_rgb=renderers.hsv_to_rgb)}
  task = tasks.FindGoalPosition(filter_distrib=None, terminate_distance=0.075)
  aspace = action_spaces.SelectMove(scale=0.1)
  pool = synthetic.make_pool(rng, P, n, [(0.0, 1.0)] * n, [[1]] * n, shape_names=('square',), scales=(0.3,), angles=(0,),
                             shuffle=False)
  for e in range(P):
    for s in range(n):
      if case == 'stack5':          # a staircase: every sprite shows a sliver left of and above the next one
        x, y = 0.3 + 0.06 * s + rng.uniform(-0.01, 0.01), 0.3 + 0.06 * s + rng.uniform(-0.01, 0.01)
      else:
        x, y = rng.uniform(0.45, 0.55), rng.uniform(0.3, 0.7)
      pool.x[e, s], pool.y[e, s] = float(np.float32(x)), float(np.float32(y))
  cfg = lowering.lower_config(task, aspace, rend, True, 6, n_envs, n, True)
  pool.assign_round_robin(n_envs, episodes_per_env)

  def sample(r):
    return r.uniform(0.0, 1.0, size=(n_envs, 4))
  return cfg, pool, sample


def run(make_engine, case, n_envs, steps, aa, seed=0):
  """Steps `make_engine(cfg, pool)` and the oracle side by side: the bar of tests/_parity.py (state, rewards, step types,
  discounts and flags bit for bit, frames +-0)."""
  from oracle import oracle
  cfg, pool, sample = build(case, n_envs, aa, seed=seed)
  ora, eng = oracle.Engine(cfg, pool), make_engine(cfg, pool)
  rng = np.random.default_rng(seed + 100)
  for t in range(steps):
    a = sample(rng)
    want = ora.step(a)
    eng.step(a)
    _parity.compare(t, ora, eng, want, eng.outputs_host(), what='%s, %d environments, anti_aliasing %d' % (case, n_envs, aa))
  eng.close()
