"""The device sampler's model (tests/_sampler_model.py) for pools of more than 16 sprites per episode: the same Philox
stream and draws, with the z-order slots sized by the engine's limit (swb_sampler.hip.inc: slot[SWB_MAX_SPRITES])."""
import math

import numpy as np

from spriteworld_amd import _abi
from tests._sampler_model import Stream, _draw


def sample_pool(spec, n_entries, max_sprites, seed, to_rgb, label_fns, shape_names, first_entry=0):
  """Returns a dict of arrays laid out like lowering.Pool (groups without hold-outs)."""
  P, S, T = n_entries, max_sprites, len(label_fns)
  out = dict(n_sprites=np.zeros(P, np.int32), x=np.zeros((P, S)), y=np.zeros((P, S)), x_vel=np.zeros((P, S)),
             y_vel=np.zeros((P, S)), scale=np.ones((P, S)), cos_a=np.ones((P, S)), sin_a=np.zeros((P, S)),
             angle=np.zeros((P, S)), shape=np.zeros((P, S), np.int32), rgb=np.zeros((P, S, 4), np.uint8),
             color=np.zeros((P, S, 3)), label=np.zeros((P, T, S), np.int8))
  for e in range(P):
    rng = Stream(seed, first_entry + e)
    if spec.n_alternatives > 0:
      alt = spec.alternatives[rng.u32() % spec.n_alternatives if spec.n_alternatives > 1 else 0]
      order = [alt.group[g] for g in range(alt.n)]
    else:
      order = list(range(spec.n_groups))
    counts, n = [], 0
    for g in order:
      grp = spec.groups[g]
      c = min(grp.count_min + rng.u32() % (grp.count_max - grp.count_min + 1), S - n)
      counts.append(c)
      n += c
    slot = list(range(_abi.SWB_MAX_SPRITES))
    m = sum(counts[:spec.shuffle])
    for i in range(m - 1, 0, -1):
      j = rng.u32() % (i + 1)
      slot[i], slot[j] = slot[j], slot[i]
    out['n_sprites'][e] = n
    k = 0
    for gi, g in enumerate(order):
      grp = spec.groups[g]
      assert grp.n_holdouts == 0
      for _ in range(counts[gi]):
        s = slot[k]
        k += 1
        fv = [None] * _abi.SWB_N_FACTORS
        fv[0], fv[1] = _draw(rng, grp.factors[0]), _draw(rng, grp.factors[1])
        shape = grp.shapes[rng.u32() % grp.n_shapes]
        for i in range(2, _abi.SWB_N_FACTORS):
          fv[i] = _draw(rng, grp.factors[i])
        x, y, scale, angle, c0, c1, c2, xv, yv = fv
        out['x'][e, s], out['y'][e, s] = float(x), float(y)
        out['x_vel'][e, s], out['y_vel'][e, s] = float(xv), float(yv)
        out['shape'][e, s], out['scale'][e, s], out['angle'][e, s] = shape, float(scale), float(angle)
        th = math.radians(angle)
        out['cos_a'][e, s], out['sin_a'][e, s] = math.cos(th), math.sin(th)
        out['color'][e, s] = [float(c0), float(c1), float(c2)]
        out['rgb'][e, s, :3] = np.asarray(to_rgb((c0, c1, c2))).astype(np.uint8)
        factors = dict(x=x, y=y, shape=shape_names[shape], angle=angle, scale=scale, c0=c0, c1=c1, c2=c2,
                       x_vel=xv, y_vel=yv)
        for t, fn in enumerate(label_fns):
          out['label'][e, t, s] = fn(factors)
  return out
