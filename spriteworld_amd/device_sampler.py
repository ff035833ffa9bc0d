"""Declarative sprite generator that the engine can sample on the device (swb_sample_pool).

The reference's `init_sprites` is an opaque Python callable (environment.py:68,75), so resets cost
host time per episode.  Every shipped config builds it from
`generate_sprites(Product([Continuous/Discrete ...]), num_sprites)` groups that are chained and
optionally shuffled (sprite_generators.py:27-70,101-128).  `DeviceSampler` takes those same
ingredients, keeps them inspectable, and lowers them to `swb_sampler` (include/swb.h):

    sampler = DeviceSampler([(target_factors, 2), (distractor_factors, (1, 4))], shuffle=True)
    env = BatchedEnvironment(init_sprites=sampler, ...)      # pool drawn by a HIP kernel
    env.refill_pool()                                        # fresh episodes, no host work

Calling the object samples on the host with numpy (same marginals), so it is also a valid
`init_sprites` for the reference's own Environment.  Device draws come from Philox4x32-10 streams:
the distribution is the reference's, the bit stream is not MT19937's.
"""
import math

import numpy as np

from spriteworld_amd import _abi
from spriteworld_amd import shapes as _shapes
from spriteworld_amd import sprite as sprite_lib
from spriteworld_amd.lowering import LoweringError, subtasks_of, _label_of, _threshold

_FACTOR_KEYS = _abi.FACTOR_ORDER
_DEFAULTS = dict(x=0.5, y=0.5, shape='square', angle=0, scale=0.1, c0=0, c1=0, c2=0, x_vel=0.0, y_vel=0.0)


def _lower_factor(dst, key, leaf):
  """Continuous / Discrete leaf (or None: the Sprite default) -> swb_factor."""
  if leaf is None:
    dst.kind, dst.n = _abi.FACTOR_DISCRETE, 1
    dst.cand[0] = float(_DEFAULTS[key])
    return [_DEFAULTS[key]]
  if type(leaf).__name__ == 'Continuous':
    dt = np.dtype(leaf.dtype)
    if dt == np.float32:
      dst.kind = _abi.FACTOR_UNIFORM_F32
    elif dt.kind in 'iu':
      dst.kind = _abi.FACTOR_UNIFORM_INT
    else:
      raise LoweringError('factor %s: dtype %s is not sampled on the device' % (key, dt))
    dst.lo, dst.hi = float(leaf.minval), float(leaf.maxval)
    return None
  if getattr(leaf, 'probs', None) is not None:
    raise LoweringError('factor %s: weighted Discrete factors are not sampled on the device' % key)
  cands = list(leaf.candidates)
  if not 1 <= len(cands) <= _abi.SWB_MAX_CANDIDATES:
    raise LoweringError('factor %s: 1..%d candidates' % (key, _abi.SWB_MAX_CANDIDATES))
  if not all(type(c) in (float, int) for c in cands):
    raise LoweringError('factor %s: Discrete candidates must be Python floats or ints' % key)
  dst.kind, dst.n = _abi.FACTOR_DISCRETE, len(cands)
  for i, c in enumerate(cands):
    dst.cand[i] = float(c)
  return cands


def _box_of(dist):
  """A hold-out region as {key: (lo, hi)}: a Continuous leaf or a Product of them."""
  name = type(dist).__name__
  if name == 'Continuous':
    return {dist.key: (float(dist.minval), float(dist.maxval))}
  if name == 'Product':
    out = {}
    for c in dist.components:
      out.update(_box_of(c))
    return out
  raise LoweringError('hold-out regions must be Continuous ranges (got %s)' % name)


def _marginals(dist, holdouts=None):
  """Flattens a Product / SetMinus tree of Continuous/Discrete leaves into {key: leaf}.

  SetMinus nodes append (redrawn keys, {key: (lo, hi)}) to `holdouts`."""
  name = type(dist).__name__
  if name == 'Product':
    out = {}
    for c in dist.components:
      sub = _marginals(c, holdouts)
      if set(sub) & set(out):
        raise LoweringError('factor %s appears twice' % sorted(set(sub) & set(out)))
      out.update(sub)
    return out
  if name in ('Continuous', 'Discrete'):
    return {dist.key: dist}
  if name == 'SetMinus' and holdouts is not None:
    inner = []
    out = _marginals(dist.base, inner)
    if inner:
      raise LoweringError('nested SetMinus distributions are not sampled on the device')
    holdouts.append((sorted(out), _box_of(dist.hold_out)))
    return out
  raise LoweringError('%s cannot be sampled on the device (Product / SetMinus / Continuous / Discrete)' % name)


def _count_range(count):
  """(lo, hi) inclusive of an int or of the (lo, hi) of np.random.randint(lo, hi)."""
  if isinstance(count, (tuple, list)):
    lo, hi = int(count[0]), int(count[1]) - 1
  else:
    lo = hi = int(count)
  if lo < 0 or hi < lo:
    raise ValueError('bad sprite count %r' % (count,))
  return lo, hi


class _GroupSampler(object):
  """What DeviceSampler and TreeSampler share: groups of (distribution, lo, hi, ...) generated in order or by one list of
  `alternatives` per episode, the shuffle of the leading groups, the Philox keys, and host sampling with numpy."""

  alternative_probs = None

  def _set_layout(self, shuffle, seed, alternatives):
    if not 1 <= len(self.groups) <= _abi.SWB_MAX_GROUPS:
      raise LoweringError('1..%d sprite groups are supported' % _abi.SWB_MAX_GROUPS)
    self.shuffle = _abi.SWB_MAX_GROUPS if shuffle is True else int(shuffle)
    if self.shuffle < 0:
      raise ValueError('shuffle must be a bool or a number of leading groups')
    self.alternatives = None if alternatives is None else [list(map(int, a)) for a in alternatives]
    if self.alternatives is not None:
      if not 1 <= len(self.alternatives) <= _abi.SWB_MAX_ALTERNATIVES:
        raise LoweringError('1..%d alternatives are supported' % _abi.SWB_MAX_ALTERNATIVES)
      for a in self.alternatives:
        if not 1 <= len(a) <= _abi.SWB_MAX_GROUPS or not all(0 <= g < len(self.groups) for g in a):
          raise ValueError('bad alternative %r' % (a,))
    self.seed = int(seed)
    self._draws = 0

  def _lists(self):
    return self.alternatives if self.alternatives is not None else [list(range(len(self.groups)))]

  @property
  def max_sprites(self):
    return max(sum(self.groups[g][2] for g in lst) for lst in self._lists())

  def next_seed(self):
    """A fresh 64-bit Philox key per pool (splitmix64 of seed and draw counter)."""
    z = (self.seed * 0x9E3779B97F4A7C15 + self._draws + 1) & 0xFFFFFFFFFFFFFFFF
    self._draws += 1
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return z ^ (z >> 31)

  # ---------------------------------------------------------------- host sampling (numpy)
  def __call__(self):
    lists = self._lists()
    if self.alternative_probs is not None:
      chosen = lists[np.random.choice(len(lists), p=self.alternative_probs)]
    else:
      chosen = lists[np.random.randint(len(lists))] if len(lists) > 1 else lists[0]
    sprites, n_shuffled = [], 0
    for g, gi in enumerate(chosen):
      dist, lo, hi = self.groups[gi][:3]
      n = lo if lo == hi else np.random.randint(lo, hi + 1)
      sprites.extend(sprite_lib.Sprite(**dist.sample()) for _ in range(n))
      if g < self.shuffle:
        n_shuffled = len(sprites)
    if n_shuffled > 1:
      order = np.random.permutation(n_shuffled)
      sprites = [sprites[i] for i in order] + sprites[n_shuffled:]
    return sprites


class DeviceSampler(_GroupSampler):
  """`groups`: list of (factor_distribution, num_sprites); num_sprites is an int or a (lo, hi)
  pair meaning np.random.randint(lo, hi).  `shuffle`: sprite_generators.shuffle of the z-order --
  True: all sprites; an int k: only the sprites of the first k groups (the rest keep their place
  on top, like the agent body of examples/goal_finding_embodied.py:88-93).  `alternatives`:
  sprite_generators.sample_generator -- a list of lists of group indices; each episode generates
  the groups of one list chosen uniformly (default: all groups, in order)."""

  def __init__(self, groups, shuffle=False, seed=0, alternatives=None):
    self.groups, self._holdouts = [], []
    for dist, count in groups:
      lo, hi = _count_range(count)
      holdouts = []
      marg = _marginals(dist, holdouts)
      if len(holdouts) > _abi.SWB_MAX_HOLDOUTS:
        raise LoweringError('at most %d SetMinus nodes per sprite group' % _abi.SWB_MAX_HOLDOUTS)
      self.groups.append((dist, lo, hi, marg))
      self._holdouts.append(holdouts)
    self._set_layout(shuffle, seed, alternatives)

  # ---------------------------------------------------------------- lowering
  def _group_label(self, sub, dist, marg):
    """Task label of a group's sprites; must not depend on the sampled values."""
    rng_state = np.random.get_state()      # the probes must not advance the caller's global numpy stream
    try:
      return self._group_label_probed(sub, dist, marg)
    finally:
      np.random.set_state(rng_state)

  def _group_label_probed(self, sub, dist, marg):
    probes = [dist.sample() for _ in range(256)]
    for key, leaf in marg.items():  # range ends of every continuous factor
      if type(leaf).__name__ == 'Continuous' and leaf.maxval > leaf.minval:
        if np.dtype(leaf.dtype) == np.float32:
          lo = np.float32(leaf.minval)
          hi = np.nextafter(np.float32(leaf.maxval), np.float32(-np.inf))
        else:
          lo = np.asarray(leaf.minval).astype(leaf.dtype)
          hi = np.asarray(np.nextafter(float(leaf.maxval), -np.inf)).astype(leaf.dtype)
        for v in (lo, hi):
          f = dist.sample()
          f[key] = v
          probes.append(f)
    labels = set()
    for f in probes:
      full = dict(_DEFAULTS)
      full.update(f)
      labels.add(_label_of(sub, sprite_lib.Sprite(**full)))
    if len(labels) != 1:
      raise LoweringError('task label of a sprite group depends on the sampled factors (%s): sample this '
                          'generator on the host instead' % sorted(labels))
    return labels.pop()

  def scale_kinds(self):
    """swb_factor kind of every group's `scale` factor (FACTOR_UNIFORM_F32: the sprites carry np.float32 scales)."""
    kinds = []
    for _, _, _, marg in self.groups:
      fac = _abi.SwbFactor()
      _lower_factor(fac, 'scale', marg.get('scale'))
      kinds.append(fac.kind)
    return kinds

  def lower(self, task, renderers):
    from spriteworld_amd import lowering
    spec = _abi.SwbSampler()
    spec.n_groups = len(self.groups)
    spec.shuffle = self.shuffle
    spec.n_alternatives = 0 if self.alternatives is None else len(self.alternatives)
    for i, lst in enumerate(self.alternatives or []):
      spec.alternatives[i].n = len(lst)
      for j, g in enumerate(lst):
        spec.alternatives[i].group[j] = g
    spec.color_map = _color_map_of(renderers)
    for d in range(360):  # sprite.py:147-151 rotates by radians of the stored degrees
      spec.deg_cos[d], spec.deg_sin[d] = math.cos(math.radians(d)), math.sin(math.radians(d))
    subs = subtasks_of(task)
    for sub in subs:      # labels that depend on WHERE a sprite is drawn (and then moved) are tabulated per episode on the host
      xc, yc = lowering.position_cuts(sub, True)
      if xc or yc:
        raise LoweringError('a task filter keys on position: its episodes are sampled on the host (lowering.lower_episodes '
                            'tabulates each sprite\'s label over the filter\'s position grid)')
    for g, (dist, lo, hi, marg) in enumerate(self.groups):
      grp = spec.groups[g]
      grp.count_min, grp.count_max = lo, hi
      unknown = set(marg) - set(_FACTOR_KEYS) - {'shape'}
      if unknown:
        raise LoweringError('unknown sprite factors %s' % sorted(unknown))
      for key in _FACTOR_KEYS:
        fac = grp.factor(key)
        cands = _lower_factor(fac, key, marg.get(key))
        if key in ('x', 'y') and fac.kind != _abi.FACTOR_UNIFORM_F32:
          raise LoweringError('%s must be a float32 Continuous factor' % key)
        if key == 'angle':
          if fac.kind == _abi.FACTOR_UNIFORM_F32 or (
              fac.kind == _abi.FACTOR_UNIFORM_INT and not 0 <= fac.lo <= fac.hi <= 360):
            raise LoweringError('angle must be Discrete or integer degrees within [0, 360]')
          for i, c in enumerate(cands or []):
            grp.cos_a[i], grp.sin_a[i] = math.cos(math.radians(c)), math.sin(math.radians(c))
        if spec.color_map == 1 and key in ('c0', 'c1', 'c2') and fac.kind == _abi.FACTOR_UNIFORM_INT:
          raise LoweringError('hsv colours must be float factors')
      grp.n_holdouts = len(self._holdouts[g])
      for i, (redrawn, box) in enumerate(self._holdouts[g]):
        ho = grp.holdouts[i]
        if 'shape' in box:
          raise LoweringError('hold-out regions over shape are not sampled on the device')
        ho.redraw_mask = sum(1 << _abi.FACTOR_ORDER.index(k) for k in redrawn if k != 'shape')
        ho.box_mask = sum(1 << _abi.FACTOR_ORDER.index(k) for k in box)
        for k, (blo, bhi) in box.items():
          ho.lo[_abi.FACTOR_ORDER.index(k)], ho.hi[_abi.FACTOR_ORDER.index(k)] = blo, bhi
        if 'shape' in redrawn:
          raise LoweringError('SetMinus over a base that includes shape is not sampled on the device')
      leaf = marg.get('shape')
      if leaf is None:
        names = [_DEFAULTS['shape']]
      elif type(leaf).__name__ == 'Discrete' and getattr(leaf, 'probs', None) is None:
        names = list(leaf.candidates)
      else:
        raise LoweringError('shape must be an unweighted Discrete factor')
      if not 1 <= len(names) <= _abi.SWB_MAX_CANDIDATES:
        raise LoweringError('shape: 1..%d candidates' % _abi.SWB_MAX_CANDIDATES)
      grp.n_shapes = len(names)
      for i, name in enumerate(names):
        grp.shapes[i] = _shapes.shape_index(name)
      for t, sub in enumerate(subs):
        grp.label[t] = self._group_label(sub, dist, marg)
    return spec


# ------------------------------------------------------------------------------ any distribution tree
def _keys_of(dist):
  keys = dist.keys
  return set(keys() if callable(keys) else keys)


def _cdf(probs, n, what):
  """numpy's choice(n, p=probs): p.cumsum() / sum; None: equal weights."""
  p = np.ones(n) / n if probs is None else np.array(probs, dtype=np.float64)
  if p.shape != (n,) or not (p >= 0).all() or not p.sum() > 0:
    raise LoweringError('%s: %d non-negative weights with a positive sum are needed' % (what, n))
  cdf = p.cumsum()
  cdf /= cdf[-1]
  return cdf


def _python_number(v, what):
  """Bounds and candidates are Python numbers (or np.float64): under NEP 50 an np.float32 one would turn comparisons with
  Python values into float32 ones."""
  if type(v) in (float, int) or isinstance(v, np.float64):
    return v
  raise LoweringError('%s must be Python floats or ints (got %s)' % (what, type(v).__name__))


class _TreeLowering(object):
  """Builds the leaves, predicates and programs of an _abi.SwbTreeSampler from distribution objects (the reference's classes or
  the mirrors: lowering is duck-typed by class name, as everywhere)."""

  def __init__(self, color_map):
    self.color_map = color_map
    self.leaves, self.leaf_index = [], {}
    self.pred_nodes, self.preds, self.pred_index = [], [], {}
    self.ops, self.choices = [], []

  # ------------------------------------------------------------ leaves
  def leaf(self, d):
    if id(d) in self.leaf_index:
      return self.leaf_index[id(d)]
    key = d.key
    if key not in _abi.TREE_FACTOR_ORDER:
      raise LoweringError('unknown sprite factors %s' % [key])
    lf = _abi.SwbTreeLeaf()
    lf.factor = _abi.TREE_FACTOR_ORDER.index(key)
    if type(d).__name__ == 'Continuous':
      if key == 'shape':
        raise LoweringError('shape must be a Discrete factor')
      dt = np.dtype(d.dtype)
      lf.kind = _abi.FACTOR_UNIFORM_INT if dt.kind in 'iu' else _abi.FACTOR_UNIFORM_F32
      lo, hi = _python_number(d.minval, 'factor %s: Continuous bounds' % key), _python_number(d.maxval, 'factor %s: Continuous bounds' % key)
      lf.lo, lf.hi = float(lo), float(hi)
      lf.lo32, lf.hi32 = _threshold(lo, True), _threshold(hi, True)
    else:
      cands = list(d.candidates)
      if not 1 <= len(cands) <= _abi.SWB_MAX_CANDIDATES:
        raise LoweringError('factor %s: 1..%d candidates' % (key, _abi.SWB_MAX_CANDIDATES))
      lf.kind, lf.n = _abi.FACTOR_DISCRETE, len(cands)
      if key == 'shape':
        cands = [_shapes.shape_index(name) for name in cands]
        lf.shape_mask = sum(1 << i for i in set(cands))
      else:
        cands = [_python_number(c, 'factor %s: Discrete candidates' % key) for c in cands]
      for i, c in enumerate(cands):
        lf.cand[i], lf.cand32[i] = float(c), float(np.float32(c))
        if key == 'angle':
          lf.cos_a[i], lf.sin_a[i] = math.cos(math.radians(c)), math.sin(math.radians(c))
      if getattr(d, 'probs', None) is not None:
        lf.weighted = 1
        for i, c in enumerate(_cdf(d.probs, len(cands), 'factor %s' % key)):
          lf.cdf[i] = c
    if len(self.leaves) >= _abi.SWB_TREE_MAX_LEAVES:
      raise LoweringError('the generator and the task need more than %d Continuous / Discrete leaves' % _abi.SWB_TREE_MAX_LEAVES)
    self.leaves.append((lf, d))     # (the object is kept: ids stay unique while the index is in use)
    self.leaf_index[id(d)] = len(self.leaves) - 1
    return self.leaf_index[id(d)]

  # ------------------------------------------------------------ contains() -> postfix predicates
  def _contains(self, d, depth):
    """Appends the nodes of d.contains(); returns the deepest the stack gets, starting from `depth` values on it."""
    name = type(d).__name__
    push = lambda op, leaf=0: self.pred_nodes.append((op, leaf))
    if name in ('Continuous', 'Discrete'):
      push(_abi.PRED_LEAF, self.leaf(d))
      return depth + 1
    if name in ('Product', 'Intersection', 'Mixture'):
      kids, op = list(d.components), (_abi.PRED_OR if name == 'Mixture' else _abi.PRED_AND)
      if not kids and name == 'Mixture':
        raise LoweringError('a Mixture needs components')
    elif name == 'SetMinus':
      kids, op = [getattr(d, 'base', None) or d.hold_in, d.hold_out], _abi.PRED_ANDNOT
    elif name == 'Selection':
      kids, op = [d.base, d.filtering], _abi.PRED_AND
    else:
      raise LoweringError('%s is not a factor distribution the device evaluates (Continuous / Discrete / Product / Mixture / '
                          'Intersection / SetMinus / Selection)' % name)
    if not kids:
      push(_abi.PRED_TRUE)
      return depth + 1
    deepest = self._contains(kids[0], depth)
    for kid in kids[1:]:
      deepest = max(deepest, self._contains(kid, depth + 1))
      push(op)
    return deepest

  def pred(self, dists):
    """Index of the predicate `all(d.contains(factors) for d in dists)`."""
    key = tuple(id(d) for d in dists)
    if key in self.pred_index:
      return self.pred_index[key]
    first, deepest = len(self.pred_nodes), 0
    for i, d in enumerate(dists):
      deepest = max(deepest, self._contains(d, min(i, 1)))
      if i:
        self.pred_nodes.append((_abi.PRED_AND, 0))
    if deepest > _abi.SWB_TREE_MAX_STACK:
      raise LoweringError('a distribution nests %d deep: predicates are evaluated on a stack of %d' % (deepest, _abi.SWB_TREE_MAX_STACK))
    if len(self.pred_nodes) > _abi.SWB_TREE_MAX_PRED_NODES:
      raise LoweringError('the generator and the task need more than %d predicate nodes' % _abi.SWB_TREE_MAX_PRED_NODES)
    if len(self.preds) >= _abi.SWB_TREE_MAX_PREDS:
      raise LoweringError('the generator and the task need more than %d predicates' % _abi.SWB_TREE_MAX_PREDS)
    self.preds.append((first, len(self.pred_nodes) - first, dists))
    self.pred_index[key] = len(self.preds) - 1
    return self.pred_index[key]

  # ------------------------------------------------------------ sample() -> bytecode
  def _drawn_leaf(self, d):
    i = self.leaf(d)
    lf, key = self.leaves[i][0], d.key
    if type(d).__name__ == 'Continuous':
      dt = np.dtype(d.dtype)
      if dt != np.float32 and dt.kind not in 'iu':
        raise LoweringError('factor %s: dtype %s is not sampled on the device' % (key, dt))
    if key in ('x', 'y') and lf.kind != _abi.FACTOR_UNIFORM_F32:
      raise LoweringError('%s must be a float32 Continuous factor' % key)
    if key == 'angle':
      if lf.kind == _abi.FACTOR_UNIFORM_F32:
        raise LoweringError('angle must be Discrete or integer degrees within [0, 360]: the kernel has no bit-exact cos / sin '
                            'of a float32 angle')
      if lf.kind == _abi.FACTOR_UNIFORM_INT and not 0 <= lf.lo <= lf.hi <= 360:
        raise LoweringError('angle must be Discrete or integer degrees within [0, 360]')
    if self.color_map == 1 and key in ('c0', 'c1', 'c2') and lf.kind == _abi.FACTOR_UNIFORM_INT:
      raise LoweringError('hsv colours must be float factors')
    return i

  def sample(self, d):
    """Appends the ops of d.sample(), in the order the reference draws."""
    name = type(d).__name__
    emit = lambda *op: self.ops.append(list(op) + [0] * (4 - len(op)))
    if name in ('Continuous', 'Discrete'):
      emit(_abi.OP_DRAW, self._drawn_leaf(d))
    elif name == 'Product':
      for c in d.components:
        self.sample(c)
    elif name == 'Mixture':
      kids = list(d.components)
      if not 1 <= len(kids) <= _abi.SWB_MAX_CANDIDATES:
        raise LoweringError('a Mixture takes 1..%d components' % _abi.SWB_MAX_CANDIDATES)
      if len(self.choices) >= _abi.SWB_TREE_MAX_CHOICES:
        raise LoweringError('at most %d Mixture nodes' % _abi.SWB_TREE_MAX_CHOICES)
      choice = {'cdf': _cdf(getattr(d, 'probs', None), len(kids), 'Mixture'), 'target': []}
      self.choices.append(choice)
      emit(_abi.OP_CHOOSE, len(self.choices) - 1)
      jumps = []
      for c in kids:
        choice['target'].append(len(self.ops))
        self.sample(c)
        jumps.append(len(self.ops))
        emit(_abi.OP_JUMP, 0)
      for j in jumps:
        self.ops[j][1] = len(self.ops)
    elif name in ('Intersection', 'SetMinus', 'Selection'):
      start = len(self.ops)
      if name == 'Intersection':
        index = getattr(d, 'index_for_sampling', getattr(d, 'index', 0))
        self.sample(d.components[index])
        emit(_abi.OP_TEST, self.pred(list(d.components)), 1, start)
      elif name == 'SetMinus':
        self.sample(getattr(d, 'base', None) or d.hold_in)
        emit(_abi.OP_TEST, self.pred([d.hold_out]), 0, start)
      else:
        self.sample(d.base)
        emit(_abi.OP_TEST, self.pred([d.filtering]), 1, start)
    else:
      raise LoweringError('%s cannot be sampled on the device (Continuous / Discrete / Product / Mixture / Intersection / '
                          'SetMinus / Selection)' % name)
    if len(self.ops) > _abi.SWB_TREE_MAX_OPS:
      raise LoweringError('the generator needs more than %d sampling ops' % _abi.SWB_TREE_MAX_OPS)

  def fill(self, spec):
    spec.n_leaves, spec.n_pred_nodes, spec.n_preds = len(self.leaves), len(self.pred_nodes), len(self.preds)
    spec.n_ops, spec.n_choices = len(self.ops), len(self.choices)
    for i, (lf, _) in enumerate(self.leaves):
      spec.leaves[i] = lf
    for i, (op, leaf) in enumerate(self.pred_nodes):
      spec.pred_nodes[i].op, spec.pred_nodes[i].leaf = op, leaf
    for i, (first, n, _) in enumerate(self.preds):
      spec.preds[i].first, spec.preds[i].n = first, n
    for i, op in enumerate(self.ops):
      spec.ops[i].kind, spec.ops[i].a, spec.ops[i].b, spec.ops[i].c = op
    for i, choice in enumerate(self.choices):
      spec.choices[i].n = len(choice['target'])
      for k, (t, c) in enumerate(zip(choice['target'], choice['cdf'])):
        spec.choices[i].target[k], spec.choices[i].cdf[k] = t, c


class TreeSampler(_GroupSampler):
  """DeviceSampler's surface for ANY tree of factor distributions (Mixture, Intersection, Selection, nested SetMinus, hold-outs
  of any form, weighted Discrete) and any task -- labels are evaluated per sprite on the device, tasks that key on position
  included (swb_sample_pool_tree).  `alternative_probs`: the `p` of sprite_generators.sample_generator.  `max_tries`: rejections
  one sprite may use up in all its loops together (the reference raises after _MAX_TRIES = 10000 per loop); sprites that run
  out keep their last draw and BatchedEnvironment.check() raises."""

  def __init__(self, groups, shuffle=False, seed=0, alternatives=None, alternative_probs=None, max_tries=_abi.SWB_TREE_DEFAULT_MAX_TRIES):
    self.groups = [(dist,) + _count_range(count) for dist, count in groups]
    self._set_layout(shuffle, seed, alternatives)
    if alternative_probs is not None:
      if self.alternatives is None:
        raise ValueError('alternative_probs without alternatives')
      alternative_probs = _cdf(alternative_probs, len(self.alternatives), 'alternative_probs')
      alternative_probs = np.diff(alternative_probs, prepend=0.)      # (normalised: what np.random.choice wants on the host)
    self.alternative_probs = alternative_probs
    self.max_tries = int(max_tries)
    if self.max_tries < 1:
      raise ValueError('max_tries must be >= 1')

  def lower(self, task, renderers):
    """_abi.SwbTreeSampler for swb_sample_pool_tree; LoweringError for what the kernel does not draw bit-exactly."""
    from spriteworld_amd import lowering
    spec = _abi.SwbTreeSampler()
    spec.n_groups, spec.shuffle, spec.max_tries = len(self.groups), self.shuffle, self.max_tries
    spec.n_alternatives = 0 if self.alternatives is None else len(self.alternatives)
    for i, lst in enumerate(self.alternatives or []):
      spec.alternatives[i].n = len(lst)
      for j, g in enumerate(lst):
        spec.alternatives[i].group[j] = g
    if self.alternative_probs is not None:
      spec.alternatives_weighted = 1
      for i, c in enumerate(_cdf(self.alternative_probs, len(self.alternatives), 'alternative_probs')):
        spec.alternative_cdf[i] = c
    spec.color_map = _color_map_of(renderers)
    for d in range(360):  # sprite.py:147-151 rotates by radians of the stored degrees
      spec.deg_cos[d], spec.deg_sin[d] = math.cos(math.radians(d)), math.sin(math.radians(d))
    low = _TreeLowering(spec.color_map)
    for g, (dist, lo, hi) in enumerate(self.groups):
      grp = spec.groups[g]
      grp.count_min, grp.count_max = lo, hi
      keys = _keys_of(dist)
      unknown = keys - set(_abi.TREE_FACTOR_ORDER)
      if unknown:
        raise LoweringError('unknown sprite factors %s' % sorted(unknown))
      for key in ('x', 'y'):
        if key not in keys:
          raise LoweringError('%s must be a float32 Continuous factor' % key)
      grp.first_op = len(low.ops)
      low.sample(dist)
      grp.n_ops = len(low.ops) - grp.first_op
      for i, key in enumerate(_abi.TREE_FACTOR_ORDER):
        grp.defaults[i] = _shapes.shape_index(_DEFAULTS[key]) if key == 'shape' else float(_DEFAULTS[key])
      grp.default_cos, grp.default_sin = math.cos(math.radians(_DEFAULTS['angle'])), math.sin(math.radians(_DEFAULTS['angle']))
    subs = subtasks_of(task)
    spec.n_tasks = len(subs)
    kinds = {'NoReward': _abi.TASK_NO_REWARD, 'FindGoalPosition': _abi.TASK_FIND_GOAL, 'Clustering': _abi.TASK_CLUSTERING}
    for t, sub in enumerate(subs):
      if type(sub).__name__ not in kinds:
        raise LoweringError('unsupported task type: ' + type(sub).__name__)
      lowering.position_cuts(sub, True)        # (refuses what the position grid cannot express: a Discrete over x / y)
      dists = lowering._task_distribs(sub)
      if len(dists) > _abi.SWB_TREE_MAX_CLUSTERS:
        raise LoweringError('a Clustering task of %d clusters (at most %d)' % (len(dists), _abi.SWB_TREE_MAX_CLUSTERS))
      spec.tasks[t].kind, spec.tasks[t].n_preds = kinds[type(sub).__name__], len(dists)
      for k, d in enumerate(dists):
        spec.tasks[t].pred[k] = low.pred([d])
    low.fill(spec)
    spec._keepalive = low                      # (ids of the distribution objects index the leaves)
    return spec


def _color_map_of(renderers):
  """swb_sampler::color_map of the PILRenderer's color_to_rgb: 0 identity, 1 hsv_to_rgb."""
  from spriteworld_amd import lowering
  _, pil = lowering.find_pil_renderer(renderers)
  to_rgb = getattr(pil, '_color_to_rgb', None) if pil is not None else None
  probe = (0.3, 0.6, 0.9)
  if to_rgb is None or tuple(to_rgb(probe)) == probe:
    return 0
  if getattr(to_rgb, '__name__', '') == 'hsv_to_rgb':
    return 1
  raise LoweringError('color_to_rgb %r is not available on the device (identity or hsv_to_rgb)' % (to_rgb,))


# ------------------------------------------------------------------------------ closures -> sampler
def _closure(fn):
  return dict(zip(fn.__code__.co_freevars, (c.cell_contents for c in fn.__closure__ or ())))


def _count_of(num_sprites):
  """int, or the (lo, hi) of a `lambda: np.random.randint(lo, hi)` (cobra/exploration.py:58)."""
  if not callable(num_sprites):
    return int(num_sprites)
  code = getattr(num_sprites, '__code__', None)
  if code is not None and code.co_argcount == 0 and code.co_names[-1:] == ('randint',):
    ints = [c for c in code.co_consts if isinstance(c, int) and not isinstance(c, bool)]
    if len(ints) == 2 and not num_sprites.__closure__:
      return (ints[0], ints[1])
  raise LoweringError('num_sprites callable is not a plain `lambda: np.random.randint(lo, hi)`')


def _flatten(fn, weights=None):
  """Generator closure -> (groups, n_leading_groups_shuffled or None, alternatives or None).  `weights`: a list that takes the
  `p` of a weighted sample_generator (None: a weighted one is refused)."""
  kind = getattr(fn, '__qualname__', '').split('.')[0]
  cells = _closure(fn) if getattr(fn, '__code__', None) is not None else {}
  if kind == 'generate_sprites':
    return [(cells['factor_dist'], _count_of(cells['num_sprites']))], None, None
  if kind == 'shuffle':
    groups, inner, alts = _flatten(cells.get('sprite_generator', cells.get('generator')), weights)
    if inner is not None:
      raise LoweringError('shuffle of an already shuffled generator is not sampled on the device')
    return groups, _abi.SWB_MAX_GROUPS, alts
  if kind == 'chain_generators':
    gens = cells.get('sprite_generators', cells.get('generators'))
    groups, shuffled = [], None
    for i, g in enumerate(gens):
      sub, sh, alts = _flatten(g)
      if alts is not None:
        raise LoweringError('sample_generator inside chain_generators is not sampled on the device')
      if sh is not None:
        if i != 0:
          raise LoweringError('only a leading shuffled sub-generator is sampled on the device')
        shuffled = len(sub)
      groups.extend(sub)
    return groups, shuffled, None
  if kind == 'sample_generator':
    if cells.get('p') is not None:
      if weights is None:
        raise LoweringError('weighted sample_generator is not sampled on the device')
      weights.extend(cells['p'])
    groups, alts, seen = [], [], {}
    for g in cells.get('sprite_generators', cells.get('generators')):
      sub, sh, inner = _flatten(g)
      if sh is not None or inner is not None:
        raise LoweringError('nested shuffle / sample_generator is not sampled on the device')
      lst = []
      for dist, count in sub:                  # the same (distribution, count) is one group
        key = (id(dist), count)
        if key not in seen:
          seen[key] = len(groups)
          groups.append((dist, count))
        lst.append(seen[key])
      alts.append(lst)
    return groups, None, alts
  raise LoweringError('%r is not built from generate_sprites / chain_generators / sample_generator / shuffle' % (fn,))


def from_generator(init_sprites, seed=0, tree=False):
  """DeviceSampler equivalent to a generator built with the reference's (or this package's)
  `sprite_generators.generate_sprites / chain_generators / sample_generator / shuffle`, by reading
  their closures.  Raises LoweringError for anything else (hand-written callables, weighted
  choices, ...).  `tree`: a TreeSampler instead, which takes what DeviceSampler refuses at construction or in
  lower(): any tree of distributions, a weighted sample_generator, tasks that select by a drawn value or key on position."""
  if isinstance(init_sprites, _GroupSampler):
    return init_sprites
  if not tree:
    groups, shuffled, alts = _flatten(init_sprites)
    return DeviceSampler(groups, shuffle=shuffled or 0, seed=seed, alternatives=alts)
  weights = []
  groups, shuffled, alts = _flatten(init_sprites, weights)
  return TreeSampler(groups, shuffle=shuffled or 0, seed=seed, alternatives=alts, alternative_probs=weights or None)
