"""device_sampler.TreeSampler without a device: the lowering to leaves / predicates / programs, what is still refused (with the
message), the refusals of DeviceSampler that stay, and the model of tests/_sampler_tree_model.py against the distributions' own
sample() under numpy (statistics)."""
import numpy as np
import pytest

from spriteworld_amd import _abi
from spriteworld_amd import action_spaces
from spriteworld_amd import device_sampler
from spriteworld_amd import environment
from spriteworld_amd import factor_distributions as D
from spriteworld_amd import lowering
from spriteworld_amd import sprite_generators
from spriteworld_amd import tasks

from tests import _sampler_tree_cases as cases
from tests import _sampler_tree_model

XY = [D.Continuous('x', 0.1, 0.9), D.Continuous('y', 0.1, 0.9)]
TASK = tasks.FindGoalPosition(filter_distrib=D.Continuous('c0', 0., 0.4))


def _ops(spec, g=0):
  grp = spec.groups[g]
  return [(o.kind, o.a, o.b, o.c) for o in spec.ops[grp.first_op:grp.first_op + grp.n_ops]]


def test_nested_tree_lowers_to_loops_that_restart_their_inner_loops():
  sampler, task, rend = cases.CASES['nested']()
  spec = sampler.lower(task, rend)
  DRAW, TEST = _abi.OP_DRAW, _abi.OP_TEST
  ops = _ops(spec)
  assert [o[0] for o in ops] == [DRAW] * 4 + [TEST, TEST, DRAW, TEST, DRAW, DRAW, TEST]
  assert [o[2:] for o in ops if o[0] == TEST] == [(0, 0), (0, 0), (1, 6), (1, 8)]       # (accept_if, retry_pc)
  assert [_abi.TREE_FACTOR_ORDER[spec.leaves[o[1]].factor] for o in ops if o[0] == DRAW] == ['x', 'y', 'shape', 'scale', 'c0', 'c1', 'c2']
  hue = spec.leaves[ops[6][1]]
  assert (hue.lo, hue.hi) == (0.4, 1.) and (hue.lo32, hue.hi32) == (float(np.float32(0.4)), 1.)      # components[index_for_sampling = 1]
  shape_member = [lf for lf in spec.leaves[:spec.n_leaves] if lf.factor == _abi.SWB_F_SHAPE and lf.n == 2][0]
  assert shape_member.shape_mask == sum(1 << int(shape_member.cand[i]) for i in range(2))
  assert spec.max_tries == 10000 and spec.n_tasks == 1 and spec.tasks[0].n_preds == 1 and spec.color_map == 1
  assert (spec.groups[0].count_min, spec.groups[0].count_max) == (1, 3) and sampler.max_sprites == 3


def test_mixture_lowers_to_a_choice_and_weighted_leaves():
  gen, task, rend = cases.CASES['mixture']()
  sampler = device_sampler.from_generator(gen, seed=1, tree=True)
  assert isinstance(sampler, device_sampler.TreeSampler) and sampler.alternatives == [[0], [1]]
  spec = sampler.lower(task, rend)
  assert spec.alternatives_weighted == 1 and [spec.alternative_cdf[i] for i in range(2)] == [0.7, 1.0]
  ops = _ops(spec)
  assert [o[0] for o in ops] == [0, 0, _abi.OP_CHOOSE, 0, 0, _abi.OP_JUMP, 0, 0, _abi.OP_JUMP, 0, 0, 0]
  choice = spec.choices[0]
  assert choice.n == 2 and list(choice.target[:2]) == [3, 6] and list(choice.cdf[:2]) == [0.2, 1.0]
  assert ops[5][1] == ops[8][1] == 9
  scale = spec.leaves[ops[4][1]]
  assert scale.weighted == 1 and list(scale.cdf[:3]) == list(np.array([0.6, 0.3, 0.1]).cumsum() / np.array([0.6, 0.3, 0.1]).sum())
  assert spec.groups[1].first_op == 12 and spec.groups[1].n_ops == 12 and spec.n_choices == 2


def test_typed_bounds_of_a_leaf():
  """An np.float32 value meets float32(bound); an np.float64 bound promotes the comparison (lowering._threshold)."""
  group = D.Product(XY + [D.Continuous('c0', 0.7, np.float64(0.7))])
  spec = device_sampler.TreeSampler([(group, 1)]).lower(TASK, cases._rend())
  lf = [lf for lf in spec.leaves[:spec.n_leaves] if lf.factor == _abi.FACTOR_ORDER.index('c0') and lf.lo == 0.7][0]
  assert lf.lo32 == float(np.float32(0.7)) < 0.7 and lf.hi == 0.7
  assert lf.hi32 == float(np.nextafter(np.float32(0.7), np.float32(1)))       # v < float64(0.7)  <=>  v < the next float32 up
  with pytest.raises(lowering.LoweringError, match='Continuous bounds must be Python floats or ints'):
    device_sampler.TreeSampler([(D.Product(XY + [D.Continuous('c0', np.float32(0.1), 0.7)]), 1)]).lower(TASK, cases._rend())


class _Odd(object):
  keys = {'c1'}


@pytest.mark.parametrize('extra,message', [
    ([D.Continuous('angle', 0., 90.)], 'no bit-exact cos / sin'),
    ([D.Continuous('angle', 0, 400, dtype='int32')], r'integer degrees within \[0, 360\]'),
    ([D.Continuous('scale', 0.1, 0.2, dtype='float64')], 'dtype float64 is not sampled on the device'),
    ([D.Discrete('c0', [np.float32(0.5)])], 'Discrete candidates must be Python floats or ints'),
    ([D.Continuous('hue', 0., 1.)], 'unknown sprite factors'),
    ([D.Continuous('shape', 0., 1.)], 'shape must be a Discrete factor'),
    ([_Odd()], '_Odd cannot be sampled on the device'),
    ([D.Mixture([D.Continuous('c0', 0.01 * k, 0.5) for k in range(13)])], r'a Mixture takes 1\.\.12 components'),
    ([D.Discrete('c0', [0.1 * k for k in range(13)])], r'factor c0: 1\.\.12 candidates'),
    ([D.Discrete('c0', [0.1, 0.2], probs=[1., -1.])], 'non-negative weights'),
    ([D.Continuous('c0', 0, 256, dtype='int32')], 'hsv colours must be float factors'),
])
def test_what_the_tree_sampler_still_refuses(extra, message):
  with pytest.raises(lowering.LoweringError, match=message):
    device_sampler.TreeSampler([(D.Product(XY + extra), 1)]).lower(TASK, cases._rend())


def test_positions_must_be_float32_draws():
  for group in (D.Product([D.Continuous('x', 0.1, 0.9, dtype='float64'), XY[1]]), D.Product([D.Discrete('x', [0.5]), XY[1]]),
                D.Product([D.Continuous('x', 0, 2, dtype='int32'), XY[1]])):
    with pytest.raises(lowering.LoweringError, match='x must be a float32 Continuous factor|dtype float64 is not sampled'):
      device_sampler.TreeSampler([(group, 1)]).lower(TASK, cases._rend())
  with pytest.raises(lowering.LoweringError, match='y must be a float32 Continuous factor'):
    device_sampler.TreeSampler([(D.Product([XY[0], D.Continuous('c0', 0., 1.)]), 1)]).lower(TASK, cases._rend())


def test_task_filters_the_tree_sampler_refuses():
  sampler = device_sampler.TreeSampler([(D.Product(XY), 1)])
  with pytest.raises(lowering.LoweringError, match='a Discrete distribution over'):
    sampler.lower(tasks.FindGoalPosition(filter_distrib=D.Discrete('x', [0.5])), cases._rend())
  with pytest.raises(lowering.LoweringError, match='_Odd is not a factor distribution the device evaluates'):
    sampler.lower(tasks.FindGoalPosition(filter_distrib=_Odd()), cases._rend())
  with pytest.raises(lowering.LoweringError, match='17 clusters'):
    sampler.lower(tasks.Clustering([D.Continuous('c0', 0.01 * k, 1.) for k in range(17)]), cases._rend())


def test_limits_of_the_tree_sampler():
  rend = cases._rend()
  deep = D.Continuous('c0', 0., 1.)
  for _ in range(33):                   # right-nested: the stack grows by one per level
    deep = D.Intersection([D.Continuous('c1', 0., 1.), deep])
  with pytest.raises(lowering.LoweringError, match='predicates are evaluated on a stack of 32'):
    device_sampler.TreeSampler([(D.Product(XY), 1)]).lower(tasks.FindGoalPosition(filter_distrib=deep), rend)
  wide = D.Intersection([D.Continuous('c0', 0.001 * k, 1.) for k in range(70)])
  with pytest.raises(lowering.LoweringError, match='more than 64 Continuous / Discrete leaves'):
    device_sampler.TreeSampler([(D.Product(XY), 1)]).lower(tasks.FindGoalPosition(filter_distrib=wide), rend)
  leaf = D.Continuous('c0', 0., 1.)
  nest = leaf
  for _ in range(130):
    nest = D.Selection(nest, leaf)
  long = D.Product(XY + [nest])
  with pytest.raises(lowering.LoweringError, match='more than 128 sampling ops'):
    device_sampler.TreeSampler([(long, 1)]).lower(TASK, rend)
  nest = leaf
  for _ in range(17):
    nest = D.Mixture([nest])
  many = D.Product(XY + [nest])
  with pytest.raises(lowering.LoweringError, match='at most 16 Mixture nodes'):
    device_sampler.TreeSampler([(many, 1)]).lower(TASK, rend)
  with pytest.raises(ValueError, match='max_tries must be >= 1'):
    device_sampler.TreeSampler([(D.Product(XY), 1)], max_tries=0)
  with pytest.raises(lowering.LoweringError, match=r'1\.\.8 sprite groups'):
    device_sampler.TreeSampler([(D.Product(XY), 1)] * 9)


def test_device_sampler_still_refuses_what_it_refused():
  gen, task, rend = cases.CASES['hue_filter']()
  sampler = device_sampler.from_generator(gen)
  assert type(sampler) is device_sampler.DeviceSampler
  with pytest.raises(lowering.LoweringError, match='task label of a sprite group depends on the sampled factors'):
    sampler.lower(task, rend)
  gen, task, rend = cases.CASES['mixture']()
  with pytest.raises(lowering.LoweringError, match='weighted sample_generator is not sampled on the device'):
    device_sampler.from_generator(gen)
  with pytest.raises(lowering.LoweringError, match=r'Mixture cannot be sampled on the device \(Product / SetMinus / Continuous / Discrete\)'):
    device_sampler.DeviceSampler([(cases.mixture_distribution(), 2)])
  with pytest.raises(lowering.LoweringError, match='a task filter keys on position'):
    device_sampler.DeviceSampler([(cases._position_group(), 2)]).lower(cases.CASES['pos_goal']()[1], rend)


def test_device_reset_tree_raises_when_neither_sampler_lowers():
  _, task, rend = cases.CASES['hue_filter']()
  with pytest.raises(lowering.LoweringError, match='is not built from generate_sprites'):
    environment.BatchedEnvironment(task=task, action_space=action_spaces.SelectMove(), renderers=rend, init_sprites=lambda: [],
                                   device_reset='tree')


def test_selection_mirror_and_weighted_host_generators():
  sel = D.Selection(D.Product([D.Continuous('c0', 0., 1.), D.Continuous('c1', 0., 1.)]), D.Continuous('c0', 0.5, 0.6))
  assert sel.keys == {'c0', 'c1'}
  rng = np.random.RandomState(0)
  draws = [sel.sample(rng=rng) for _ in range(50)]
  assert all(0.5 <= d['c0'] < 0.6 and sel.contains(d) for d in draws) and not sel.contains({'c0': 0.7, 'c1': 0.5})
  with pytest.raises(ValueError):
    D.Selection(D.Continuous('c0', 0., 1.), D.Continuous('c1', 0., 1.))
  np.random.seed(1)
  gen = sprite_generators.sample_generator([sprite_generators.generate_sprites(D.Product(XY), n) for n in (1, 2)], p=[0.9, 0.1])
  assert 820 < sum(len(gen()) == 1 for _ in range(1000)) < 980
  sampler = device_sampler.from_generator(gen, tree=True)
  assert 820 < sum(len(sampler()) == 1 for _ in range(1000)) < 980


# ---- statistics: the model's frequencies against the distributions' own sample() under numpy
def _z(k1, n1, k2, n2):
  """Two-sample z of the shares k1 / n1 and k2 / n2 under the pooled binomial variance."""
  p = (k1 + k2) / (n1 + n2)
  return (k1 / n1 - k2 / n2) / np.sqrt(p * (1 - p) * (1 / n1 + 1 / n2))


def _model_sprites(sampler, task, rend, entries, seed):
  pool, exhausted, _ = _sampler_tree_model.sample_pool(sampler, task, rend['image']._color_to_rgb, entries, sampler.max_sprites, seed)
  assert exhausted == 0
  live = np.arange(sampler.max_sprites)[None, :] < pool['n_sprites'][:, None]
  return pool, {k: pool[k][live] for k in ('x', 'y', 'scale', 'shape')} | {'c%d' % i: pool['color'][..., i][live] for i in range(3)}


def _numpy_sprites(dist, n, seed):
  np.random.seed(seed)
  draws = [dist.sample() for _ in range(n)]
  from spriteworld_amd import shapes
  out = {k: np.array([float(d[k]) for d in draws]) for k in ('x', 'y', 'scale', 'c0', 'c1', 'c2')}
  out['shape'] = np.array([shapes.shape_index(d['shape']) for d in draws])
  return out


def _assert_shares_agree(model, numpy_, events):
  """|z| <= 5 for every event: under the null the two-sample z is standard normal whatever the sizes, so a bound of 5 fails a
  correct sampler with probability 6e-7 per event -- and the seeds are fixed, so the outcome is deterministic."""
  for name, event in events.items():
    a, b = event(model), event(numpy_)
    assert 0 < b.sum() < len(b), name
    z = _z(a.sum(), len(a), b.sum(), len(b))
    assert abs(z) <= 5, (name, z, a.mean(), b.mean())


def test_mixture_model_draws_the_distribution_numpy_draws():
  gen, task, rend = cases.CASES['mixture']()
  sampler = device_sampler.from_generator(gen, seed=1, tree=True)
  pool, model = _model_sprites(sampler, task, rend, 500, seed=2024)
  numpy_ = _numpy_sprites(cases.mixture_distribution(), 6000, seed=7)
  from spriteworld_amd import shapes
  events = {'warm component': lambda s: s['c0'] < 0.3, 'scale 0.1': lambda s: s['scale'] == 0.1, 'scale 0.15': lambda s: s['scale'] == 0.15,
            'scale 0.2': lambda s: s['scale'] == 0.2, 'square': lambda s: s['shape'] == shapes.shape_index('square'),
            'circle': lambda s: s['shape'] == shapes.shape_index('circle'), 'x < 0.5': lambda s: s['x'] < 0.5,
            'c0 in the lower half of its component': lambda s: (s['c0'] < 0.1) | ((s['c0'] >= 0.5) & (s['c0'] < 0.6)), 'c1 < 0.65': lambda s: s['c1'] < 0.65}
  _assert_shares_agree(model, numpy_, events)
  np.random.seed(3)
  host = np.array([len(gen()) for _ in range(4000)])
  assert abs(_z((pool['n_sprites'] == 2).sum(), 500, (host == 2).sum(), 4000)) <= 5


def test_nested_model_draws_the_distribution_numpy_draws():
  sampler, task, rend = cases.CASES['nested']()
  _, model = _model_sprites(sampler, task, rend, 500, seed=2025)
  numpy_ = _numpy_sprites(cases.nested_distribution()[0], 4000, seed=8)
  from spriteworld_amd import shapes
  events = {'x < 0.3': lambda s: s['x'] < 0.3, 'y < 0.3': lambda s: s['y'] < 0.3, 'x < 0.2': lambda s: s['x'] < 0.2,
            'square': lambda s: s['shape'] == shapes.shape_index('square'), 'triangle': lambda s: s['shape'] == shapes.shape_index('triangle'),
            'scale < 0.15': lambda s: s['scale'] < 0.15, 'scale < 0.1': lambda s: s['scale'] < 0.1, 'c0 < 0.5': lambda s: s['c0'] < 0.5,
            'c1 < 0.8': lambda s: s['c1'] < 0.8, 'c2 < 0.75': lambda s: s['c2'] < 0.75}
  _assert_shares_agree(model, numpy_, events)
  assert model['c0'].min() >= np.float32(0.4) and model['c0'].max() < 0.6 and model['c1'].min() >= np.float32(0.6)
  inside = (model['x'] >= np.float32(0.3)) & (model['y'] >= np.float32(0.3))
  assert not inside.any() and not ((model['shape'] != shapes.shape_index('square')) & (model['scale'] < 0.15)).any()


def test_tree_struct_layouts_match_the_header(tmp_path):
  import ctypes
  import os
  import subprocess
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  names = ('swb_tree_leaf', 'swb_pred_node', 'swb_tree_pred', 'swb_tree_op', 'swb_tree_choice', 'swb_tree_group', 'swb_tree_task',
           'swb_tree_sampler')
  src = tmp_path / 'sizes.c'
  src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "swb.h"\nint main(void) {\n' +
                 ''.join('  printf("%%zu\\n", sizeof(%s));\n' % n for n in names) +
                 '  printf("%zu %zu %zu\\n", offsetof(swb_tree_sampler, groups), offsetof(swb_tree_sampler, ops), offsetof(swb_tree_sampler, leaves));\n'
                 '  return 0;\n}\n')
  exe = tmp_path / 'sizes'
  subprocess.check_call(['gcc', '-I', os.path.join(root, 'include'), '-o', str(exe), str(src)])
  out = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
  mirrors = (_abi.SwbTreeLeaf, _abi.SwbPredNode, _abi.SwbTreePred, _abi.SwbTreeOp, _abi.SwbTreeChoice, _abi.SwbTreeGroup, _abi.SwbTreeTask,
             _abi.SwbTreeSampler)
  assert out == [ctypes.sizeof(m) for m in mirrors] + [getattr(_abi.SwbTreeSampler, f).offset for f in ('groups', 'ops', 'leaves')]
