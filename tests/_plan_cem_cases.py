"""Scenarios of BatchedEnvironment.plan_cem (a cross-entropy-method planner over rollout_guided), shared by the emulated suite
(tests/test_plan_cem.py) and the GPU suite (tests/test_gpu_plan_cem.py): N = 4 environments, M = 8 candidates, K = 4 steps,
I = 3 rounds, on the scenes of the goal_s5 and embodied_s12 workloads at a 16 x 16 frame.  The engine class is
environment._engine.Engine: the caller has patched the emulated one in, or runs on the GPU.  TEST INFRASTRUCTURE ONLY."""
import contextlib

import numpy as np
import torch

from spriteworld_amd import _abi
from tests import _parity

_bits = _parity.bits
N, M, K, I = 4, 8, 4, 3
NAMES = ('goal_s5', 'embodied_s12')
# |torch std - numpy std| of the refit, float64, population form, E = 3 values in [0, 1].  torch reduces with Welford's update,
# numpy in two passes; both are backward stable, so each is within a few units of 2^-53 times the largest value (1) of the exact
# deviation.  Measured on the CPU over 2 * 10^5 uniform triples and 2 * 10^5 triples within 1e-9 of each other (the elites of a
# converged plan) by tests/test_plan_cem.py::test_cem_refit_std_bound_is_what_this_cpu_measures: the largest difference was
# 1.11e-16 = 2^-53.  The bound is 8 * 2^-53, eight times that.
STD_BOUND = 8.0 * 2.0 ** -53


def make_env(name, n_envs=N, **kw):
  """The scene of workloads.build(name) as a BatchedEnvironment drawn by sprite generators: goal_s5 -- two targets (c0 < 0.4)
  and three distractors, SelectMove(scale 0.25), FindGoalPosition on the targets; embodied_s12 -- eleven sprites and the body
  circle, Embodied(step 0.05), FindGoalPosition."""
  from spriteworld_amd import action_spaces, environment, renderers, sprite_generators, tasks
  from spriteworld_amd import factor_distributions as distribs
  rend = {'image': renderers.PILRenderer(image_size=(16, 16), anti_aliasing=1, color_to_rgb=renderers.color_maps.hsv_to_rgb)}

  def factors(c0_low, c0_high, scale=0.15, shapes=('square', 'triangle', 'star_4')):
    return distribs.Product([
        distribs.Continuous('x', 0.1, 0.9), distribs.Continuous('y', 0.1, 0.9), distribs.Discrete('shape', list(shapes)),
        distribs.Discrete('scale', [scale]), distribs.Continuous('c0', c0_low, c0_high), distribs.Continuous('c1', 0.3, 1.),
        distribs.Continuous('c2', 0.9, 1.)])

  if name == 'goal_s5':
    init = sprite_generators.chain_generators(sprite_generators.generate_sprites(factors(0.0, 0.4), num_sprites=2),
                                              sprite_generators.generate_sprites(factors(0.5, 0.9), num_sprites=3))
    task = tasks.FindGoalPosition(filter_distrib=distribs.Continuous('c0', 0.0, 0.4), terminate_distance=0.075)
    space = action_spaces.SelectMove(scale=0.25)
  else:
    init = sprite_generators.chain_generators(sprite_generators.generate_sprites(factors(0.0, 0.9, scale=0.1), num_sprites=11),
                                              sprite_generators.generate_sprites(factors(0.95, 1.0, scale=0.07, shapes=('circle',)),
                                                                                 num_sprites=1))
    task = tasks.FindGoalPosition(filter_distrib=distribs.Continuous('c0', 0.0, 0.4), terminate_distance=0.075)
    space = action_spaces.Embodied(step_size=0.05)
  return environment.BatchedEnvironment(task=task, action_space=space, renderers=rend, init_sprites=init, max_episode_length=20,
                                        num_envs=n_envs, episodes_per_env=2, seed=7, **kw)


def started(name):
  env = make_env(name)
  env.reset()
  env.step(env.sample_actions())
  env.seed_actions(31)
  return env


def _host(t):
  return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def plan_case(name):
  """Shapes and dtypes; best_per_iteration never decreases and ends at episode_return; rollout(plan.actions[:, None]) returns
  plan.episode_return bit for bit; stepping the live batch with plan.actions[:, k] reproduces that rollout's rewards and step
  types."""
  from spriteworld_amd import environment
  env = started(name)
  e = env.engine
  embodied = e.cfg.action_space == _abi.ACTION_EMBODIED
  width, a_width = (8, 2) if embodied else (e.S, 4)
  plan = env.plan_cem(M, K, iterations=I)
  assert isinstance(plan, environment.CemPlan)
  assert tuple(plan.actions.shape) == (N, K, a_width) and plan.actions.dtype == (torch.int32 if embodied else torch.float64)
  assert tuple(plan.episode_return.shape) == (N,) and tuple(plan.best_per_iteration.shape) == (N, I)
  assert tuple(plan.sprite_weights.shape) == (N, K, width) and tuple(plan.motion_mean.shape) == tuple(plan.motion_std.shape) == (N, K, 2)
  assert all(t.device == e.device for t in plan)
  best = _host(plan.best_per_iteration)
  assert (np.diff(best, axis=1) >= 0).all(), best
  np.testing.assert_array_equal(_bits(best[:, -1]), _bits(_host(plan.episode_return)))
  weights = _host(plan.sprite_weights)
  # one elite (M // 8) per round: every row holds one vote and the floor
  np.testing.assert_array_equal(np.sort(weights, axis=-1)[..., -1], np.full((N, K), 1.0 + 0.1))
  np.testing.assert_array_equal(np.sort(weights, axis=-1)[..., :-1], np.full((N, K, width - 1), 0.1))
  if embodied:
    assert (_host(plan.motion_mean) == 0.5).all() and (_host(plan.motion_std) == 0.25).all()
  else:
    assert (_host(plan.motion_std) == 0.02).all()         # (the deviation of one elite is 0: the floor)
    assert ((_host(plan.motion_mean) >= 0) & (_host(plan.motion_mean) <= 1)).all()
  r = env.rollout(plan.actions[:, None])
  np.testing.assert_array_equal(_bits(_host(r.episode_return())[:, 0]), _bits(_host(plan.episode_return)))
  step_type, reward = _host(r.step_type)[:, 0], _host(r.reward)[:, 0]
  for k in range(K):
    ts = env.step(plan.actions[:, k])
    np.testing.assert_array_equal(_host(ts.step_type), step_type[:, k], err_msg='step type of step %d' % k)
    live = step_type[:, k] != _abi.STEP_FIRST
    np.testing.assert_array_equal(_bits(_host(ts.reward).astype(np.float64)[live]), _bits(reward[live, k]), err_msg='reward of step %d' % k)
  env.close()


def refit_case(name):
  """The refit of one round equals a numpy restatement on the same elites (three of them): weights and mean exactly, the
  deviation within STD_BOUND."""
  from spriteworld_amd import environment
  env = started(name)
  e = env.engine
  embodied = e.cfg.action_space == _abi.ACTION_EMBODIED
  width, n_elites, floor, min_std = (8 if embodied else e.S), 3, 0.25, 0.02
  r, actions, sprite = env.rollout_guided(M, K)
  top, elite = r.episode_return().topk(n_elites, dim=1)
  weights, mean, std = environment.cem_refit(actions, sprite, elite, width, floor, min_std)
  a, s, el = _host(actions), _host(sprite), _host(elite)
  want = np.full((N, K, width), floor)
  for n in range(N):
    for j in el[n]:
      for k in range(K):
        if 0 <= s[n, j, k] < width:
          want[n, k, s[n, j, k]] += 1.0
  np.testing.assert_array_equal(_bits(_host(weights)), _bits(want))
  assert (want.sum(-1) == n_elites + width * floor).all()
  if embodied:
    assert mean is None and std is None
  else:
    picked = np.stack([a[n, el[n]] for n in range(N)])[..., 2:4].astype(np.float64)      # [N, E, K, 2]
    np.testing.assert_array_equal(_bits(_host(mean)), _bits(np.add.reduce(picked, axis=1) / n_elites))
    want_std = np.maximum(picked.std(axis=1), min_std)
    diff = np.abs(_host(std) - want_std)
    print('refit: largest |std - numpy std| = %.3g (bound %.3g)' % (diff.max(), STD_BOUND))
    assert diff.max() <= STD_BOUND, diff.max()
    assert (want_std > min_std).any()
  # the same refit inside plan_cem: one round from the same key leaves these weights
  env.seed_actions(31)
  plan = env.plan_cem(M, K, iterations=1, num_elites=n_elites, weight_floor=floor, min_std=min_std)
  np.testing.assert_array_equal(_bits(_host(plan.sprite_weights)), _bits(want))
  if not embodied:
    np.testing.assert_array_equal(_bits(_host(plan.motion_mean)), _bits(_host(mean)))
    np.testing.assert_array_equal(_bits(_host(plan.motion_std)), _bits(_host(std)))
  np.testing.assert_array_equal(_bits(_host(plan.episode_return)), _bits(_host(top[:, 0])))
  env.close()


def warm_start_case(name):
  """init takes a CemPlan, or the three tensors shifted by one step (MPC); a wrong shape is refused."""
  env = started(name)
  plan = env.plan_cem(M, K, iterations=2)
  again = env.plan_cem(M, K, iterations=2, init=plan)
  assert (np.diff(_host(again.best_per_iteration), axis=1) >= 0).all()
  shift = lambda t, fill: torch.cat([t[:, 1:], torch.full_like(t[:, :1], fill)], dim=1)
  moved = env.plan_cem(M, K, iterations=1, init=(shift(plan.sprite_weights, 1.0), shift(plan.motion_mean, 0.5), shift(plan.motion_std, 0.25)))
  assert tuple(moved.actions.shape) == tuple(plan.actions.shape)
  for bad in ((plan.sprite_weights[:, :2], plan.motion_mean, plan.motion_std), (plan.sprite_weights, plan.motion_mean[..., :1], plan.motion_std)):
    try:
      env.plan_cem(M, K, init=bad)
    except ValueError as e:
      assert 'plan_cem: init' in str(e)
    else:
      raise AssertionError('plan_cem(init of a wrong shape) did not raise')
  for bad in (dict(iterations=0), dict(num_elites=0), dict(num_elites=M + 1)):
    try:
      env.plan_cem(M, K, **bad)
    except ValueError as e:
      assert 'plan_cem' in str(e)
    else:
      raise AssertionError('plan_cem(%r) did not raise' % (bad,))
  env.close()


@contextlib.contextmanager
def no_host_reads(monkeypatch):
  """Every way a tensor's value reaches Python raises while the block runs."""
  def refuse(what):
    def raiser(*args, **kw):
      raise AssertionError('plan_cem read a tensor on the host: Tensor.%s' % what)
    return raiser
  with monkeypatch.context() as mp:
    for what in ('item', 'tolist', 'cpu', 'numpy', '__bool__', '__int__', '__float__', '__index__'):
      mp.setattr(torch.Tensor, what, refuse(what))
    yield
