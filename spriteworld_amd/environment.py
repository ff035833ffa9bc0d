"""Batched Spriteworld environment on MI355X behind the reference's dm_env surface.

`BatchedEnvironment(task, action_space, renderers, init_sprites, keep_in_frame,
max_episode_length, metadata, num_envs=N)` takes exactly the keyword arguments of
the reference's `Environment` (reference: spriteworld/environment.py:34-72), i.e.
the dict a config's `get_config()` returns, plus `num_envs`.  `reset()` /
`step(actions)` / `observation_spec()` / `action_spec()` / `.action_space` follow
:74-161 with a leading N axis on every array:

  step_type u8[N] (0 FIRST, 1 MID, 2 LAST), reward f64[N] (NaN where the
  reference returns None, i.e. on FIRST steps), discount f32[N] (NaN on FIRST),
  observation {name: tensor}: the PILRenderer's key -> u8[N, H, W, 3] (device
  tensor), a `Success` renderer's key -> bool[N].

Per-environment auto-reset is the reference's: the step after a LAST step
ignores its action and returns FIRST (:90-91).  Where new episodes come from:

  * `device_reset='auto'` (default): when `init_sprites` was built with
    sprite_generators.* from Product / SetMinus / Continuous / Discrete
    distributions (every shipped config), episodes are drawn ON THE DEVICE
    (device_sampler, Philox streams keyed by `seed`) and the idle pool entries
    are redrawn every `refresh_every` steps, so an environment never meets an
    episode twice -- the reference's "fresh init_sprites() at every reset";
  * `device_reset='tree'`: the same, and generators or tasks that path refuses
    (Mixture / Intersection / Selection, any SetMinus, weighted choices, tasks
    that select by a drawn value or key on position) are drawn on the device
    too, by device_sampler.TreeSampler; LoweringError if neither lowers;
  * otherwise (opaque `init_sprites` callables) the pool holds
    `episodes_per_env` host draws per environment and each environment CYCLES
    through them: a long run replays these episodes until `refill_pool()` is
    called (which restarts every environment).  Use a declarative generator, or
    raise `episodes_per_env`, for training runs.

The tensors of a returned time step (observation, reward, ...) are the engine's
output buffers: the next `step()` overwrites them in place; clone what must
outlive a step (e.g. `obs` vs `next_obs`).

`Environment` is the N = 1 form returning `dm_env.TimeStep`s of numpy values, a
drop-in for the reference class in `example_run_loop.py:62-80`.
"""
import collections

import numpy as np
import torch

from spriteworld_amd import _abi
from spriteworld_amd import device_sampler
from spriteworld_amd import dm_env_compat as dm_env
from spriteworld_amd import engine as _engine
from spriteworld_amd import lowering

BatchedTimeStep = collections.namedtuple('BatchedTimeStep',
                                         ['step_type', 'reward', 'discount', 'observation'])


class Rollout(collections.namedtuple('Rollout', ['step_type', 'reward', 'discount', 'success', 'x', 'y', 'n_sprites', 'error'])):
  """What `BatchedEnvironment.rollout` returns, device tensors: step_type u8, reward f64 (NaN on FIRST steps), discount f32,
  success u8 -- [N, M, K] views, entry [n, m, k] what step k + 1 of environment n would return under candidate m -- then
  x, y f64[N, M, S] and n_sprites i32[N, M] after step K, and error u8[N, M] (swb_env_error bits of the K steps)."""
  __slots__ = ()

  def episode_return(self):
    """f64[N, M]: the sum of rewards from step 0 through the candidate's first LAST step (all K steps when it never ends);
    the NaN of FIRST steps is left out.  Torch operations on the device, no synchronisation."""
    last = (self.step_type == _abi.STEP_LAST).to(torch.int32)
    ended_before = torch.cumsum(last, dim=2) - last          # LAST steps strictly before step k
    keep = (ended_before == 0) & (self.step_type != _abi.STEP_FIRST)
    return torch.where(keep, self.reward, torch.zeros_like(self.reward)).sum(dim=2)


# What `BatchedEnvironment.rollout_positions` returns, device tensors in the planner's layout: x, y f64[N, M, K, S] and n_sprites
# i32[N, M, K] views, entry [n, m, k] the sprites of environment n after step k + 1 of candidate m.
RolloutSteps = collections.namedtuple('RolloutSteps', ['x', 'y', 'n_sprites'])

# What `BatchedEnvironment.plan_cem` returns, device tensors: actions [N, K, A] and episode_return f64[N] of the best sequence found
# per environment, best_per_iteration f64[N, I] (the best return known after each round: never decreasing), and the plan
# distribution after the last refit -- sprite_weights f64[N, K, W], motion_mean, motion_std f64[N, K, 2] --, which `init=` takes.
CemPlan = collections.namedtuple('CemPlan', ['actions', 'episode_return', 'best_per_iteration', 'sprite_weights', 'motion_mean',
                                             'motion_std'])


def cem_refit(actions, sprite, elite, width, weight_floor, min_std):
  """One refit of `plan_cem`: actions [N, M, K, A] and sprite i32[N, M, K] as `rollout_guided` returns them, elite int64[N, E]
  the candidates to fit -> (sprite_weights f64[N, K, width], motion_mean, motion_std f64[N, K, 2]).  Weights: the number of
  elites that picked sprite j at step k (indices outside [0, width) pick none) plus `weight_floor`.  Motion: the elites'
  population mean and standard deviation (divisor E) of actions[..., 2:4], the deviation at least `min_std`; for Embodied
  actions (A = 2) mean and deviation are None.  Torch operations on the tensors' device, no synchronisation."""
  N, E = elite.shape
  rows = torch.arange(N, device=elite.device)[:, None]
  picked = sprite[rows, elite].permute(0, 2, 1).to(torch.int64)          # [N, K, E]
  valid = (picked >= 0) & (picked < width)
  counts = torch.zeros((N, picked.shape[1], width), dtype=torch.float64, device=elite.device)
  counts.scatter_add_(2, picked.clamp(0, width - 1), valid.to(torch.float64))
  weights = counts + weight_floor
  if actions.shape[-1] != 4:
    return weights, None, None
  motion = actions[rows, elite][..., 2:4].to(torch.float64)              # [N, E, K, 2]
  # (the sum divided by a device tensor: mean(), and a division by a Python number, multiply by a rounded 1 / E on the device,
  # which a restatement elsewhere does not reproduce)
  count = torch.full((), float(E), dtype=torch.float64, device=elite.device)
  return weights, motion.sum(dim=1) / count, motion.std(dim=1, unbiased=False).clamp_min(min_std)


# What `BatchedEnvironment.run_episodes` returns, device tensors [N]: episode_return f64 (the rewards of the environment's active
# non-FIRST steps, summed in step order), length i64 (how many such steps), episodes i32 (LAST steps seen) and success bool (the
# success flag of its most recent LAST step).
EpisodeStats = collections.namedtuple('EpisodeStats', ['episode_return', 'length', 'episodes', 'success'])


_ACTION_KEY_DOMAIN = 0xA5A5C3D2E1F00F1E      # folded into the seed of the device action stream (_next_action_seed)

# What `BatchedEnvironment.sample_contained_positions` returns, device tensors: position f64[N, 2], sprite i32[N], tries i32[N].
ContainedPositions = collections.namedtuple('ContainedPositions', ['position', 'sprite', 'tries'])


class EnvironmentError_(RuntimeError):
  pass


class BatchedEnvironment(object):
  """N independent Spriteworld environments stepped by the HIP engine (two kernels per step, csrc/swb_kernels.hip.inc)."""

  @classmethod
  def from_configs(cls, configs, num_envs, task_set_of_entry='cycle', **kwargs):
    """One BatchedEnvironment whose episodes are played under the tasks of several reference-style config dicts (`task`,
    `action_space`, `renderers`, `init_sprites`, optionally `keep_in_frame`, `max_episode_length`, `metadata`): multi-task
    training in one batch.  The dicts must agree on the action space (class and parameters), the renderers and keep_in_frame
    -- LoweringError names the field otherwise -- and may differ in `task`, `init_sprites` and `max_episode_length`.
    task_set_of_entry: which config entry k of environment n is played under -- 'cycle': (n + k) mod G; 'per_env': n mod G; or
    an int array [num_envs, episodes_per_env].
    Where every config shares ONE `init_sprites` object the episodes are drawn on the device as for a single config
    (`device_reset`: 'auto', True or 'tree'), the sampler lowered against the sub-tasks of all configs, and the pool is
    refreshed as usual.  Otherwise entry (n, k) is drawn on the host from its own config's `init_sprites`: 'auto' does that
    silently, True / 'tree' raise LoweringError.  Either way every entry is labelled for every config's task.
    `task_sets()` says which config every environment is playing now, `set_task_set_of_entry()` changes the assignment;
    resets, masked steps, snapshots, `fork` and `run_episodes` work unchanged, the rollouts and `plan_cem` raise.
    kwargs: the other arguments of the constructor (episodes_per_env, device, check_errors, action_dtype, ...)."""
    configs = [dict(c) for c in configs]
    if not 1 <= len(configs) <= _abi.SWB_MAX_TASK_SETS:
      raise lowering.LoweringError('between 1 and %d configs supported, got %d' % (_abi.SWB_MAX_TASK_SETS, len(configs)))
    lowering.check_shared_config(configs)
    first = configs[0]
    device_reset = kwargs.pop('device_reset', 'auto')
    if not all(c['init_sprites'] is first['init_sprites'] for c in configs):
      if device_reset not in ('auto', False, None, 0):
        raise lowering.LoweringError('device-side reset sampling under task sets needs every config to share one init_sprites '
                                     'object; these draw from different ones (device_reset=\'auto\' samples them on the host)')
      device_reset = False
    which = lowering.task_set_assignment(task_set_of_entry, num_envs, int(kwargs.get('episodes_per_env', 8)), len(configs))
    return cls(task=lowering.ConcatenatedTasks([c['task'] for c in configs]), action_space=first['action_space'],
               renderers=first['renderers'], init_sprites=first['init_sprites'], keep_in_frame=first.get('keep_in_frame', True),
               max_episode_length=max(c.get('max_episode_length', 1000) for c in configs), metadata=first.get('metadata'),
               num_envs=num_envs, device_reset=device_reset, _task_sets=(configs, which), **kwargs)

  def __init__(self, task, action_space, renderers, init_sprites, keep_in_frame=True,
               max_episode_length=1000, metadata=None, num_envs=1, episodes_per_env=8,
               max_sprites=None, device=0, check_errors=32, action_dtype=np.float64,
               global_env_offset=0, device_reset='auto', refresh_every='auto', seed=None, _task_sets=None):
    # _task_sets (from_configs only): (the config dicts, u8[N, episodes_per_env] the set of every pool
    # entry); `task` is then lowering.ConcatenatedTasks of the configs' tasks -- what labels are lowered against
    self._configs, self._set_of_entry = _task_sets if _task_sets is not None else (None, None)
    self._task = task
    self._action_space = action_space
    self._renderers = renderers
    self._init_sprites = init_sprites
    self._keep_in_frame = keep_in_frame
    self._max_episode_length = max_episode_length
    self._metadata = metadata
    self._num_envs = int(num_envs)
    self._episodes_per_env = int(episodes_per_env)
    # index of this shard's first environment in the whole job (distributed.shard_range): device-side
    # reset sampling draws entry streams by global index, so shards never repeat each other's episodes
    self._global_env_offset = int(global_env_offset)
    # Per-environment error flags (conditions that make the reference raise) are read back every
    # `check_errors` steps (True/1: every step, which costs a device sync per step; 0/False: never;
    # `check()` can be called at any time).
    self._check_errors = int(check_errors)
    self._steps_since_check = 0
    # With device-side reset sampling: redraw the idle pool entries every `refresh_every` steps (0: never;
    # refresh_pool() can be called by hand).  episodes_per_env * shortest episode length is a safe period.
    # 'auto': 2 * (episodes_per_env - 1) steps -- an episode lasts at least two steps (FIRST + one more), so no
    # environment can run out of unseen entries between two refreshes.
    self._refresh_every = 2 * (self._episodes_per_env - 1) if refresh_every == 'auto' else int(refresh_every)
    self._steps_since_refresh = 0
    self._image_key, self._pil = lowering.find_pil_renderer(renderers)
    self._success_keys = [k for k, r in renderers.items() if type(r).__name__ == 'Success']
    self._factor_keys = {k: r for k, r in renderers.items() if type(r).__name__ == 'SpriteFactors'}
    unsupported = [k for k, r in renderers.items()
                   if k != self._image_key and k not in self._success_keys and k not in self._factor_keys]
    if unsupported:
      raise lowering.LoweringError('renderers not supported on device: %s' % unsupported)
    # Episodes are drawn on the device when init_sprites is a DeviceSampler, or -- device_reset=True /
    # 'auto' -- when it was built with sprite_generators.* from Product/SetMinus/Continuous/Discrete
    # distributions (the generator's closures are read, device_sampler.from_generator); 'auto' falls
    # back to calling init_sprites() on the host when that is not possible.
    # device_reset='tree': generators the DeviceSampler takes draw the episodes they draw today; every other tree of factor
    # distributions, and tasks that select by a sampled value or key on position, go through device_sampler.TreeSampler
    # (swb_sample_pool_tree); LoweringError if neither lowers.
    self._sampler = init_sprites if isinstance(init_sprites, (device_sampler.DeviceSampler, device_sampler.TreeSampler)) else None
    if self._sampler is None and device_reset:
      try:
        try:
          sampler = device_sampler.from_generator(init_sprites, seed=0)
          sampler.lower(task, renderers)
        except lowering.LoweringError:
          if device_reset != 'tree':
            raise
          sampler = device_sampler.from_generator(init_sprites, seed=0, tree=True)
          sampler.lower(task, renderers)
        # `seed` keys the Philox episode streams; None draws it from numpy's global stream, so np.random.seed()
        # makes runs reproducible and different seeds give different episodes.  Drawn only once the generator is
        # known to lower: a generator that falls back to the host path sees numpy's stream untouched.
        sampler.seed = int(np.random.randint(0, 2**31 - 1)) if seed is None else int(seed)
        self._sampler = sampler
      except lowering.LoweringError:
        if device_reset != 'auto':
          raise
    if self._sampler is not None and self._episodes_per_env < 2 and refresh_every == 'auto':
      import warnings
      warnings.warn('device-side reset sampling with episodes_per_env=1 cannot refresh the pool while it is in use: every '
                    'environment replays its one episode (raise episodes_per_env, or call refill_pool() yourself)')
    if self._sampler is not None:   # episodes are drawn by the engine (swb_sample_pool)
      episodes = None
      S = max_sprites or max(self._sampler.max_sprites, 1)
      pos_dt = np.float32
    else:
      episodes = self._draw_episodes()
      S = max_sprites or max([len(ep) for ep in episodes] + [1])
      pos_dt = lowering.position_dtype(episodes)
    self._max_sprites = S
    # SelectMove noise (action_spaces.py:69-75) is added to the action tensor on the device.  `action +
    # np.random.normal(...)` is float64 whatever the action's dtype (array + float64 array), so a noisy action
    # space always runs the engine's float64-action arithmetic.
    ns = getattr(action_space, '_noise_scale', None)
    if ns:
      action_dtype = np.float64
    if self._configs is None:
      self._cfg, sets = lowering.lower_config(task, action_space, renderers, keep_in_frame, max_episode_length, self._num_envs, S,
                                              pos_is_f32=(pos_dt == np.float32), action_dtype=action_dtype), None
    else:                             # task sets: one sub-task table, one set per config
      self._cfg, sets = lowering.merge_task_set_configs([
          lowering.lower_config(c['task'], action_space, renderers, keep_in_frame, c.get('max_episode_length', 1000),
                                self._num_envs, S, pos_is_f32=(pos_dt == np.float32), action_dtype=action_dtype)
          for c in self._configs])
    self._noise_scale = None if not ns else torch.as_tensor(np.asarray(ns, dtype=np.float64))
    self._noise_gen = None
    self._action_seed, self._action_draws = None, 0      # device action sampling (seed_actions / _next_action_seed)
    if self._sampler is not None:
      self._sampler_spec = self._sampler.lower(task, renderers)
      self._engine = self._new_engine(sets, device)
      self.refill_pool()
    elif sets is None:
      self._engine = _engine.Engine(self._cfg, self._lower_pool(episodes), device=device)
    else:                             # (the sets go in before the pool, the pool's entry sets right behind it)
      self._engine = self._new_engine(sets, device)
      self._engine.set_pool(self._lower_pool(episodes))
    self._render = self._pil is not None
    self._attr_assigned = {}      # (env, sprite, 'angle' | 'scale') -> (episode, the assigned value was an np.float32)

  # ------------------------------------------------------------------ pool
  def _draw_episodes(self):
    if self._configs is not None:     # entry (n, k) from the init_sprites of its own set
      return [list(self._configs[g]['init_sprites']()) for g in self._set_of_entry.reshape(-1)]
    return [list(self._init_sprites()) for _ in range(self._num_envs * self._episodes_per_env)]

  def _new_engine(self, sets, device):
    """An engine without a pool yet, with its task sets installed (an engine stand-in need not know the keyword)."""
    eng = _engine.Engine(self._cfg, None, device=device)
    if sets is not None:
      eng.set_task_sets(sets)
    return eng

  def _lower_pool(self, episodes):
    """The host pool of `episodes`; with task sets every entry is labelled for the sub-tasks of every set and names its own."""
    pool = lowering.lower_episodes(episodes, self._task, self._renderers, max_sprites=self._max_sprites)
    pool.assign_round_robin(self._num_envs, self._episodes_per_env)
    if self._configs is not None:
      pool.task_set = np.ascontiguousarray(self._set_of_entry.reshape(-1), dtype=np.uint8)
    return pool

  # ------------------------------------------------------------------ task sets
  @property
  def num_task_sets(self):
    """The number of task sets (configs of `from_configs`); 0: one task for the whole batch."""
    return self._engine.num_task_sets

  def task_sets(self):
    """i32[N] device tensor: the task set (the index of the config) of the episode every environment is in -- what an agent
    trained on the mix conditions on.  One small kernel, no host synchronisation."""
    return self._engine.task_sets()

  def set_task_set_of_entry(self, task_set_of_entry):
    """Changes which task set the pool entries are played under ('cycle', 'per_env' or an int array [N, episodes_per_env]).
    Takes effect at once, for running episodes too: every entry carries the labels of every set's sub-tasks.  Entries are
    not redrawn: with configs that draw from different `init_sprites` an entry keeps the sprites of the config it was drawn
    for (`refill_pool()` draws a fresh pool under the new assignment)."""
    if self._configs is None:
      raise lowering.LoweringError('set_task_set_of_entry: the environment has no task sets (BatchedEnvironment.from_configs)')
    which = lowering.task_set_assignment(task_set_of_entry, self._num_envs, self._episodes_per_env, len(self._configs))
    self._engine.set_entry_task_sets(which.reshape(-1))
    self._set_of_entry = which

  def refill_pool(self):
    """Draws a fresh pool with init_sprites(); every environment restarts (next step is FIRST).

    With a DeviceSampler the pool is drawn by a HIP kernel (no host sampling, no upload)."""
    if self._sampler is not None:
      k = self._episodes_per_env
      base = np.arange(self._num_envs, dtype=np.int32) * k
      sample = self._engine.sample_pool_tree if self._tree_sampled else self._engine.sample_pool
      sample(self._sampler_spec, self._num_envs * k, base, np.full(self._num_envs, k, np.int32), self._sampler.next_seed(),
             first_entry=self._global_env_offset * k)
      if self._configs is not None:   # (a pool call puts every entry in set 0; refresh_pool -- swb_resample_pool -- keeps the sets)
        self._engine.set_entry_task_sets(self._set_of_entry.reshape(-1))
      return
    self._engine.set_pool(self._lower_pool(self._draw_episodes()))

  @property
  def _tree_sampled(self):
    return isinstance(self._sampler, device_sampler.TreeSampler)

  def refresh_pool(self):
    """DeviceSampler / TreeSampler only: redraws every pool entry that no environment is playing right now, without
    resetting anything.  Called every few episodes, environments never meet an episode twice."""
    if self._sampler is None:
      raise lowering.LoweringError('refresh_pool() needs init_sprites to be a device_sampler.DeviceSampler')
    self._engine.resample_pool(self._sampler.next_seed(),
                               first_entry=self._global_env_offset * self._episodes_per_env)

  # ------------------------------------------------------------------ dm_env surface
  @property
  def num_envs(self):
    return self._num_envs

  @property
  def action_space(self):
    return self._action_space

  @property
  def engine(self):
    return self._engine

  def action_spec(self):
    return self._action_space.action_spec()

  def observation_spec(self):
    spec = {}
    if self._image_key is not None:
      spec[self._image_key] = self._pil.observation_spec()
    for k in self._success_keys:
      spec[k] = dm_env.specs.Array(shape=(), dtype=np.bool_)
    for k, r in self._factor_keys.items():
      spec[k] = dm_env.specs.Array(shape=(self._max_sprites, len(r._factors)), dtype=np.float64)
    return spec

  def _timestep(self):
    e = self._engine
    if self._check_errors:
      self._steps_since_check += 1
      if self._steps_since_check >= self._check_errors:
        self.check()
    obs = {}
    if self._image_key is not None:
      obs[self._image_key] = e.obs
    for k in self._success_keys:
      obs[k] = e.success.bool()
    self._add_factor_obs(obs)
    return BatchedTimeStep(e.step_type, e.reward, e.discount, obs)

  def _add_factor_obs(self, obs):
    if not self._factor_keys:
      return
    from spriteworld_amd import sprite as sprite_lib
    full = self._engine.factors()
    for k, r in self._factor_keys.items():
      cols = [sprite_lib.FACTOR_NAMES.index(f) for f in r._factors]
      obs[k] = full if cols == list(range(10)) else full[:, :, cols]

  def seed_noise(self, seed):
    """Seeds the generator of the SelectMove action noise."""
    self._noise_gen = torch.Generator(device=self._engine.device)
    self._noise_gen.manual_seed(int(seed))

  def check(self):
    """Raises what the reference would have raised if any environment flagged an error."""
    self._steps_since_check = 0
    if self._tree_sampled:
      spent = self._engine.sampler_exhausted()
      if spent:      # (the reference: ValueError after _MAX_TRIES rejections, factor_distributions.py)
        raise EnvironmentError_('%d sprites of the last pool kept a draw their distribution rejects: max_tries = %d rejections '
                                'were used up (TreeSampler(max_tries=...))' % (spent, self._sampler.max_tries))
    rejected = self._engine.load_rejected() if getattr(self, '_state_loaded', False) else 0      # (one word, after a load_state only)
    if rejected:
      raise IndexError('load_state: %d slot values were outside [-1, len(snapshot)); those environments were left as they were' % rejected)
    err = int(self._engine.error.max().item())
    if err:
      self._engine.error.zero_()          # the flags are sticky on the device (include/swb.h): consumed here
      if err & _abi.ENV_ERR_DB_ZERO:
        raise ZeroDivisionError('float division by zero (Davies-Bouldin score is 0)')
      if err & _abi.ENV_ERR_DB_LABELS:
        raise ValueError('Number of labels is invalid for davies_bouldin_score')
      raise EnvironmentError_('internal engine error bits 0x%x' % err)

  def reset(self, envs=None):
    """Environment.reset() for every environment: returns the FIRST time steps.
    With `envs` (a bool or uint8 mask of shape [N]; anything else raises ValueError) only those environments are reset
    (swb_reset_envs), by one null-action step in which only they are active: they return FIRST, from their next pool entry, and
    the others are untouched -- their entries of the returned time step are those of their last active step, as in
    `step(active=...)`."""
    if envs is None:
      self._engine.reset_all()
      return self.step(self.null_actions())
    mask = self._engine._mask_tensor(envs, 'reset envs')  # pylint: disable=protected-access
    self._engine.reset_envs(mask)
    return self.step(self.null_actions(), active=mask)

  def null_actions(self):
    if self._cfg.action_space == _abi.ACTION_EMBODIED:
      return torch.zeros((self._num_envs, 2), dtype=torch.int32, device=self._engine.device)
    dt = torch.float32 if self._cfg.action_is_f32 else torch.float64
    return torch.zeros((self._num_envs, 4), dtype=dt, device=self._engine.device)

  def step(self, actions, active=None):
    """actions: [N, 4] float (SelectMove / DragAndDrop) or [N, 2] int (Embodied).
    active: None (every environment), or a bool or uint8 mask of shape [N] (anything else raises ValueError).  An environment
    whose entry is 0 takes no part in the step: its state does not change, an auto-reset that is due stays due, and its action
    row is never read (it may hold NaN).  The returned time step HOLDS, for such an environment, the step type, reward, discount
    and success flag of its last active step -- a held reward must not be summed twice: weigh sums with the mask -- while the
    image shows its current state.  SelectMove noise is drawn for the whole batch whatever the mask, so an environment's noise
    does not depend on which others are active; the pool refresh and error check tick as for any step."""
    if active is not None:
      active = self._engine._mask_tensor(active, 'step active')  # pylint: disable=protected-access
    if self._noise_scale is not None:
      e = self._engine
      if not isinstance(actions, torch.Tensor):
        actions = torch.as_tensor(np.ascontiguousarray(actions))
      actions = actions.to(device=e.device)
      noise = torch.randn(actions.shape, dtype=torch.float64, device=e.device, generator=self._noise_gen)
      actions = actions.to(torch.float64) + noise * self._noise_scale.to(e.device)      # float64 from here on (see __init__)
    if active is None:      # (an engine stand-in with the older step(actions, render) surface still serves unmasked steps)
      self._engine.step(actions, render=self._render)
    else:
      self._engine.step(actions, render=self._render, active=active)
    if self._refresh_every and self._sampler is not None:
      self._steps_since_refresh += 1
      if self._steps_since_refresh >= self._refresh_every:
        self._steps_since_refresh = 0
        self.refresh_pool()
    return self._timestep()

  def run_episodes(self, policy, episodes_per_env=1, max_steps=None):
    """Exactly `episodes_per_env` (E) episodes of every environment, then stop: the evaluation loop.  Starts with `reset()`, then
    calls `policy(timestep, active) -> actions` before every step -- `timestep` the `BatchedTimeStep` of the step before
    (entries of frozen environments held, see `step`), `active` the bool[N] device mask of the step about to be taken; the
    action rows of inactive environments are never read -- and freezes an environment as soon as its E-th LAST step has been
    seen.  A frozen environment is not stepped again: it does not start episode E + 1, draws nothing from the pool and is
    rendered from the frame cache.  Returns `EpisodeStats` of device tensors [N], accumulated on the device: episode_return
    (float64, the rewards of the environment's active non-FIRST steps added in step order), length (those steps), episodes and
    success (of its last LAST step).  One `.any()` synchronisation per step decides when to stop; `max_steps` bounds the steps
    taken after the reset (None: no bound) -- environments that have not finished by then report episodes < E.
    Afterwards every finished environment has `state()['episode'] == E` and a reset pending: the next `step()` in which it is
    active, or `reset()`, starts its next episode."""
    E = int(episodes_per_env)
    if E < 1:
      raise ValueError('run_episodes: episodes_per_env must be positive, got %d' % E)
    N, dev = self._num_envs, self._engine.device
    ret = torch.zeros(N, dtype=torch.float64, device=dev)
    length = torch.zeros(N, dtype=torch.int64, device=dev)
    episodes = torch.zeros(N, dtype=torch.int32, device=dev)
    success = torch.zeros(N, dtype=torch.bool, device=dev)
    ts = self.reset()
    active = torch.ones(N, dtype=torch.bool, device=dev)
    steps = 0
    while max_steps is None or steps < int(max_steps):
      ts = self.step(policy(ts, active), active=active)
      steps += 1
      counted = active & (ts.step_type != _abi.STEP_FIRST)
      ret = ret + torch.where(counted, ts.reward, torch.zeros_like(ts.reward))
      length = length + counted.to(torch.int64)
      ended = active & (ts.step_type == _abi.STEP_LAST)
      episodes = episodes + ended.to(torch.int32)
      success = torch.where(ended, self._engine.success.bool(), success)
      active = active & (episodes < E)
      if not bool(active.any()):
        break
    return EpisodeStats(ret, length, episodes, success)

  def rollout(self, actions, keep_steps=False):
    """Scores candidate action sequences from where every environment is now, without stepping: actions is [N, M, K, A]
    (tensor or array; A = 4, or 2 for Embodied) -- M candidates of K steps per environment.  Returns a `Rollout` whose
    [n, m, k] entries are exactly what step k + 1 of environment n would return had the next K steps been actions[n, m, :]
    (auto-resets included: a candidate that ends plays FIRST on its next step; `Rollout.episode_return()` sums up to the
    first LAST).  One permute to the engine's [K, N, M, A] layout, two kernels (swb_rollout), no host synchronisation; the
    live environments, their error flags and the pool are untouched.
    A rollout is of the NOISELESS dynamics: a SelectMove `noise_scale` is not applied to the candidates (`step()` draws its
    noise per call; the candidates are scored as given).
    With `keep_steps` (swb_rollout_trajectory) the same `Rollout` is returned and the state after every step is kept:
    `rollout_frames(step=...)` draws it and `rollout_positions()` returns the sprite positions per step."""
    e = self._engine
    if not isinstance(actions, torch.Tensor):
      actions = torch.as_tensor(np.ascontiguousarray(actions))
    if actions.dim() != 4 or actions.shape[0] != self._num_envs:
      raise ValueError('rollout actions must be [N, M, K, A] with N = %d, got %s' % (self._num_envs, tuple(actions.shape)))
    self._rollout_steps = None
    res = e.rollout(actions.to(device=e.device).permute(2, 0, 1, 3), positions=True, keep_steps=keep_steps)
    if keep_steps:
      self._rollout_steps = RolloutSteps(res['x_steps'].permute(1, 2, 0, 3), res['y_steps'].permute(1, 2, 0, 3),
                                         res['n_sprites_steps'].permute(1, 2, 0))
    per_step = [res[k].permute(1, 2, 0) for k in ('step_type', 'reward', 'discount', 'success')]
    return Rollout(*(per_step + [res['x'], res['y'], res['n_sprites'], res['error']]))

  def rollout_random(self, num_candidates, num_steps, click='uniform', keep_steps=False):
    """A random-shooting planner's rollout: `num_candidates` (M) sequences of `num_steps` (K) random actions per environment,
    drawn by the rollout kernel itself, step by step, from the state each candidate has reached (swb_rollout_sampled: two
    kernels, no host synchronisation, no action tensor generated, permuted and loaded back).  Returns `(Rollout, actions)`:
    the `Rollout` of `rollout(actions)` -- bit for bit what that call returns for these actions -- and actions [N, M, K, A], a
    view of the engine's tensor in the layout `rollout()` accepts (A = 4 float64, float32 with action_dtype=np.float32, or 2
    int32 for Embodied): `actions[torch.arange(N), best, 0]` is the first step of the chosen plans, ready for `step()`.
    click='uniform': every action is `action_space.sample()`.  click='sprite': the click of every SelectMove / DragAndDrop
    action lands inside a sprite drawn by index among those of its candidate, where they are at that step -- inside a
    rollout the sprites move per candidate, so no `sample_actions` call can place such clicks; Embodied actions stay uniform.
    Containment is guaranteed for float64 actions only: rounded to float32 a click may leave its sprite at the edge.
    The rollout is of the NOISELESS dynamics, as `rollout`'s: a SelectMove `noise_scale` is not applied to the drawn actions.
    The draws are Philox streams keyed by `seed_actions()` (one key per call, as `sample_actions(where='device')`), one stream
    per (global environment, candidate): `seed_actions(s)` or `np.random.seed` reproduces a call, and a candidate's stream
    depends neither on M nor on K.  `rollout_frames()` works afterwards and, with `keep_steps`, `rollout_frames(step=...)`
    and `rollout_positions()`, as after `rollout`."""
    if click not in ('uniform', 'sprite'):
      raise ValueError("rollout_random: click is 'uniform' or 'sprite', got %r" % (click,))
    mode = _abi.SAMPLE_ON_SPRITE if click == 'sprite' else _abi.SAMPLE_UNIFORM
    self._rollout_steps = None
    res = self._engine.rollout_sampled(mode, self._next_action_seed(), int(num_candidates), int(num_steps),
                                       first_env=self._global_env_offset, positions=True, keep_steps=keep_steps)
    if keep_steps:
      self._rollout_steps = RolloutSteps(res['x_steps'].permute(1, 2, 0, 3), res['y_steps'].permute(1, 2, 0, 3),
                                         res['n_sprites_steps'].permute(1, 2, 0))
    per_step = [res[k].permute(1, 2, 0) for k in ('step_type', 'reward', 'discount', 'success')]
    return Rollout(*(per_step + [res['x'], res['y'], res['n_sprites'], res['error']])), res['actions'].permute(1, 2, 0, 3)

  def rollout_guided(self, num_candidates, num_steps, sprite_weights=None, motion_mean=0.5, motion_std=0.25, keep_steps=False):
    """An iterative planner's rollout: as `rollout_random(click='sprite')`, but step k of every candidate of environment n is
    drawn from a plan distribution of (n, k) the caller owns and refits between calls (swb_rollout_guided):
      sprite_weights [N, K, W] (tensor or array, W <= max_sprites; None: uniform): the sprite to click is drawn with
        probability proportional to its weight among those the candidate has at that step -- negative weights count as 0,
        sprites at index >= W have weight 0, a row that sums to 0 (or is not finite) means uniform --, the click is a uniform
        point inside that sprite WHERE THE CANDIDATE HAS IT at that step;
      motion_mean, motion_std [N, K, 2] or scalars: action[2:4] = clip(mean + std * z, 0, 1).  z is NOT Gaussian: it is a sum
        of four uniforms, centred and scaled (Irwin-Hall, n = 4): mean 0, variance 1, bell-shaped, support +-3.46 -- every
        operation of it is an IEEE add or multiply, so the draws are reproducible bit for bit.
    Embodied: sprite_weights are ACTION weights [N, K, 8] over index = carry * 4 + direction; motion_mean / motion_std are not
    used.  Returns `(Rollout, actions, sprite)`: the first two as `rollout_random`'s -- `rollout(actions)` returns the same
    `Rollout` bit for bit --, sprite i32[N, M, K] the index drawn (-1: the candidate had no sprite; Embodied: the action index).
    Keys, streams, `global_env_offset`, `keep_steps` and what works afterwards (`rollout_frames`, `rollout_positions`,
    `rollout_snapshot`) are `rollout_random`'s.  Torch operations and two kernels, no host synchronisation."""
    e = self._engine
    N, K = self._num_envs, int(num_steps)
    embodied = e.cfg.action_space == _abi.ACTION_EMBODIED

    def per_step(t, last, what):      # [N, K, last] (or a scalar) -> f64[K, N, last] on the device
      if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(np.asarray(t, dtype=np.float64))
      t = t.to(device=e.device, dtype=torch.float64)
      if t.dim() == 0:
        return t.expand(K, N, last).contiguous()
      if t.dim() != 3 or tuple(t.shape[:2]) != (N, K) or (last is not None and t.shape[2] != last):
        raise ValueError('rollout_guided: %s must be [N, K, %s] with N = %d, K = %d, got %s' % (what, last or 'W', N, K, tuple(t.shape)))
      return t.permute(1, 0, 2).contiguous()

    cdf = width = None
    if sprite_weights is not None:
      w = sprite_weights if isinstance(sprite_weights, torch.Tensor) else torch.as_tensor(np.asarray(sprite_weights))
      if w.dim() != 3:
        raise ValueError('rollout_guided: sprite_weights must be [N, K, W], got %s' % (tuple(w.shape),))
      cdf = per_step(w.to(device=e.device).clamp_min(0).double().cumsum(-1), None, 'sprite_weights')
      width = int(cdf.shape[2])
    mean = std = None
    if not embodied:
      mean, std = per_step(motion_mean, 2, 'motion_mean'), per_step(motion_std, 2, 'motion_std')
    self._rollout_steps = None
    res = e.rollout_guided(self._next_action_seed(), int(num_candidates), K, choice_cdf=cdf, width=width, motion_mean=mean,
                           motion_std=std, first_env=self._global_env_offset, positions=True, keep_steps=keep_steps)
    if keep_steps:
      self._rollout_steps = RolloutSteps(res['x_steps'].permute(1, 2, 0, 3), res['y_steps'].permute(1, 2, 0, 3),
                                         res['n_sprites_steps'].permute(1, 2, 0))
    fields = [res[k].permute(1, 2, 0) for k in ('step_type', 'reward', 'discount', 'success')]
    return (Rollout(*(fields + [res['x'], res['y'], res['n_sprites'], res['error']])), res['actions'].permute(1, 2, 0, 3),
            res['sprite'].permute(1, 2, 0))

  def plan_cem(self, num_candidates, num_steps, iterations=3, num_elites=None, weight_floor=0.1, min_std=0.02, init=None):
    """A cross-entropy-method planner on the device: `iterations` (I) rounds of `rollout_guided` with M = `num_candidates`
    sequences of K = `num_steps` steps per environment, the plan distribution refitted to each round's elites.  Returns
    `CemPlan(actions [N, K, A], episode_return f64[N], best_per_iteration f64[N, I], sprite_weights [N, K, W], motion_mean,
    motion_std [N, K, 2])`: the best sequence found per environment, its `Rollout.episode_return()`, the best return known
    after each round, and the distribution the last refit left.
    Round 0 draws from `init` -- a `CemPlan` or a `(sprite_weights, motion_mean, motion_std)` triple; None: uniform weights,
    mean 0.5, std 0.25.  To warm-start MPC pass the returned fields shifted by one step.  Every round
      * takes the `num_elites` (E; default max(1, M // 8)) candidates of highest `episode_return()` per environment (topk);
      * refits the weights: how many elites picked sprite j at step k (scatter_add over [N, K, W]; a candidate without sprites
        picks none), plus `weight_floor`, so that no sprite's probability falls below floor / (E + W * floor) and an
        environment whose elites agree still looks elsewhere (default 0.1: an eleventh of one elite's vote);
      * refits the motion: the elites' population mean and standard deviation of actions[2:4] per (n, k), the deviation at least
        `min_std` (default 0.02 of the motion range: below it the next round's candidates would all but repeat the elites).
        Embodied: the weights are ACTION weights (W = 8) and the motion parameters stay as given.
    An incumbent -- the best sequence so far and its return -- is replaced only where a round's best is STRICTLY greater, so
    best_per_iteration never decreases; `actions` and `episode_return` are the incumbent's, and `rollout(actions[:, None])`
    returns that return bit for bit (the rollouts are noiseless).
    Afterwards the engine holds the LAST round's rollout, not the incumbent's: `rollout_frames`, `rollout_positions` and
    `rollout_snapshot` speak of that round's candidates.  To adopt the plan, step with `actions[:, k]`, or call
    `rollout(actions[:, None])` first and take `rollout_snapshot()`.
    Everything is torch on the device and two kernels per round: no host synchronisation."""
    e = self._engine
    N, M, K, I = self._num_envs, int(num_candidates), int(num_steps), int(iterations)
    if I <= 0:
      raise ValueError('plan_cem: iterations must be positive, got %d' % I)
    E = max(1, M // 8) if num_elites is None else int(num_elites)
    if not 1 <= E <= M:
      raise ValueError('plan_cem: num_elites must be in [1, %d], got %d' % (M, E))
    embodied = e.cfg.action_space == _abi.ACTION_EMBODIED
    W = 8 if embodied else e.S
    f64 = dict(dtype=torch.float64, device=e.device)
    if init is None:
      weights, mean, std = torch.ones((N, K, W), **f64), torch.full((N, K, 2), 0.5, **f64), torch.full((N, K, 2), 0.25, **f64)
    else:
      weights, mean, std = (init.sprite_weights, init.motion_mean, init.motion_std) if isinstance(init, CemPlan) else init
      weights, mean, std = [torch.as_tensor(t).to(**f64) for t in (weights, mean, std)]
      if tuple(weights.shape) != (N, K, W) or tuple(mean.shape) != (N, K, 2) or tuple(std.shape) != (N, K, 2):
        raise ValueError('plan_cem: init must be sprite_weights [%d, %d, %d] and motion_mean, motion_std [%d, %d, 2], got %s, %s, %s' % (
            N, K, W, N, K, tuple(weights.shape), tuple(mean.shape), tuple(std.shape)))
    rows = torch.arange(N, device=e.device)
    best_actions = best_return = None
    history = []
    for it in range(I):
      r, actions, sprite = self.rollout_guided(M, K, weights, mean, std)
      top, elite = r.episode_return().topk(E, dim=1)                  # [N, E], best first
      round_actions, round_return = actions[rows, elite[:, 0]], top[:, 0]
      if it == 0:
        best_actions, best_return = round_actions.clone(), round_return
      else:
        better = round_return > best_return
        best_actions = torch.where(better[:, None, None], round_actions, best_actions)
        best_return = torch.where(better, round_return, best_return)
      history.append(best_return)
      weights, fit_mean, fit_std = cem_refit(actions, sprite, elite, W, weight_floor, min_std)
      if not embodied:
        mean, std = fit_mean, fit_std
    return CemPlan(best_actions, best_return, torch.stack(history, dim=1), weights, mean, std)

  def rollout_positions(self):
    """`RolloutSteps(x, y, n_sprites)` of the last `rollout(..., keep_steps=True)`: x, y f64[N, M, K, S] and n_sprites
    i32[N, M, K] views of device tensors, entry [n, m, k] the sprites of environment n after step k + 1 of candidate m
    ([..., K - 1, :] is the `Rollout`'s x, y).  Raises when the last rollout kept no steps."""
    if getattr(self, '_rollout_steps', None) is None:
      raise EnvironmentError_('rollout_positions: the last rollout kept no steps (call rollout(actions, keep_steps=True) first)')
    return self._rollout_steps

  def rollout_frames(self, candidates=None, step=None):
    """The frames the candidates of the last `rollout` end in, a fresh device tensor u8[N, M, H, W, 3]: entry [n, m] is to the
    byte the image observation step K of environment n would have returned had the K steps been actions[n, m, :] (a candidate
    that ended on step K shows its terminal sprites, one that restarted on it the new episode).  With `candidates` (int[N],
    e.g. `rollout.episode_return().argmax(1)`; values outside [0, M) are clamped) only the frame of candidate candidates[n] of
    environment n, u8[N, H, W, 3], for the cost of one step's rendering.  Call it after `rollout(...)`, on the same stream
    (swb_rollout_frames: the engine's render path on the rollout's scratch state, no host synchronisation; the live
    environments, their last observation and the pool are untouched).
    `step`, after `rollout(..., keep_steps=True)` (swb_rollout_step_frames): an int k in [0, K) gives the same two forms for
    the states after step k + 1; 'all' gives the K frames of the picked candidates, a u8[N, K, H, W, 3] view, and raises
    ValueError without `candidates`."""
    obs = self._engine.rollout_frames(candidates, step=step)['obs']
    return obs.permute(1, 0, 2, 3, 4) if isinstance(step, str) else obs

  # ------------------------------------------------------------------ snapshots
  # A snapshot is the DEVICE state of environments: positions, sprite counts, pool entries, step counts, episode numbers, reset
  # flags and the pool range each resets through.  NOT part of it, and unchanged by load_state: the generator of the SelectMove
  # noise (seed_noise), the seed and draw count of the device action stream (seed_actions), the reset sampler's seed sequence,
  # and the record of attribute types assigned through sprite setters (_attr_assigned; engines with setter overrides refuse
  # snapshots altogether).
  def save_state(self, envs=None):
    """An `engine.Snapshot` of the environments `envs` (int[C]; None: all, in order): device tensors, one kernel, no host
    synchronisation.  `snapshot.cpu()` and `engine.get_pool()` together are a checkpoint."""
    return self._engine.save_state(envs)

  def load_state(self, snapshot, slots=None):
    """Puts environment n into the state of slot slots[n] of `snapshot` (int[N]; -1: the environment stays as it is; None:
    slot n): one kernel, no host synchronisation.  From the next `step()` on a loaded environment returns, bit for bit, what
    its source would have -- auto-resets through the source's pool entries included.  Raises when the pool has been redrawn
    since the snapshot was taken (refresh_pool / refill_pool: its entries may be gone).  Slot values outside
    [-1, len(snapshot)) leave their environment alone and make the next `check()` raise IndexError.  With device-side reset
    sampling the automatic pool refresh is switched off by a load: the pool ranges may have moved between environments, which
    `refresh_pool()` cannot follow (`refill_pool()` starts afresh)."""
    self._engine.load_state(snapshot, slots)
    self._state_loaded = True
    self._refresh_every = 0

  def rollout_snapshot(self, candidates=None):
    """The states the candidates of the last rollout ended in, as an `engine.Snapshot`: all N * M (slot n * M + m: candidate m
    of environment n), or, with `candidates` (int[N]; values outside [0, M) are clamped, as in `rollout_frames`), slot n the
    end state of candidate candidates[n] of environment n -- `env.load_state(env.rollout_snapshot(best))` advances every
    environment by its chosen plan in one launch, without replaying the K steps."""
    e = self._engine
    if candidates is None:
      return e.save_state(None, source='rollout')
    cand = candidates if isinstance(candidates, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(candidates))
    if cand.dim() != 1 or cand.shape[0] != self._num_envs or cand.is_floating_point():
      raise ValueError('rollout_snapshot candidates must be int[%d], got %s %s' % (self._num_envs, cand.dtype, tuple(cand.shape)))
    M = max(e._rollout_M, 1)  # pylint: disable=protected-access
    cand = cand.to(device=e.device, dtype=torch.int64).clamp(0, M - 1)
    index = torch.arange(self._num_envs, device=e.device, dtype=torch.int64) * M + cand
    return e.save_state(index, source='rollout')

  def _pool_ranges(self):
    """(pool_base, pool_len) int32[N] as the pool was laid out when it was installed."""
    if getattr(self, '_ranges', None) is not None:
      return self._ranges
    if self._engine.pool is not None:
      return np.asarray(self._engine.pool.pool_base, np.int32), np.asarray(self._engine.pool.pool_len, np.int32)
    k = self._episodes_per_env
    return np.arange(self._num_envs, dtype=np.int32) * k, np.full(self._num_envs, k, np.int32)

  def fork(self, num_copies):
    """A new BatchedEnvironment of N * num_copies environments, environment n * num_copies + m in the state of environment n of
    this one: the same task, action space, renderers and limits, the device pool copied device to device (swb_copy_pool), the
    states put in by one save and one load.  No episode is drawn and nothing is uploaded on the way; this environment is left
    as it is.  Every copy steps, renders and auto-resets as its source would from here on (copies that take the same actions
    stay equal).  The copy has no sampler: its automatic pool refresh is off and `refresh_pool()` raises; `refill_pool()`
    draws a fresh pool on the host.  Its noise generator, action stream and setter records start unset (they are not state)."""
    M = int(num_copies)
    if M < 1:
      raise ValueError('fork: num_copies must be positive, got %d' % M)
    child = object.__new__(BatchedEnvironment)
    child.__dict__.update(self.__dict__)
    N = self._num_envs
    child._num_envs = N * M
    child._cfg = type(self._cfg).from_buffer_copy(self._cfg)
    child._cfg.n_envs = N * M
    child._sampler = None
    child._refresh_every = 0
    child._steps_since_refresh = child._steps_since_check = 0
    child._noise_gen = None
    child._action_seed, child._action_draws = None, 0
    child._attr_assigned = {}
    child._rollout_steps = None
    child._state_loaded = True
    base, length = self._pool_ranges()
    child._ranges = (np.repeat(base, M), np.repeat(length, M))
    child._engine = _engine.Engine(child._cfg, None, device=self._engine.device.index or 0)
    if self._engine.task_set_table is not None:          # (the sets first: swb_copy_pool refuses handles whose tables differ)
      child._engine.set_task_sets(self._engine.task_set_table)
    child._engine.copy_pool_from(self._engine, *child._ranges)
    child._engine.load_state(self._engine.save_state(), torch.arange(N * M, device=self._engine.device) // M)
    return child

  def observation(self):
    """environment.py:136-142: every renderer's view of the sprites AS THEY ARE NOW -- the frame is rendered now (swb_render)
    and a Success renderer evaluates the task now (swb_evaluate; environment.py:128-131 `state()` calls `success()` on the
    current sprites), so that a setter or `set_positions` since the last step shows in both (round-5 advice: the Success key
    used to carry the last step's flag)."""
    obs = {}
    if self._image_key is not None:
      obs[self._image_key] = self._engine.render()
    if self._success_keys:
      success = self._engine.evaluate().bool()
      for k in self._success_keys:
        obs[k] = success
    self._add_factor_obs(obs)
    return obs

  def state(self):
    """Live structure-of-arrays state (host copies): x, y [N, S], n_sprites, step_count, ..."""
    return self._engine.state()

  def sample_actions(self, where='host', click='uniform'):
    """One random-agent action per environment.  With no arguments (where='host'): `action_space.sample(num_envs)` --
    numpy's global stream on the host, float64, uploaded by the next step().
    where='device': drawn by a HIP kernel (swb_sample_actions) into a device tensor that step() takes as it is; no host
    synchronisation.  click='sprite' (device only; the batched `Environment.sample_contained_position()`): the click of a
    SelectMove / DragAndDrop action lands inside a randomly chosen sprite of its environment, as it is now; Embodied
    actions stay uniform.  Containment holds for float64 actions; rounded to float32 (action_dtype=np.float32) a click may
    leave its sprite at the edge.  The device stream is Philox keyed by seed_actions(), not numpy's MT19937."""
    mode = self._sampling_mode(where, click)
    if mode is None:
      return self._action_space.sample(self._num_envs)
    return self._engine.sample_actions(mode, self._next_action_seed(), first_env=self._global_env_offset)['actions']

  def sample_contained_positions(self):
    """environment.py:110-126 for every environment, on the device: a sprite drawn uniformly by index, then a position of
    its bounding box redrawn until the sprite contains it.  Returns ContainedPositions(position f64[N, 2], sprite i32[N],
    tries i32[N]) of device tensors: sprite -1 / tries 0 for an environment without sprites (its position is uniform in the
    frame); tries -1 and the sprite's own position where _abi.SWB_CONTAINED_MAX_TRIES draws all missed (a degenerate sprite)."""
    res = self._engine.sample_actions(_abi.SAMPLE_ON_SPRITE, self._next_action_seed(), first_env=self._global_env_offset,
                                      outputs=('position', 'sprite', 'tries'))
    return ContainedPositions(res['position'], res['sprite'], res['tries'])

  def seed_actions(self, seed):
    """Seeds the device action stream: call k after it draws with splitmix64(seed ^ a constant, k) as its Philox key (the
    constant keeps it apart from the reset sampler's keys under the same seed).  Unseeded, the base
    seed is drawn once from numpy's global stream at the first device call, so np.random.seed() reproduces a run."""
    self._action_seed = int(seed)
    self._action_draws = 0

  def _sampling_mode(self, where, click):
    if where not in ('host', 'device') or click not in ('uniform', 'sprite'):
      raise ValueError("sample_actions: where is 'host' or 'device' and click 'uniform' or 'sprite', got %r, %r" % (where, click))
    if where == 'host':
      if click != 'uniform':
        raise ValueError("sample_actions: click='sprite' is drawn on the device (where='device')")
      return None
    return _abi.SAMPLE_ON_SPRITE if click == 'sprite' else _abi.SAMPLE_UNIFORM

  def _next_action_seed(self):
    """A fresh 64-bit Philox key per call (splitmix64 of seed and call counter, as DeviceSampler.next_seed)."""
    if self._action_seed is None:
      self.seed_actions(int(np.random.randint(0, 2**31 - 1)))
    # (the constant keeps these keys apart from DeviceSampler.next_seed's under the same seed: the kernels share the counter
    # layout, and action call k of environment e must not replay the stream that drew pool entry e in reset draw k)
    z = ((self._action_seed ^ _ACTION_KEY_DOMAIN) * 0x9E3779B97F4A7C15 + self._action_draws + 1) & 0xFFFFFFFFFFFFFFFF
    self._action_draws += 1
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return z ^ (z >> 31)

  # ------------------------------------------------------------------ live sprites (sprite.py:152-175)
  def sprites(self, env=0):
    """The sprites of environment `env` in its current episode, back to front, as `sprite.LiveSprite` handles
    (the reference's `env.state()['sprites']`): `env.sprites(3)[0].angle = 45` acts on the device state."""
    from spriteworld_amd import sprite as sprite_lib
    n = self._engine.env_state(env)['n_sprites']
    return [sprite_lib.LiveSprite(self, env, k) for k in range(n)]

  def set_sprite_attr(self, env, sprite, name, value):
    """`sprites(env)[sprite].<name> = value` for name in ('shape', 'angle', 'scale'): the reference's setters
    (sprite.py:152-175) through swb_set_sprite_attr.  The sprite's task labels are re-evaluated with the new
    factor (tasks.py:134-137,196-205), so a filter keyed on shape / angle / scale follows the change."""
    from spriteworld_amd import shapes as shapes_lib
    from spriteworld_amd import sprite as sprite_lib
    attr = {'shape': _abi.ATTR_SHAPE, 'angle': _abi.ATTR_ANGLE, 'scale': _abi.ATTR_SCALE}[name]
    live = sprite_lib.LiveSprite(self, env, sprite)
    factors = live.factors
    before = factors[name]               # (one read of the sprite serves the labels and the setter's difference)
    factors[name] = value
    proxy = collections.namedtuple('_Factors', ['factors'])(factors)
    subs = lowering.subtasks_of(self._task)
    label = np.array([lowering._label_of(sub, proxy) for sub in subs], dtype=np.int8)  # pylint: disable=protected-access
    # tasks whose filters key on position: the sprite's label in every cell of the task's grid, with the new attribute
    cell_label = None
    f32 = bool(self._cfg.pos_is_f32)
    cuts = [lowering.position_cuts(sub, f32) for sub in subs]
    if any(xc or yc for xc, yc in cuts):
      cell_label = np.zeros((len(subs), _abi.SWB_MAX_CELLS), np.int8)
      for t, (sub, (xc, yc)) in enumerate(zip(subs, cuts)):
        if xc or yc:
          cell_label[t] = lowering.cell_labels_of(sub, proxy, xc, yc, np.float32 if f32 else np.float64)
    delta = None
    episode = self._engine.env_state(env)['episode']
    if name != 'shape':
      # sprite.py:163,173 take `a - self._angle` / `s - self._scale` with whatever types the two carry: an np.float32
      # attribute (factor distributions draw float32) makes it a float32 subtraction under NEP 50.  numpy decides here too.
      old = before
      old = np.float32(old) if self._attr_is_f32(env, sprite, name, episode, old) else float(old)
      delta = float(value - old)
    self._engine.set_sprite_attr(env, sprite, attr, shapes_lib.shape_index(value) if name == 'shape' else float(value),
                                 delta=delta, label=label, cell_label=cell_label)
    if name != 'shape':           # from now on the attribute is the object the caller assigned
      self._attr_assigned[(env, sprite, name)] = (episode, getattr(value, 'dtype', None) == np.float32)

  def _attr_is_f32(self, env, sprite, name, episode, value):
    """Is this sprite's angle / scale an np.float32 in the reference?  A value assigned through a setter keeps the type it
    was given; otherwise it is what the episode's generator drew -- factor distributions draw float32, Discrete candidates
    and Sprite() arguments are Python numbers -- which the pool records per sprite (swb_pool::attr_f32: written by
    `lowering.lower_episodes` from the sprite objects and by the device sampler from the factor's kind)."""
    del value
    rec = self._attr_assigned.get((env, sprite, name))
    if rec is not None and rec[0] == episode:
      return rec[1]
    angle_f32, scale_f32 = self._engine.sprite_types(env, sprite)
    return angle_f32 if name == 'angle' else scale_f32

  def close(self):
    self._engine.close()


class EnvironmentGroups(object):
  """`num_groups` independent BatchedEnvironments of `num_envs // num_groups` environments, each on its own
  HIP stream: the double-buffered stepping of RL samplers (the policy works on one group's observations while
  another group steps).  Work of different groups is unordered, so consecutive steps of different groups
  overlap on the GPU and hide each launch's fill and drain (bench.py `extra`, `*_2_groups_2_streams`).  Each group's `global_env_offset` is set, so device-side reset sampling draws the episodes of
  one `num_envs` batch."""

  def __init__(self, num_groups=2, num_envs=2, device=0, **kwargs):
    if num_envs % num_groups:
      raise ValueError('num_envs must be a multiple of num_groups')
    per = num_envs // num_groups
    base = int(kwargs.pop('global_env_offset', 0))
    self.streams = [torch.cuda.Stream(device=torch.device('cuda', device)) for _ in range(num_groups)]
    self.groups = []
    for g in range(num_groups):
      with torch.cuda.stream(self.streams[g]):
        self.groups.append(BatchedEnvironment(num_envs=per, device=device, global_env_offset=base + g * per, **kwargs))

  def __len__(self):
    return len(self.groups)

  def reset(self, g):
    with torch.cuda.stream(self.streams[g]):
      return self.groups[g].reset()

  def step(self, g, actions, active=None):
    """Steps group `g` on its stream; the returned tensors are valid on `self.streams[g]`.  `active`: the group's mask, as in
    `BatchedEnvironment.step`."""
    with torch.cuda.stream(self.streams[g]):
      return self.groups[g].step(actions, active=active)

  def sample_actions(self, g, where='host', click='uniform'):
    """`BatchedEnvironment.sample_actions` of group `g`; the device forms run on its stream.  The groups' global_env_offset
    keeps their device streams apart under one seed."""
    with torch.cuda.stream(self.streams[g]):
      return self.groups[g].sample_actions(where=where, click=click)

  def rollout_random(self, g, num_candidates, num_steps, click='uniform', keep_steps=False):
    """`BatchedEnvironment.rollout_random` of group `g`, on its stream; the returned tensors are valid on `self.streams[g]`.
    The groups' global_env_offset keeps their candidates' streams apart under one seed."""
    with torch.cuda.stream(self.streams[g]):
      return self.groups[g].rollout_random(num_candidates, num_steps, click=click, keep_steps=keep_steps)

  def rollout_guided(self, g, num_candidates, num_steps, sprite_weights=None, motion_mean=0.5, motion_std=0.25, keep_steps=False):
    """`BatchedEnvironment.rollout_guided` of group `g`, on its stream; the plan tensors must be valid on `self.streams[g]`, as
    the returned ones are."""
    with torch.cuda.stream(self.streams[g]):
      return self.groups[g].rollout_guided(num_candidates, num_steps, sprite_weights=sprite_weights, motion_mean=motion_mean,
                                           motion_std=motion_std, keep_steps=keep_steps)

  def synchronize(self):
    for s in self.streams:
      s.synchronize()

  def close(self):
    self.synchronize()
    for env in self.groups:
      env.close()


class Environment(object):
  """Single environment with the reference's exact return types (dm_env.TimeStep of numpy).

  `device_reset` defaults to False here -- unlike BatchedEnvironment's 'auto' -- on purpose: the N = 1 form exists to be
  swapped for the reference class (example_run_loop.py:62-80), and calling `init_sprites()` on the host at every reset keeps
  the episodes those of the reference under the same np.random.seed().

  The episode sequence is the reference's: the k-th call of `init_sprites()` plays the same part in both.  Call 0 -- pool
  entry 0 -- is the sprites the reference's CONSTRUCTOR draws (`self._sprites = self._init_sprites()`, environment.py:68):
  what `state()`, `observation()`, `success()` ... see before the first step, never an episode that is stepped; the first
  `reset()` / `step()` plays call 1, the next one call 2, ...  Whether the caller looks at the state first changes nothing
  (the pool, `episodes_per_pool` calls, is drawn up front and again when it is used up)."""

  def __init__(self, task, action_space, renderers, init_sprites, keep_in_frame=True,
               max_episode_length=1000, metadata=None, episodes_per_pool=32, device=0,
               action_dtype=np.float64, device_reset=False):
    self._batched = BatchedEnvironment(
        task, action_space, renderers, init_sprites, keep_in_frame=keep_in_frame,
        max_episode_length=max_episode_length, metadata=metadata, num_envs=1,
        episodes_per_env=episodes_per_pool, device=device, action_dtype=action_dtype, check_errors=1,
        device_reset=device_reset)
    self._episodes_per_pool = episodes_per_pool
    self._episodes_used = 0
    self._reset_next_step = True
    self._started = False           # the constructor's sprites (pool entry 0) are on the device

  @property
  def action_space(self):
    return self._batched.action_space

  def action_spec(self):
    return self._batched.action_spec()

  def observation_spec(self):
    return self._batched.observation_spec()

  def reward_spec(self):
    """dm_env.Environment's default (the reference does not override it): a float scalar."""
    return dm_env.specs.Array(shape=(), dtype=float, name='reward')

  def discount_spec(self):
    """dm_env.Environment's default: a float scalar in [0, 1]."""
    return dm_env.specs.BoundedArray(shape=(), dtype=float, minimum=0., maximum=1., name='discount')

  def _convert(self, ts):
    step_type = dm_env.StepType(int(ts.step_type[0].item()))
    obs = {}
    for k, v in ts.observation.items():
      a = v[0].cpu().numpy()
      obs[k] = bool(a) if a.shape == () else a
    if step_type == dm_env.StepType.FIRST:
      return dm_env.TimeStep(step_type, None, None, obs)
    return dm_env.TimeStep(step_type, float(ts.reward[0].item()), float(ts.discount[0].item()), obs)

  def _maybe_refill(self):
    # a fresh draw of init_sprites() per episode, like the reference; the pool is re-drawn when used up
    if self._episodes_used >= self._episodes_per_pool:
      self._batched.refill_pool()
      self._episodes_used = 0
    self._episodes_used += 1

  def reset(self):
    self._ensure_started()
    self._maybe_refill()
    ts = self._convert(self._batched.reset())
    self._reset_next_step = False
    return ts

  def step(self, action):
    if self._reset_next_step:
      return self.reset()
    a = np.asarray(action)[None]
    ts = self._convert(self._batched.step(a))
    if ts.last():
      self._reset_next_step = True
    return ts

  # ---- the rest of the reference's public surface (environment.py:80-86,110-142), acting on the device state
  def _ensure_started(self):
    """The reference's constructor already holds sprites (`self._sprites = self._init_sprites()`, environment.py:68), so
    its introspection methods work before the first step: pool entry 0 is put on the device for them, once, by the first
    call of anything -- `reset()` included, so the episodes that are stepped start with entry 1 whether or not anybody
    looked at the constructor's sprites.  The first `step()` still resets (environment.py:90-91), as the reference does."""
    if not self._started:
      self._started = True
      self._maybe_refill()
      self._batched.reset()

  def success(self):
    """environment.py:80-81: `task.success(sprites)` of the sprites as they are NOW -- evaluated on the device (swb_evaluate:
    the cover kernel's task phase, no time step), so that a setter or `set_positions` since the last step is seen, as the
    reference sees it."""
    self._ensure_started()
    return bool(self._batched.engine.evaluate()[0].item())

  def should_terminate(self):
    """environment.py:83-86."""
    self._ensure_started()
    timeout = self._batched.engine.env_state(0)['step_count'] >= self._batched._max_episode_length  # pylint: disable=protected-access
    out_of_frame = any([s.out_of_frame for s in self.sprites])
    return self.success() or out_of_frame or timeout

  def sample_contained_position(self):
    """environment.py:110-126: a random sprite (np.random.randint), then a random position inside it."""
    sprites = self.sprites
    return sprites[np.random.randint(len(sprites))].sample_contained_position()

  def observation(self):
    """environment.py:136-142: every renderer's view of the current state, rendered now (swb_render: the cover and
    resample kernels without a state change), as numpy values."""
    self._ensure_started()
    obs = {}
    for k, v in self._batched.observation().items():
      a = v[0].cpu().numpy()
      obs[k] = bool(a) if a.shape == () else a
    return obs

  def state(self):
    """environment.py:128-134: {'sprites': [...], 'global_state': {'success': ..., 'metadata': ...}} -- the sprites as
    `LiveSprite` handles on the device state (attributes read and, for shape / angle / scale, assigned like the reference's).
    The structure-of-arrays state (x, y, step_count, ...) is `soa_state()`."""
    global_state = {'success': self.success()}
    if self._batched._metadata:  # pylint: disable=protected-access
      global_state['metadata'] = self._batched._metadata  # pylint: disable=protected-access
    return {'sprites': self.sprites, 'global_state': global_state}

  def soa_state(self):
    """Host copies of the live structure-of-arrays state (swb_get_state): x, y f64[1, S], n_sprites, step_count, ..."""
    return self._batched.state()

  @property
  def sprites(self):
    """The current episode's sprites (reference: `env.state()['sprites']`) as `sprite.LiveSprite` handles whose
    shape / angle / scale can be assigned like on the reference's Sprite (sprite.py:152-175)."""
    self._ensure_started()
    return self._batched.sprites(0)

  def close(self):
    self._batched.close()
