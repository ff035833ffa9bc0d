"""Thin Python handle on the HIP engine: device buffers are torch tensors.

PyTorch is used here for device memory and streams only; all computation is in
libswb.so.  One `Engine` = one `swb_handle` = N environments on one GPU.
"""
import ctypes as C

import numpy as np
import torch

from spriteworld_amd import _abi
from spriteworld_amd import _lib
from spriteworld_amd import lanczos
from spriteworld_amd import shapes as _shapes


def _ptr(a):
  return None if a is None else C.c_void_p(a.ctypes.data)


class Snapshot(object):
  """The state of C environments (swb_snapshot): the nine tensors x, y f64[C, S], n_sprites, pool_entry, step_count, episode,
  pool_base, pool_len i32[C] and reset_next u8[C], the id of the pool they were saved under (`pool_id`) and S (`max_sprites`).
  `len()` is C.  `.cpu()` / `.to(device)` return a copy elsewhere (a checkpoint and its way back); the tensors are plain torch
  tensors and may be indexed, stacked or saved like any.  A snapshot means something only beside the pool it was saved under:
  `Engine.get_pool()` is the other half of a checkpoint."""

  FIELDS = ('x', 'y', 'n_sprites', 'pool_entry', 'step_count', 'episode', 'pool_base', 'pool_len', 'reset_next')
  _DTYPES = dict(x=torch.float64, y=torch.float64, reset_next=torch.uint8)

  def __init__(self, tensors, pool_id, max_sprites):
    self.pool_id, self.max_sprites = int(pool_id), int(max_sprites)
    for k in self.FIELDS:
      setattr(self, k, tensors[k])

  @classmethod
  def empty(cls, C, S, device, pool_id=0):
    """C slots that no state has been saved into yet: each an environment without sprites that resets through pool entry 0 at
    its next step -- what a slot `save_state` leaves untouched (an index out of range) loads as."""
    new = lambda k: torch.zeros((C, S) if k in ('x', 'y') else (C,), dtype=cls._DTYPES.get(k, torch.int32), device=device)
    tensors = {k: new(k) for k in cls.FIELDS}
    tensors['pool_len'].fill_(1)
    tensors['reset_next'].fill_(1)
    return cls(tensors, pool_id, S)

  def __len__(self):
    return int(self.n_sprites.shape[0])

  @property
  def device(self):
    return self.x.device

  def to(self, device):
    return Snapshot({k: getattr(self, k).to(device, copy=True) for k in self.FIELDS}, self.pool_id, self.max_sprites)

  def cpu(self):
    return self.to(torch.device('cpu'))

  def as_struct(self):
    s = _abi.SwbSnapshot()
    for k in self.FIELDS:
      t = getattr(self, k)
      want = (len(self), self.max_sprites) if k in ('x', 'y') else (len(self),)
      if tuple(t.shape) != want or t.dtype != self._DTYPES.get(k, torch.int32) or not t.is_contiguous():
        raise ValueError('Snapshot.%s must be a contiguous %s%s tensor, got %s %s' % (k, self._DTYPES.get(k, torch.int32), list(want),
                                                                                   t.dtype, tuple(t.shape)))
      setattr(s, k, t.data_ptr())
    return s


class Engine(object):
  """N batched environments on one MI355X (`cfg`: _abi.SwbConfig, `pool`: lowering.Pool)."""

  # Where the library runs: these four members and `_stream()` are all that knows of the GPU.  (The CPU test suite runs this
  # very class over the kernel sources compiled for the host by overriding them: tests/_emu_engine.py.)
  _check = staticmethod(_lib.check)      # status of a C call -> SwbError with the library's message

  def _open(self, device):
    """(the loaded library, the torch device the buffers live on)"""
    if not torch.cuda.is_available():
      raise _lib.SwbError('no GPU visible: the Spriteworld engine has no CPU path')
    return _lib.load(), torch.device('cuda', device)

  def _device_scope(self):
    return torch.cuda.device(self.device)

  def _sync(self):
    torch.cuda.synchronize(self.device)

  def _stream(self):
    return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

  def __init__(self, cfg, pool, device=0, task_sets=None):
    """task_sets: a list of _abi.SwbTaskSet (swb_set_task_sets), installed before the pool; `pool.task_set` then names the set
    of every entry.  None: one task for the whole batch, the one `cfg` holds."""
    self.lib, self.device = self._open(device)
    self.cfg = cfg
    self.N, self.S = cfg.n_envs, cfg.max_sprites
    # the reference's np.array(image) is [image_size[1], image_size[0], 3]
    self.obs_shape = (cfg.image_w, cfg.image_h, 3)
    h = C.c_void_p()
    self._check(self.lib.swb_create(C.byref(cfg), device, C.byref(h)))
    self._h = h
    verts, offs = _shapes.packed_table()
    self._check(self.lib.swb_upload_shapes(self._h, _ptr(verts), _ptr(offs), len(offs) - 1))
    aa = cfg.anti_aliasing
    if aa != 1:
      for axis, out_size in ((0, cfg.image_h), (1, cfg.image_w)):
        bounds, coeffs = lanczos.resample_tables(aa * out_size, out_size)
        bounds = np.ascontiguousarray(bounds)
        coeffs = np.ascontiguousarray(coeffs)
        self._check(self.lib.swb_upload_resample(self._h, axis, out_size, coeffs.shape[1],
                                                 _ptr(bounds), _ptr(coeffs)))
    self.pool = None
    self.task_set_table = None
    if task_sets is not None:
      self.set_task_sets(task_sets)
    if pool is not None:
      self.set_pool(pool)
    with self._device_scope():
      self.obs = torch.zeros((self.N,) + self.obs_shape, dtype=torch.uint8, device=self.device)
      self.reward = torch.zeros(self.N, dtype=torch.float64, device=self.device)
      self.discount = torch.zeros(self.N, dtype=torch.float32, device=self.device)
      self.step_type = torch.zeros(self.N, dtype=torch.uint8, device=self.device)
      self.success = torch.zeros(self.N, dtype=torch.uint8, device=self.device)
      self.error = torch.zeros(self.N, dtype=torch.uint8, device=self.device)
    self._outs = self._make_outs(render=True)
    self._outs_norender = self._make_outs(render=False)
    self._rendered = 0        # rendering launches so far (the run lists are trimmed after TRIM_AFTER of them)
    self._rollout_M = 0       # candidates of the last rollout (rollout_frames)
    self._rollout_K = 0       # ... and its steps, when it kept them (rollout(keep_steps=True); 0: it did not)

  TRIM_AFTER = 3

  def _make_outs(self, render):
    o = _abi.SwbOutputs()
    o.obs = self.obs.data_ptr() if render else None
    o.reward = self.reward.data_ptr()
    o.discount = self.discount.data_ptr()
    o.step_type = self.step_type.data_ptr()
    o.success = self.success.data_ptr()
    o.error = self.error.data_ptr()
    return o

  def close(self):
    if getattr(self, '_h', None):
      self._sync()
      self.lib.swb_destroy(self._h)
      self._h = None

  def __del__(self):
    try:
      self.close()
    except Exception:  # pylint: disable=broad-except
      pass

  def set_task_sets(self, task_sets):
    """Installs the table of task sets (a list of _abi.SwbTaskSet; swb_set_task_sets): once, before any pool.  From then on
    the task of an episode is the set its pool entry names (`Pool.task_set`, `set_entry_task_sets`); rollouts are refused."""
    table = (_abi.SwbTaskSet * len(task_sets))(*task_sets)
    self._check(self.lib.swb_set_task_sets(self._h, len(task_sets), table))
    self.task_set_table = list(task_sets)

  @property
  def num_task_sets(self):
    return len(self.task_set_table) if self.task_set_table is not None else 0

  def set_pool(self, pool):
    if getattr(pool, 'task_set', None) is not None and self.task_set_table is None:
      raise ValueError('the pool names a task set per entry (Pool.task_set) but the engine has no task sets (set_task_sets)')
    self.pool = pool
    cpool = pool.as_struct()
    self._check(self.lib.swb_set_pool(self._h, C.byref(cpool)))
    self._rendered = 0        # (a new pool restores the lists' full reservation: trimmed again after TRIM_AFTER launches)
    if getattr(pool, 'task_set', None) is not None:       # (right after the pool: swb_set_pool put every entry in set 0)
      self.set_entry_task_sets(pool.task_set)

  def _n_pool_entries(self):
    return self.pool.n_entries if self.pool is not None else getattr(self, '_pool_entries', 0)

  def set_entry_task_sets(self, set_of_entry):
    """The set of every pool entry (u8[P]; swb_set_entry_task_sets): takes effect at once, for running episodes too.
    The labels are the pool's: an entry moved to another set is evaluated against the label rows of THAT set's sub-tasks as
    the pool holds them.  `lowering.lower_task_sets` and the device samplers fill every row of every entry;
    `lowering.merge_task_sets` (`workloads.build_task_sets`) fills only the rows of the set an entry was built for -- its scenes
    come from different workloads --, the others are 0: on such a pool reassign only after filling those rows yourself."""
    a = np.ascontiguousarray(set_of_entry)
    if a.shape != (self._n_pool_entries(),) or a.dtype.kind not in 'iub':
      raise ValueError('set_entry_task_sets takes an integer array of shape [%d], got %s %s' % (self._n_pool_entries(), a.dtype, a.shape))
    if a.size and (a.min() < 0 or a.max() > 255):
      raise ValueError('set_entry_task_sets: a task set index outside [0, 255]')
    a = np.ascontiguousarray(a, dtype=np.uint8)
    self._check(self.lib.swb_set_entry_task_sets(self._h, _ptr(a), self._stream()))
    if self.pool is not None:
      self.pool.task_set = a.copy()

  def entry_task_sets(self):
    """u8[P]: the set of every pool entry as the device holds it (swb_get_entry_task_sets; blocking)."""
    a = np.zeros(self._n_pool_entries(), np.uint8)
    self._check(self.lib.swb_get_entry_task_sets(self._h, _ptr(a)))
    return a

  def task_sets(self):
    """i32[N] device tensor: the task set of the episode every environment is in (swb_env_task_sets: one small kernel,
    asynchronous) -- what an agent trained on a mix of tasks conditions on.  The tensor is the engine's and is overwritten
    by the next call."""
    if getattr(self, '_env_sets', None) is None:
      with self._device_scope():
        self._env_sets = torch.zeros(self.N, dtype=torch.int32, device=self.device)
    self._check(self.lib.swb_env_task_sets(self._h, C.c_void_p(self._env_sets.data_ptr()), self._stream()))
    return self._env_sets

  def sample_pool(self, spec, n_entries, pool_base, pool_len, seed, first_entry=0):
    """Draws `n_entries` episodes on the device from an _abi.SwbSampler (swb_sample_pool)."""
    base = np.ascontiguousarray(pool_base, dtype=np.int32)
    length = np.ascontiguousarray(pool_len, dtype=np.int32)
    assert base.shape == (self.N,) and length.shape == (self.N,)
    self._check(self.lib.swb_sample_pool(self._h, C.byref(spec), int(n_entries), _ptr(base), _ptr(length),
                                         C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), C.c_uint64(int(first_entry)),
                                         self._stream()))
    self.pool = None
    self._pool_entries = int(n_entries)
    self._rendered = 0

  def sample_pool_tree(self, spec, n_entries, pool_base, pool_len, seed, first_entry=0):
    """`sample_pool` for an _abi.SwbTreeSampler (swb_sample_pool_tree): any tree of factor distributions, labels per sprite,
    tasks that key on position included."""
    base = np.ascontiguousarray(pool_base, dtype=np.int32)
    length = np.ascontiguousarray(pool_len, dtype=np.int32)
    assert base.shape == (self.N,) and length.shape == (self.N,)
    self._check(self.lib.swb_sample_pool_tree(self._h, C.byref(spec), int(n_entries), _ptr(base), _ptr(length),
                                              C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), C.c_uint64(int(first_entry)),
                                              self._stream()))
    self.pool = None
    self._pool_entries = int(n_entries)
    self._rendered = 0

  def sampler_exhausted(self):
    """Sprites of the last tree (re)sampling whose retry budget ran out (swb_sampler_exhausted; blocking)."""
    n = C.c_int64(0)
    self._check(self.lib.swb_sampler_exhausted(self._h, C.byref(n), self._stream()))
    return n.value

  def resample_pool(self, seed, first_entry=0):
    """Fresh episodes in every pool entry no environment is playing; nothing is reset (swb_resample_pool)."""
    self._check(self.lib.swb_resample_pool(self._h, C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF),
                                           C.c_uint64(int(first_entry)), self._stream()))

  def get_pool(self):
    """Host copy (lowering.Pool) of the pool the device currently holds."""
    from spriteworld_amd import lowering
    n = self.pool.n_entries if self.pool is not None else self._pool_entries
    pool = lowering.Pool(n, self.S, self.cfg.n_tasks)
    pool.pool_base = np.zeros(self.N, np.int32)
    pool.pool_len = np.zeros(self.N, np.int32)
    if any(t.n_xcuts + t.n_ycuts for t in self.cfg.tasks[:self.cfg.n_tasks]):     # a task keys on position
      pool.cell_label = np.zeros((n, self.cfg.n_tasks, self.S, _abi.SWB_MAX_CELLS), np.int8)
    cpool = pool.as_struct()
    self._check(self.lib.swb_get_pool(self._h, C.byref(cpool)))
    if self.task_set_table is not None:
      pool.task_set = self.entry_task_sets()
    return pool

  def reset_all(self):
    self._check(self.lib.swb_reset_all(self._h, self._stream()))

  def _mask_tensor(self, mask, what):
    """Contiguous uint8 device tensor of a bool or uint8 mask of shape [N] (tensor or array)."""
    t = mask if isinstance(mask, torch.Tensor) else None
    if t is None:
      try:
        t = torch.as_tensor(np.ascontiguousarray(mask))
      except (TypeError, ValueError, RuntimeError):
        raise ValueError('%s must be a bool or uint8 tensor or array of shape [%d], got %r' % (what, self.N, type(mask)))
    if t.dtype not in (torch.bool, torch.uint8) or tuple(t.shape) != (self.N,):
      raise ValueError('%s must be a bool or uint8 tensor or array of shape [%d], got %s %s' % (what, self.N, t.dtype, tuple(t.shape)))
    return t.to(device=self.device, dtype=torch.uint8).contiguous()

  def reset_envs(self, mask):
    """Environment.reset() for the environments of `mask` (bool or uint8 [N]; swb_reset_envs: one small kernel, asynchronous):
    the next step in which such an environment is active is a FIRST step from its next pool entry.  The others are untouched and
    go on keeping their run lists and cached frames."""
    m = self._mask_tensor(mask, 'reset_envs mask')
    self._last_reset_mask = m  # keep alive until the launch is consumed
    self._check(self.lib.swb_reset_envs(self._h, C.c_void_p(m.data_ptr()), self._stream()))

  def step(self, actions, render=True, active=None):
    """actions: device tensor f64[N,4] (f32 if cfg.action_is_f32) or i32[N,2] (Embodied).
    active: None, or a bool or uint8 mask of shape [N] (swb_step_masked).  An environment whose entry is 0 takes no part in the
    step: its state does not change, a pending reset stays pending, its action row is never read (NaN is fine) and its entries
    of reward, discount, step_type, success and error keep the values of its last active step; `obs` holds the frame of its
    current state all the same."""
    if self.cfg.action_space == _abi.ACTION_EMBODIED:
      want = torch.int32
    else:
      want = torch.float32 if self.cfg.action_is_f32 else torch.float64
    if not isinstance(actions, torch.Tensor):
      actions = torch.as_tensor(np.ascontiguousarray(actions), device=self.device)
    if actions.dtype != want or actions.device != self.device or not actions.is_contiguous():
      actions = actions.to(device=self.device, dtype=want).contiguous()
    assert actions.numel() == self.N * (2 if want == torch.int32 else 4), actions.shape
    self._last_actions = actions  # keep alive until the launch is consumed
    outs = self._outs if render else self._outs_norender
    if active is None:
      self._check(self.lib.swb_step(self._h, C.c_void_p(actions.data_ptr()), C.byref(outs),
                                    self._stream()))
    else:
      m = self._mask_tensor(active, 'step active')
      self._last_active = m  # keep alive until the launch is consumed
      self._check(self.lib.swb_step_masked(self._h, C.c_void_p(actions.data_ptr()), C.c_void_p(m.data_ptr()), C.byref(outs),
                                           self._stream()))
    if render:
      self._rendered += 1
      if self._rendered == self.TRIM_AFTER:
        self.trim()

  def rollout(self, actions, positions=False, keep_steps=False):
    """Scores M candidate action sequences of K steps per environment from the CURRENT state without stepping it
    (swb_rollout: two kernels, asynchronous, the live state untouched).  actions: [K, N, M, 4] float (f32 if
    cfg.action_is_f32) or [K, N, M, 2] int32 (Embodied).  Returns a dict of fresh device tensors in the C layout: reward
    f64, discount f32, step_type u8, success u8 -- all [K, N, M], entry [k, n, m] what step k + 1 of environment n would
    return under actions[k, n, m] -- and error u8[N, M] (swb_env_error bits of the K steps); with `positions`, also x, y
    f64[N, M, S] and n_sprites i32[N, M] after step K.  With `keep_steps` (swb_rollout_trajectory) the engine also keeps the
    state after every step, for `rollout_frames(step=...)`, and with `positions` returns x_steps, y_steps f64[K, N, M, S]
    and n_sprites_steps i32[K, N, M] too: entry [k] the state after step k + 1.  The scratch state belongs to the handle:
    issue the rollouts of one engine on one stream (or order the streams yourself)."""
    if self.cfg.action_space == _abi.ACTION_EMBODIED:
      want, width = torch.int32, 2
    else:
      want, width = (torch.float32 if self.cfg.action_is_f32 else torch.float64), 4
    if not isinstance(actions, torch.Tensor):
      actions = torch.as_tensor(np.ascontiguousarray(actions), device=self.device)
    if actions.dim() != 4 or actions.shape[1] != self.N or actions.shape[3] != width:
      raise ValueError('rollout actions must be [K, %d, M, %d], got %s' % (self.N, width, tuple(actions.shape)))
    if actions.dtype != want or actions.device != self.device or not actions.is_contiguous():
      actions = actions.to(device=self.device, dtype=want).contiguous()
    K, _, M, _ = actions.shape
    with self._device_scope():
      new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=self.device)
      res = {'reward': new((K, self.N, M), torch.float64), 'discount': new((K, self.N, M), torch.float32),
             'step_type': new((K, self.N, M), torch.uint8), 'success': new((K, self.N, M), torch.uint8),
             'error': torch.zeros((self.N, M), dtype=torch.uint8, device=self.device)}
      if positions:
        res.update(x=new((self.N, M, self.S), torch.float64), y=new((self.N, M, self.S), torch.float64),
                   n_sprites=new((self.N, M), torch.int32))
      steps = {}
      if positions and keep_steps:
        steps = {'x': new((K, self.N, M, self.S), torch.float64), 'y': new((K, self.N, M, self.S), torch.float64),
                 'n_sprites': new((K, self.N, M), torch.int32)}
    o = _abi.SwbRolloutOutputs()
    for k, t in res.items():
      setattr(o, k, t.data_ptr())
    self._last_rollout_actions = actions  # keep alive until the launch is consumed
    self._rollout_M = self._rollout_K = 0
    if keep_steps:
      so = _abi.SwbRolloutStepOutputs()
      for k, t in steps.items():
        setattr(so, k, t.data_ptr())
      self._check(self.lib.swb_rollout_trajectory(self._h, C.c_void_p(actions.data_ptr()), int(M), int(K), C.byref(o), C.byref(so),
                                                  self._stream()))
      self._rollout_K = int(K)
      res.update((k + '_steps', t) for k, t in steps.items())
    else:
      self._check(self.lib.swb_rollout(self._h, C.c_void_p(actions.data_ptr()), int(M), int(K), C.byref(o), self._stream()))
    self._rollout_M = int(M)
    return res

  def rollout_sampled(self, mode, seed, M, K, first_env=0, positions=False, keep_steps=False, outputs=('actions',)):
    """A rollout whose M x K candidate actions per environment are drawn by the rollout kernel itself, step by step, from the
    state each candidate has reached (swb_rollout_sampled: two kernels, asynchronous, the live state untouched).  mode:
    _abi.SAMPLE_UNIFORM or _abi.SAMPLE_ON_SPRITE (every click inside a randomly chosen sprite, where the candidate's sprites
    are at that step); candidate m of environment n draws Philox stream (`first_env + n`, 1 + m) of key `seed`.  Returns the
    dict of `rollout(..., positions, keep_steps)` plus the `outputs` asked for among 'actions' ([K, N, M, 4] f64, f32 if
    cfg.action_is_f32, or [K, N, M, 2] i32 for Embodied: what was drawn, the layout `rollout` takes -- always drawn, the
    library requires the buffer), 'sprite' and 'tries' (i32[K, N, M], SAMPLE_ON_SPRITE only).  Afterwards the engine holds a
    rollout as after `rollout`: `rollout_frames` works."""
    if self.cfg.action_space == _abi.ACTION_EMBODIED:
      a_dtype, width = torch.int32, 2
    else:
      a_dtype, width = (torch.float32 if self.cfg.action_is_f32 else torch.float64), 4
    M, K = int(M), int(K)
    layout = {'actions': ((K, self.N, M, width), a_dtype), 'sprite': ((K, self.N, M), torch.int32), 'tries': ((K, self.N, M), torch.int32)}
    unknown = [k for k in outputs if k not in layout]
    if unknown:
      raise ValueError('rollout_sampled outputs must be among %s, got %s' % (sorted(layout), unknown))
    if M <= 0 or K <= 0:
      raise ValueError('rollout_sampled: M and K must be positive, got M = %d, K = %d' % (M, K))
    self._rollout_M = self._rollout_K = 0
    with self._device_scope():
      new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=self.device)
      res = {'reward': new((K, self.N, M), torch.float64), 'discount': new((K, self.N, M), torch.float32),
             'step_type': new((K, self.N, M), torch.uint8), 'success': new((K, self.N, M), torch.uint8),
             'error': torch.zeros((self.N, M), dtype=torch.uint8, device=self.device)}
      if positions:
        res.update(x=new((self.N, M, self.S), torch.float64), y=new((self.N, M, self.S), torch.float64),
                   n_sprites=new((self.N, M), torch.int32))
      steps = {}
      if positions and keep_steps:
        steps = {'x': new((K, self.N, M, self.S), torch.float64), 'y': new((K, self.N, M, self.S), torch.float64),
                 'n_sprites': new((K, self.N, M), torch.int32)}
      drawn = {k: new(*layout[k]) for k in set(outputs) | {'actions'}}
    o, so, sa = _abi.SwbRolloutOutputs(), _abi.SwbRolloutStepOutputs(), _abi.SwbRolloutSampledOutputs()
    for k, t in res.items():
      setattr(o, k, t.data_ptr())
    for k, t in steps.items():
      setattr(so, k, t.data_ptr())
    for k, t in drawn.items():
      setattr(sa, k, t.data_ptr())
    self._last_rollout_actions = drawn['actions']  # keep alive until the launch is consumed
    self._check(self.lib.swb_rollout_sampled(self._h, int(mode), C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), C.c_uint64(int(first_env)),
                                             M, K, int(bool(keep_steps)), C.byref(o), C.byref(so) if keep_steps else None, C.byref(sa),
                                             self._stream()))
    self._rollout_M, self._rollout_K = M, (K if keep_steps else 0)
    res.update((k + '_steps', t) for k, t in steps.items())
    res.update((k, drawn[k]) for k in outputs)
    return res

  def rollout_guided(self, seed, M, K, choice_cdf=None, width=None, motion_mean=None, motion_std=None, first_env=0, positions=False,
                     keep_steps=False, outputs=('actions', 'sprite')):
    """A rollout whose candidates are drawn by the rollout kernel from a plan distribution per (step, environment)
    (swb_rollout_guided: two kernels, asynchronous, the live state untouched): a categorical over sprite indices, a uniform
    point inside the chosen sprite where the candidate has it at that step, and a motion mean + std * z clipped to [0, 1], z
    Irwin-Hall (n = 4) with mean 0 and variance 1.  choice_cdf: f64[K, N, W] device tensor of running sums of non-negative
    weights along W, or None (uniform choice; `width` then defaults to max_sprites, 8 for Embodied); motion_mean, motion_std:
    f64[K, N, 2] device tensors, required for SelectMove / DragAndDrop and None for Embodied (W = 8: index = carry * 4 +
    direction).  The streams are `rollout_sampled`'s.  Returns the dict of `rollout(..., positions, keep_steps)` plus the
    `outputs` asked for among 'actions' (as `rollout_sampled`'s), 'sprite' (i32[K, N, M]: the chosen sprite, -1 without
    sprites; Embodied: the chosen index) and 'tries' (i32[K, N, M], not for Embodied).  Afterwards the engine holds a rollout
    as after `rollout`."""
    embodied = self.cfg.action_space == _abi.ACTION_EMBODIED
    if embodied:
      a_dtype, a_width = torch.int32, 2
    else:
      a_dtype, a_width = (torch.float32 if self.cfg.action_is_f32 else torch.float64), 4
    M, K = int(M), int(K)
    layout = {'actions': ((K, self.N, M, a_width), a_dtype), 'sprite': ((K, self.N, M), torch.int32), 'tries': ((K, self.N, M), torch.int32)}
    unknown = [k for k in outputs if k not in layout]
    if unknown:
      raise ValueError('rollout_guided outputs must be among %s, got %s' % (sorted(layout), unknown))
    if M <= 0 or K <= 0:
      raise ValueError('rollout_guided: M and K must be positive, got M = %d, K = %d' % (M, K))

    def plan_tensor(t, last, what):
      if t is None:
        return None
      if not isinstance(t, torch.Tensor) or t.dim() != 3 or tuple(t.shape[:2]) != (K, self.N) or (last is not None and t.shape[2] != last):
        raise ValueError('rollout_guided: %s must be a tensor [%d, %d, %s], got %s' % (
            what, K, self.N, 'W' if last is None else last, tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__))
      if t.dtype != torch.float64 or t.device != self.device or not t.is_contiguous():
        t = t.to(device=self.device, dtype=torch.float64).contiguous()
      return t

    cdf = plan_tensor(choice_cdf, None, 'choice_cdf')
    mean, std = plan_tensor(motion_mean, 2, 'motion_mean'), plan_tensor(motion_std, 2, 'motion_std')
    if width is None:
      width = int(cdf.shape[2]) if cdf is not None else (8 if embodied else self.S)
    if cdf is not None and cdf.shape[2] != int(width):
      raise ValueError('rollout_guided: choice_cdf has %d columns, width is %d' % (cdf.shape[2], int(width)))
    self._rollout_M = self._rollout_K = 0
    with self._device_scope():
      new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=self.device)
      res = {'reward': new((K, self.N, M), torch.float64), 'discount': new((K, self.N, M), torch.float32),
             'step_type': new((K, self.N, M), torch.uint8), 'success': new((K, self.N, M), torch.uint8),
             'error': torch.zeros((self.N, M), dtype=torch.uint8, device=self.device)}
      if positions:
        res.update(x=new((self.N, M, self.S), torch.float64), y=new((self.N, M, self.S), torch.float64),
                   n_sprites=new((self.N, M), torch.int32))
      steps = {}
      if positions and keep_steps:
        steps = {'x': new((K, self.N, M, self.S), torch.float64), 'y': new((K, self.N, M, self.S), torch.float64),
                 'n_sprites': new((K, self.N, M), torch.int32)}
      drawn = {k: new(*layout[k]) for k in set(outputs) | {'actions'}}
    o, so, sa, plan = _abi.SwbRolloutOutputs(), _abi.SwbRolloutStepOutputs(), _abi.SwbRolloutSampledOutputs(), _abi.SwbRolloutPlan()
    for k, t in res.items():
      setattr(o, k, t.data_ptr())
    for k, t in steps.items():
      setattr(so, k, t.data_ptr())
    for k, t in drawn.items():
      setattr(sa, k, t.data_ptr())
    plan.width = int(width)
    for k, t in (('choice_cdf', cdf), ('motion_mean', mean), ('motion_std', std)):
      if t is not None:
        setattr(plan, k, t.data_ptr())
    self._last_rollout_actions = (drawn['actions'], cdf, mean, std)  # keep alive until the launch is consumed
    self._check(self.lib.swb_rollout_guided(self._h, C.byref(plan), C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), C.c_uint64(int(first_env)),
                                            M, K, int(bool(keep_steps)), C.byref(o), C.byref(so) if keep_steps else None, C.byref(sa),
                                            self._stream()))
    self._rollout_M, self._rollout_K = M, (K if keep_steps else 0)
    res.update((k + '_steps', t) for k, t in steps.items())
    res.update((k, drawn[k]) for k in outputs)
    return res

  def rollout_frames(self, candidates=None, step=None):
    """The frames the candidates of the LAST rollout end in (swb_rollout_frames: the render path of this engine on the
    rollout's scratch state, asynchronous, on the rollout's stream; the live state, `self.obs`, `self.error` and the pool
    untouched).  Returns a dict of fresh device tensors: obs u8[N, M, H, W, 3] -- frame [n, m] what step K of environment n
    would have rendered under candidate m -- and error u8[N, M] (swb_env_error bits of the render phases, zero-initialised).
    With `candidates` (int[N], tensor or array; values outside [0, M) are clamped into it) only the frame of candidate
    candidates[n] of environment n is rendered: obs u8[N, H, W, 3], error u8[N].  Raises when no rollout preceded it, or the
    pool has changed since.  Not a rendering step as far as `trim()` after TRIM_AFTER launches is concerned.
    `step` (swb_rollout_step_frames, after `rollout(keep_steps=True)`): an int k in [0, K) renders the states after step k + 1
    in the same two forms; 'all' needs `candidates` and renders candidates[n] after every step: obs u8[K, N, H, W, 3], error
    u8[K, N].  Raises when the last rollout kept no steps."""
    if isinstance(step, str):
      if step != 'all':
        raise ValueError("rollout_frames step must be an int or 'all', got %r" % (step,))
      if candidates is None:
        raise ValueError("rollout_frames step='all' needs candidates: loop over the steps for the frames of all candidates")
      step = _abi.SWB_ALL_STEPS
    elif step is not None and int(step) < 0:     # (not an index from the end: -1 is SWB_ALL_STEPS in the C ABI)
      raise ValueError('rollout_frames step must be in [0, K), got %d' % int(step))
    M = self._rollout_M
    if not M or (step is not None and not self._rollout_K):     # (the library refuses: no rollout has run, or it kept no steps)
      if step is None:
        self._check(self.lib.swb_rollout_frames(self._h, 0, None, None, None, self._stream()))
      self._check(self.lib.swb_rollout_step_frames(self._h, M, int(step), None, None, None, self._stream()))
    cand = None
    if candidates is not None:
      cand = candidates if isinstance(candidates, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(candidates))
      if cand.dim() != 1 or cand.shape[0] != self.N or cand.is_floating_point():
        raise ValueError('rollout_frames candidates must be int[%d], got %s %s' % (self.N, cand.dtype, tuple(cand.shape)))
      cand = cand.to(device=self.device, dtype=torch.int32).contiguous()
    lead = (self.N,) if cand is not None else (self.N, M)
    if step == _abi.SWB_ALL_STEPS:
      lead = (self._rollout_K,) + lead
    with self._device_scope():
      res = {'obs': torch.empty(lead + self.obs_shape, dtype=torch.uint8, device=self.device),
             'error': torch.zeros(lead, dtype=torch.uint8, device=self.device)}
    self._last_rollout_candidates = cand  # keep alive until the launch is consumed
    cand_p, obs_p, err_p = (None if cand is None else C.c_void_p(cand.data_ptr()), C.c_void_p(res['obs'].data_ptr()),
                            C.c_void_p(res['error'].data_ptr()))
    if step is None:
      self._check(self.lib.swb_rollout_frames(self._h, M, cand_p, obs_p, err_p, self._stream()))
    else:
      self._check(self.lib.swb_rollout_step_frames(self._h, M, int(step), cand_p, obs_p, err_p, self._stream()))
    return res

  def sample_actions(self, mode, seed, first_env=0, outputs=('actions',)):
    """Random-agent actions drawn on the device from the sprites as they are now (swb_sample_actions: one kernel,
    asynchronous, the handle only read).  mode: _abi.SAMPLE_UNIFORM or _abi.SAMPLE_ON_SPRITE (a click inside a randomly chosen
    sprite); environment n draws Philox stream `first_env + n` of key `seed`.  `outputs`: which of 'actions' (f64[N, 4], f32
    if cfg.action_is_f32, or i32[N, 2] for Embodied: what step() takes), 'position' (f64[N, 2]), 'sprite' (i32[N]) and
    'tries' (i32[N]) to return -- the last three with SAMPLE_ON_SPRITE only.  Returns a dict of fresh device tensors."""
    if self.cfg.action_space == _abi.ACTION_EMBODIED:
      shape, dtype = (self.N, 2), torch.int32
    else:
      shape, dtype = (self.N, 4), (torch.float32 if self.cfg.action_is_f32 else torch.float64)
    layout = {'actions': (shape, dtype), 'position': ((self.N, 2), torch.float64), 'sprite': ((self.N,), torch.int32),
              'tries': ((self.N,), torch.int32)}
    unknown = [k for k in outputs if k not in layout]
    if unknown:
      raise ValueError('sample_actions outputs must be among %s, got %s' % (sorted(layout), unknown))
    with self._device_scope():
      res = {k: torch.empty(layout[k][0], dtype=layout[k][1], device=self.device) for k in outputs}
    o = _abi.SwbSampledActions()
    for k, t in res.items():
      setattr(o, k, t.data_ptr())
    self._check(self.lib.swb_sample_actions(self._h, int(mode), C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF),
                                            C.c_uint64(int(first_env)), C.byref(o), self._stream()))
    return res

  def trim(self):
    """Cuts the hand-off lists between the two kernels of a step from their start-up reservation (any scene of convex sprites:
    133 KB per environment on 12 sprites at 128x128) down to 1.25 x what the launches so far needed, plus a shared arena for the
    lists that outgrow that (swb_trim_run_lists; blocking, once -- `step()` calls it after its third rendering launch, so it
    falls into any warm-up).  Returns the units of 8 bytes a list owns afterwards.  Results never change."""
    if not hasattr(self.lib, 'swb_trim_run_lists'):      # (an A/B build of an older revision)
      return None
    cap = C.c_int32(0)
    self._check(self.lib.swb_trim_run_lists(self._h, C.byref(cap), self._stream()))
    return cap.value

  def list_stats(self):
    """(kept, built): the cover waves of rendering launches that handed on the run lists already in memory / built them, since
    the engine was created (swb_list_stats; blocking).  Needs SWB_LIST_STATS in the environment when the engine is created."""
    kept, built = C.c_int64(0), C.c_int64(0)
    self._check(self.lib.swb_list_stats(self._h, C.byref(kept), C.byref(built), self._stream()))
    return kept.value, built.value

  def task_stats(self):
    """(reused, evaluated): the environment-steps -- environments that took part in a step -- that took the task's reward,
    success and error bits from the engine's task cache / evaluated the task, since the engine was created (swb_task_stats;
    blocking).  Needs SWB_LIST_STATS like list_stats."""
    reused, evaluated = C.c_int64(0), C.c_int64(0)
    self._check(self.lib.swb_task_stats(self._h, C.byref(reused), C.byref(evaluated), self._stream()))
    return reused.value, evaluated.value

  def frame_stats(self):
    """(copied, filled, resampled): the tasks of the resample kernel -- one per environment, column group and band task of a
    rendering launch -- that copied their part of the frame from the engine's frame cache / resampled it and left it in the
    cache / only resampled it, since the engine was created (swb_frame_stats; blocking).  Needs SWB_LIST_STATS like list_stats."""
    w = [C.c_int64(0) for _ in range(3)]
    self._check(self.lib.swb_frame_stats(self._h, C.byref(w[0]), C.byref(w[1]), C.byref(w[2]), self._stream()))
    return tuple(x.value for x in w)

  def split_stats(self):
    """(whole, bands, whole_copies): the tasks of the resample kernel of a handle in split-bands mode (variant()['split_bands'])
    that took a frame's whole rows and resampled or filled / one band of them / the whole rows and copied, since the engine was
    created (swb_split_stats; blocking).  Needs SWB_LIST_STATS like list_stats."""
    w = [C.c_int64(0) for _ in range(3)]
    self._check(self.lib.swb_split_stats(self._h, C.byref(w[0]), C.byref(w[1]), C.byref(w[2]), self._stream()))
    return tuple(x.value for x in w)

  def frame_cycles(self):
    """(cycles of the copying tasks, cycles of all other tasks, list bytes those walked): measurement (swb_frame_cycles)."""
    w = (C.c_int64 * 3)()
    self._check(self.lib.swb_frame_cycles(self._h, w, self._stream()))
    return tuple(w)

  def spec_copy_stats(self):
    """The copy workgroups of the cover launches -- one per environment and column group of a rendering launch -- that copied
    from the frame cache, since the engine was created (swb_spec_copy_stats; blocking): the frames counted by frame_stats as
    copied, plus the copies a resample task overwrote.  Needs SWB_LIST_STATS like list_stats."""
    w = C.c_int64(0)
    self._check(self.lib.swb_spec_copy_stats(self._h, C.byref(w), self._stream()))
    return w.value

  def render(self):
    self._check(self.lib.swb_render(self._h, C.c_void_p(self.obs.data_ptr()), self._stream()))
    return self.obs

  def evaluate(self):
    """task.success() of the sprites as they are now (environment.py:80-81), into `self.success`: after sprite setters or
    set_positions the flag of the last step no longer describes them."""
    self._check(self.lib.swb_evaluate(self._h, C.c_void_p(self.success.data_ptr()), self._stream()))
    return self.success

  def factors(self):
    """SpriteFactors observation: f64 [N, S, 10] device tensor (FACTOR_NAMES order, shape as ShapeType id)."""
    if getattr(self, '_factors', None) is None:
      self._factors = torch.zeros((self.N, self.S, 10), dtype=torch.float64, device=self.device)
    self._check(self.lib.swb_factors(self._h, C.c_void_p(self._factors.data_ptr()), self._stream()))
    return self._factors

  def state(self):
    st = {
        'x': np.zeros((self.N, self.S)), 'y': np.zeros((self.N, self.S)),
        'n_sprites': np.zeros(self.N, np.int32), 'pool_entry': np.zeros(self.N, np.int32),
        'step_count': np.zeros(self.N, np.int32), 'reset_next': np.zeros(self.N, np.uint8),
        'episode': np.zeros(self.N, np.int32),
    }
    cs = _abi.SwbState(*[a.ctypes.data for a in (st['x'], st['y'], st['n_sprites'], st['pool_entry'],
                                                  st['step_count'], st['reset_next'], st['episode'])])
    self._check(self.lib.swb_get_state(self._h, C.byref(cs), self._stream()))
    return st

  def env_state(self, env):
    """dict(n_sprites, pool_entry, step_count, episode, reset_next) of ONE environment (swb_get_env_state: a few bytes,
    whatever the batch size)."""
    out = np.zeros(5, np.int32)
    self._check(self.lib.swb_get_env_state(self._h, int(env), _ptr(out), self._stream()))
    return dict(zip(('n_sprites', 'pool_entry', 'step_count', 'episode', 'reset_next'), (int(v) for v in out)))

  def sprite_types(self, env, sprite):
    """(angle is np.float32, scale is np.float32) for a sprite of the episode `env` is playing: the types the reference's
    Sprite holds (swb_pool::attr_f32, recorded by lowering / the device sampler)."""
    f = C.c_int32(0)
    self._check(self.lib.swb_get_sprite_types(self._h, int(env), int(sprite), C.byref(f), self._stream()))
    return bool(f.value & 1), bool(f.value & 2)

  def set_positions(self, x, y):
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    self._check(self.lib.swb_set_positions(self._h, _ptr(x), _ptr(y), self._stream()))

  # ------------------------------------------------------------------ snapshots (swb_save_state / swb_load_state / swb_copy_pool)
  def pool_id(self):
    """The id of the pool the handle holds (swb_pool_id): renewed by every call that installs or redraws it, 0 without one."""
    v = C.c_uint64(0)
    self._check(self.lib.swb_pool_id(self._h, C.byref(v)))
    return v.value

  def _index_tensor(self, values, what):
    """int32 device tensor of a 1-D integer index (tensor or array)."""
    t = values if isinstance(values, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(values))
    if t.dim() != 1 or t.is_floating_point():
      raise ValueError('%s must be a 1-D integer tensor or array, got %s %s' % (what, t.dtype, tuple(t.shape)))
    return t.to(device=self.device, dtype=torch.int32).contiguous()

  def save_state(self, index=None, source='live'):
    """A `Snapshot` of the environments `index` (int[C], tensor or array; None: all N, in order), as fresh device tensors
    (swb_save_state: one kernel, asynchronous, the handle only read).  source='rollout': the states the candidates of the last
    rollout ended in -- index n * M + m is candidate m of environment n, None all N * M; raises where `rollout_frames` would.
    A slot whose index is out of range is left as `Snapshot.empty` made it."""
    if source not in ('live', 'rollout'):
      raise ValueError("save_state source is 'live' or 'rollout', got %r" % (source,))
    idx = None if index is None else self._index_tensor(index, 'save_state index')
    n_src = self.N * self._rollout_M if source == 'rollout' else self.N
    count = int(idx.shape[0]) if idx is not None else max(n_src, 1)      # (no rollout: the library refuses)
    with self._device_scope():
      snap = Snapshot.empty(count, self.S, self.device, self.pool_id())
    cs = snap.as_struct()
    self._last_state_index = idx  # keep alive until the launch is consumed
    self._check(self.lib.swb_save_state(self._h, _abi.STATE_ROLLOUT_END if source == 'rollout' else _abi.STATE_LIVE,
                                        None if idx is None else C.c_void_p(idx.data_ptr()), count, C.byref(cs), self._stream()))
    return snap

  def load_state(self, snapshot, slots=None, check_pool=True):
    """Environment n takes slot slots[n] of `snapshot` (int[N], tensor or array; -1: the environment stays exactly as it is;
    None: slot n, and the snapshot must hold N) -- swb_load_state: one kernel, asynchronous; from the next launch on a loaded
    environment behaves bit for bit as its source would have.  A slot value outside [-1, len(snapshot)) leaves the environment
    alone and is counted (`load_rejected()`).  Raises when the snapshot was saved under another pool than the handle holds now,
    unless check_pool=False: the caller vouches that the pool is the one the snapshot was saved under (a run resumed from
    `get_pool()` + `set_pool()`).  A snapshot on another device is copied over first.  `self.obs`, the outputs of the last
    step, the sticky error buffer and a held rollout are not touched; `resample_pool()` is refused afterwards (the pool ranges
    may have moved between environments) until `set_pool` / `sample_pool`."""
    if snapshot.max_sprites != self.S:
      raise ValueError('the snapshot holds %d sprites per environment, the engine %d' % (snapshot.max_sprites, self.S))
    if snapshot.device != self.device:
      snapshot = snapshot.to(self.device)
    sl = None if slots is None else self._index_tensor(slots, 'load_state slots')
    if sl is not None and sl.shape[0] != self.N:
      raise ValueError('load_state slots must be int[%d], got %s' % (self.N, tuple(sl.shape)))
    if getattr(self, '_rejected', None) is None:
      self._rejected = torch.zeros(1, dtype=torch.int32, device=self.device)
    cs = snapshot.as_struct()
    self._last_loaded = (snapshot, sl)  # keep alive until the launch is consumed
    self._check(self.lib.swb_load_state(self._h, C.byref(cs), len(snapshot), None if sl is None else C.c_void_p(sl.data_ptr()),
                                        C.c_uint64(snapshot.pool_id if check_pool else 0), C.c_void_p(self._rejected.data_ptr()),
                                        self._stream()))

  def load_rejected(self):
    """Slot values outside [-1, C) that `load_state` calls have met since the last call of this; reads and clears the word
    (blocking)."""
    if getattr(self, '_rejected', None) is None:
      return 0
    n = int(self._rejected.item())
    if n:
      self._rejected.zero_()
    return n

  def copy_pool_from(self, other, pool_base, pool_len):
    """The device pool of engine `other` copied into this one, device to device (swb_copy_pool); environment n of this engine
    resets through entries [pool_base[n], pool_base[n] + pool_len[n]).  This engine takes over `other`'s pool id -- snapshots
    of `other` load here -- and every environment is marked "reset on next step", as after `set_pool`."""
    base = np.ascontiguousarray(pool_base, dtype=np.int32)
    length = np.ascontiguousarray(pool_len, dtype=np.int32)
    if base.shape != (self.N,) or length.shape != (self.N,):
      raise ValueError('copy_pool_from: pool_base and pool_len must be int[%d]' % self.N)
    self._check(self.lib.swb_copy_pool(self._h, other._h, _ptr(base), _ptr(length), self._stream()))
    self.pool = None
    self._pool_entries = other.pool.n_entries if other.pool is not None else other._pool_entries
    self._rendered = 0        # (the lists' full reservation is back: trimmed again after TRIM_AFTER launches)

  def set_sprite_attr(self, env, sprite, attr, value, delta=None, label=None, cell_label=None):
    """sprite.py:152-175 setters on a live sprite (swb_set_sprite_attr; attr: _abi.ATTR_SHAPE / ATTR_ANGLE / ATTR_SCALE).
    cell_label: i8[n_tasks, SWB_MAX_CELLS], the sprite's labels per cell for tasks that key on position."""
    d = None if delta is None else C.byref(C.c_double(float(delta)))
    lab = None if label is None else np.ascontiguousarray(label, dtype=np.int8)
    self._check(self.lib.swb_set_sprite_attr(self._h, int(env), int(sprite), int(attr), float(value), d, _ptr(lab),
                                             self._stream()))
    if cell_label is not None:
      cells = np.ascontiguousarray(cell_label, dtype=np.int8)
      assert cells.shape == (self.cfg.n_tasks, _abi.SWB_MAX_CELLS), cells.shape
      self._check(self.lib.swb_set_sprite_cell_labels(self._h, int(env), int(sprite), _ptr(cells), self._stream()))

  def get_sprite(self, env, sprite):
    """dict(shape=index, angle, scale, path=f64[n,2]): the sprite as the engine currently sees it (swb_get_sprite)."""
    shape, nv = C.c_int32(0), C.c_int32(0)
    angle, scale = C.c_double(0.0), C.c_double(0.0)
    path = np.zeros((_abi.SWB_MAX_SHAPE_VERTS, 2), dtype=np.float64)
    self._check(self.lib.swb_get_sprite(self._h, int(env), int(sprite), C.byref(shape), C.byref(angle), C.byref(scale),
                                        C.byref(nv), _ptr(path), self._stream()))
    return {'shape': shape.value, 'angle': angle.value, 'scale': scale.value, 'path': path[:nv.value].copy()}

  def outputs_host(self):
    self._sync()
    return {k: getattr(self, k).to('cpu', copy=True).numpy()       # (host copies, wherever the buffers live)
            for k in ('obs', 'reward', 'discount', 'step_type', 'success', 'error')}

  def variant(self):
    """dict(nw, ncol, vs, lds_bytes_per_wave, waves_per_simd, kernel, build_id): the step kernel this engine launches."""
    info = _abi.SwbVariantInfo()
    self._check(self.lib.swb_variant(self._h, C.byref(info)))
    d = {k: getattr(info, k) for k, _ in _abi.SwbVariantInfo._fields_}
    d['cover_kernel'] = 'swb_cover_kernel<%d>' % info.nw
    if info.many_sprites:                # (more than 16 sprites: no cover kernel, the state phase is a kernel of its own)
      d['cover_kernel'] = 'none'
      d['state_kernel'] = 'swb_ms_state_kernel'
    if info.large_frames:
      if not info.many_sprites:
        d['cover_kernel'] += ' (state phase only)'
      d['kernel'] = 'swb_lf_raster_kernel' + ('' if self.cfg.anti_aliasing == 1 else ' + swb_lf_vertical_kernel')
    else:
      d['kernel'] = ('swb_resample_kernel<%d>' % info.vs if info.vs else
                     ('none (the cover kernel paints the frame)' if info.paint_in_cover else 'swb_fill_kernel'))
    d['build_id'] = self.lib.swb_build_id().decode()
    return d

  def timing(self, enable):
    """Three HIP events per step (before the cover kernel, between the two kernels, after the second): `step_time_ms()` /
    `kernel_times_ms()` read them.  A diagnostic: each event is a completion signal the device has to raise between two
    kernels that would otherwise follow each other directly -- measured, a run of back-to-back steps is 6 % slower with
    them (tools/exp_timing_overhead.py), so time a run with ONE pair of events around it and use this mode for the split."""
    self._check(self.lib.swb_timing_enable(self._h, int(enable)))

  def step_time_ms(self):
    ms, n = C.c_double(0.0), C.c_int64(0)
    self._check(self.lib.swb_step_time_ms(self._h, C.byref(ms), C.byref(n)))
    return ms.value, n.value

  def kernel_times_ms(self):
    """(cover ms, resample / fill ms, launches) since timing(True): the step interval split between its two kernels."""
    a, b, n = C.c_double(0.0), C.c_double(0.0), C.c_int64(0)
    self._check(self.lib.swb_kernel_times_ms(self._h, C.byref(a), C.byref(b), C.byref(n)))
    return a.value, b.value, n.value
