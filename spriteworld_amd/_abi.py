"""ctypes mirror of include/swb.h (struct layouts and enums of the C ABI)."""
import ctypes as C

SWB_MAX_SPRITES = 64
SWB_TUNED_SPRITES = 16      # handles of more sprites take the many-sprite path (swb_variant_info::many_sprites)
SWB_MAX_TASKS = 8
SWB_MAX_SHAPES = 32
SWB_MAX_SHAPE_VERTS = 64
SWB_MAX_GROUPS = 8
SWB_MAX_CUTS = 4
SWB_MAX_CELLS = (SWB_MAX_CUTS + 1) * (SWB_MAX_CUTS + 1)
SWB_MAX_CANDIDATES = 12

# enum swb_action_space
ACTION_SELECT_MOVE, ACTION_DRAG_AND_DROP, ACTION_EMBODIED = 0, 1, 2
# enum swb_task_kind
TASK_NO_REWARD, TASK_FIND_GOAL, TASK_CLUSTERING = 0, 1, 2
# enum swb_meta_aggregator / swb_meta_termination
AGG_SUM, AGG_MAX, AGG_MIN, AGG_MEAN = 0, 1, 2, 3
TERM_ALL, TERM_ANY = 0, 1
# enum swb_step_type (== dm_env.StepType)
STEP_FIRST, STEP_MID, STEP_LAST = 0, 1, 2
# enum swb_env_error
ENV_ERR_DB_ZERO, ENV_ERR_DB_LABELS, ENV_ERR_SPAN_OVERFLOW = 1, 2, 4
# enum swb_sprite_attr
ATTR_SHAPE, ATTR_ANGLE, ATTR_SCALE = 0, 1, 2
# enum swb_action_sampling
SAMPLE_UNIFORM, SAMPLE_ON_SPRITE = 0, 1
SWB_CONTAINED_MAX_TRIES = 1024


class SwbTask(C.Structure):
  _fields_ = [
      ('kind', C.c_int32),
      ('sparse_reward', C.c_int32),
      ('goal_position', C.c_double * 2),
      ('weights_dimensions', C.c_double * 2),
      ('terminate_distance', C.c_double),
      ('raw_reward_multiplier', C.c_double),
      ('terminate_bonus', C.c_double),
      ('termination_threshold', C.c_double),
      ('reward_range', C.c_double),
      ('n_xcuts', C.c_int32),
      ('n_ycuts', C.c_int32),
      ('xcuts', C.c_double * SWB_MAX_CUTS),
      ('ycuts', C.c_double * SWB_MAX_CUTS),
  ]


class SwbConfig(C.Structure):
  _fields_ = [
      ('n_envs', C.c_int32),
      ('max_sprites', C.c_int32),
      ('image_h', C.c_int32),
      ('image_w', C.c_int32),
      ('anti_aliasing', C.c_int32),
      ('bg_rgb', C.c_uint8 * 4),
      ('action_space', C.c_int32),
      ('action_scale', C.c_double),
      ('motion_cost', C.c_double),
      ('keep_in_frame', C.c_int32),
      ('max_episode_length', C.c_int32),
      ('pos_is_f32', C.c_int32),
      ('n_tasks', C.c_int32),
      ('is_meta', C.c_int32),
      ('meta_aggregator', C.c_int32),
      ('meta_termination', C.c_int32),
      ('action_is_f32', C.c_int32),
      ('meta_terminate_bonus', C.c_double),
      ('tasks', SwbTask * SWB_MAX_TASKS),
  ]


SWB_MAX_TASK_SETS = 8


class SwbTaskSet(C.Structure):
  """swb_task_set: a range of SwbConfig.tasks with the aggregation and the time limit of one reference task."""
  _fields_ = [
      ('first_task', C.c_int32),
      ('n_tasks', C.c_int32),
      ('is_meta', C.c_int32),
      ('meta_aggregator', C.c_int32),
      ('meta_termination', C.c_int32),
      ('max_episode_length', C.c_int32),
      ('meta_terminate_bonus', C.c_double),
  ]


class SwbPool(C.Structure):
  _fields_ = [
      ('n_entries', C.c_int32),
      ('n_sprites', C.c_void_p),
      ('x', C.c_void_p),
      ('y', C.c_void_p),
      ('x_vel', C.c_void_p),
      ('y_vel', C.c_void_p),
      ('scale', C.c_void_p),
      ('cos_a', C.c_void_p),
      ('sin_a', C.c_void_p),
      ('shape', C.c_void_p),
      ('rgb', C.c_void_p),
      ('label', C.c_void_p),
      ('cell_label', C.c_void_p),
      ('pool_base', C.c_void_p),
      ('pool_len', C.c_void_p),
      ('angle', C.c_void_p),
      ('color', C.c_void_p),
      ('attr_f32', C.c_void_p),
  ]


class SwbOutputs(C.Structure):
  _fields_ = [
      ('obs', C.c_void_p),
      ('reward', C.c_void_p),
      ('discount', C.c_void_p),
      ('step_type', C.c_void_p),
      ('success', C.c_void_p),
      ('error', C.c_void_p),
  ]


class SwbRolloutOutputs(C.Structure):
  _fields_ = [
      ('reward', C.c_void_p),
      ('discount', C.c_void_p),
      ('step_type', C.c_void_p),
      ('success', C.c_void_p),
      ('error', C.c_void_p),
      ('x', C.c_void_p),
      ('y', C.c_void_p),
      ('n_sprites', C.c_void_p),
  ]


class SwbRolloutStepOutputs(C.Structure):
  _fields_ = [
      ('x', C.c_void_p),
      ('y', C.c_void_p),
      ('n_sprites', C.c_void_p),
  ]


SWB_ALL_STEPS = -1


class SwbSampledActions(C.Structure):
  _fields_ = [
      ('actions', C.c_void_p),
      ('position', C.c_void_p),
      ('sprite', C.c_void_p),
      ('tries', C.c_void_p),
  ]


class SwbRolloutSampledOutputs(C.Structure):
  _fields_ = [
      ('actions', C.c_void_p),
      ('sprite', C.c_void_p),
      ('tries', C.c_void_p),
  ]


class SwbRolloutPlan(C.Structure):
  _fields_ = [
      ('choice_cdf', C.c_void_p),
      ('width', C.c_int32),
      ('motion_mean', C.c_void_p),
      ('motion_std', C.c_void_p),
  ]


class SwbState(C.Structure):
  _fields_ = [
      ('x', C.c_void_p),
      ('y', C.c_void_p),
      ('n_sprites', C.c_void_p),
      ('pool_entry', C.c_void_p),
      ('step_count', C.c_void_p),
      ('reset_next', C.c_void_p),
      ('episode', C.c_void_p),
  ]


class SwbSnapshot(C.Structure):
  _fields_ = [
      ('x', C.c_void_p),
      ('y', C.c_void_p),
      ('n_sprites', C.c_void_p),
      ('pool_entry', C.c_void_p),
      ('step_count', C.c_void_p),
      ('episode', C.c_void_p),
      ('pool_base', C.c_void_p),
      ('pool_len', C.c_void_p),
      ('reset_next', C.c_void_p),
  ]


# enum swb_state_source
STATE_LIVE, STATE_ROLLOUT_END = 0, 1


class SwbVariantInfo(C.Structure):
  _fields_ = [('nw', C.c_int32), ('ncol', C.c_int32), ('vs', C.c_int32), ('lds_bytes_per_wave', C.c_int32),
              ('waves_per_simd', C.c_int32), ('resample_waves_per_simd', C.c_int32), ('n_bands', C.c_int32),
              ('n_column_groups', C.c_int32), ('run_cap', C.c_int32), ('paint_in_cover', C.c_int32),
              ('arena_units', C.c_int32), ('large_frames', C.c_int32), ('many_sprites', C.c_int32), ('reserved_', C.c_int32),
              ('run_list_bytes', C.c_int64), ('frame_cache_bytes', C.c_int64),
              ('split_bands', C.c_int32), ('split_pad_', C.c_int32), ('task_cache_bytes', C.c_int64)]


FACTOR_UNIFORM_F32, FACTOR_UNIFORM_INT, FACTOR_DISCRETE = 0, 1, 2


class SwbFactor(C.Structure):
  _fields_ = [
      ('kind', C.c_int32),
      ('n', C.c_int32),
      ('lo', C.c_double),
      ('hi', C.c_double),
      ('cand', C.c_double * SWB_MAX_CANDIDATES),
  ]


FACTOR_ORDER = ('x', 'y', 'scale', 'angle', 'c0', 'c1', 'c2', 'x_vel', 'y_vel')   # enum swb_factor_index
SWB_N_FACTORS = len(FACTOR_ORDER)
SWB_MAX_HOLDOUTS = 2


class SwbHoldout(C.Structure):
  _fields_ = [
      ('redraw_mask', C.c_uint32),
      ('box_mask', C.c_uint32),
      ('lo', C.c_double * SWB_N_FACTORS),
      ('hi', C.c_double * SWB_N_FACTORS),
  ]


class SwbSpriteGroup(C.Structure):

  def factor(self, key):
    return self.factors[FACTOR_ORDER.index(key)]

  _fields_ = [
      ('count_min', C.c_int32),
      ('count_max', C.c_int32),
      ('factors', SwbFactor * SWB_N_FACTORS),
      ('n_holdouts', C.c_int32),
      ('reserved', C.c_int32),
      ('holdouts', SwbHoldout * SWB_MAX_HOLDOUTS),
      ('n_shapes', C.c_int32),
      ('shapes', C.c_int32 * SWB_MAX_CANDIDATES),
      ('cos_a', C.c_double * SWB_MAX_CANDIDATES),
      ('sin_a', C.c_double * SWB_MAX_CANDIDATES),
      ('label', C.c_int8 * SWB_MAX_TASKS),
  ]


SWB_MAX_ALTERNATIVES = 16


class SwbAlternative(C.Structure):
  _fields_ = [
      ('n', C.c_int32),
      ('group', C.c_int32 * SWB_MAX_GROUPS),
  ]


class SwbSampler(C.Structure):
  _fields_ = [
      ('n_groups', C.c_int32),
      ('shuffle', C.c_int32),
      ('color_map', C.c_int32),
      ('n_alternatives', C.c_int32),
      ('alternatives', SwbAlternative * SWB_MAX_ALTERNATIVES),
      ('deg_cos', C.c_double * 360),
      ('deg_sin', C.c_double * 360),
      ('groups', SwbSpriteGroup * SWB_MAX_GROUPS),
  ]


# swb_tree_sampler (swb_sample_pool_tree): leaves, postfix predicates and one bytecode program per sprite group
SWB_TREE_MAX_LEAVES, SWB_TREE_MAX_PRED_NODES, SWB_TREE_MAX_PREDS, SWB_TREE_MAX_OPS = 64, 128, 64, 128
SWB_TREE_MAX_CHOICES, SWB_TREE_MAX_STACK, SWB_TREE_MAX_CLUSTERS = 16, 32, 16
SWB_F_SHAPE = SWB_N_FACTORS
SWB_TREE_N_FACTORS = SWB_N_FACTORS + 1
TREE_FACTOR_ORDER = FACTOR_ORDER + ('shape',)
SWB_TREE_DEFAULT_MAX_TRIES = 10000
# enum swb_pred_op / swb_tree_op_kind
PRED_LEAF, PRED_AND, PRED_OR, PRED_ANDNOT, PRED_TRUE = 0, 1, 2, 3, 4
OP_DRAW, OP_CHOOSE, OP_JUMP, OP_TEST = 0, 1, 2, 3


class SwbTreeLeaf(C.Structure):
  _fields_ = [
      ('factor', C.c_int32),
      ('kind', C.c_int32),
      ('n', C.c_int32),
      ('weighted', C.c_int32),
      ('shape_mask', C.c_uint32),
      ('reserved', C.c_uint32),
      ('lo', C.c_double),
      ('hi', C.c_double),
      ('lo32', C.c_double),
      ('hi32', C.c_double),
      ('cand', C.c_double * SWB_MAX_CANDIDATES),
      ('cand32', C.c_double * SWB_MAX_CANDIDATES),
      ('cdf', C.c_double * SWB_MAX_CANDIDATES),
      ('cos_a', C.c_double * SWB_MAX_CANDIDATES),
      ('sin_a', C.c_double * SWB_MAX_CANDIDATES),
  ]


class SwbPredNode(C.Structure):
  _fields_ = [('op', C.c_int16), ('leaf', C.c_int16)]


class SwbTreePred(C.Structure):
  _fields_ = [('first', C.c_int16), ('n', C.c_int16)]


class SwbTreeOp(C.Structure):
  _fields_ = [('kind', C.c_int16), ('a', C.c_int16), ('b', C.c_int16), ('c', C.c_int16)]


class SwbTreeChoice(C.Structure):
  _fields_ = [
      ('n', C.c_int32),
      ('reserved', C.c_int32),
      ('target', C.c_int32 * SWB_MAX_CANDIDATES),
      ('cdf', C.c_double * SWB_MAX_CANDIDATES),
  ]


class SwbTreeGroup(C.Structure):
  _fields_ = [
      ('count_min', C.c_int32),
      ('count_max', C.c_int32),
      ('first_op', C.c_int32),
      ('n_ops', C.c_int32),
      ('defaults', C.c_double * SWB_TREE_N_FACTORS),
      ('default_cos', C.c_double),
      ('default_sin', C.c_double),
  ]


class SwbTreeTask(C.Structure):
  _fields_ = [
      ('kind', C.c_int32),
      ('n_preds', C.c_int32),
      ('pred', C.c_int16 * SWB_TREE_MAX_CLUSTERS),
  ]


class SwbTreeSampler(C.Structure):
  _fields_ = [
      ('n_groups', C.c_int32),
      ('shuffle', C.c_int32),
      ('color_map', C.c_int32),
      ('n_alternatives', C.c_int32),
      ('alternatives_weighted', C.c_int32),
      ('max_tries', C.c_int32),
      ('n_leaves', C.c_int32),
      ('n_pred_nodes', C.c_int32),
      ('n_preds', C.c_int32),
      ('n_ops', C.c_int32),
      ('n_choices', C.c_int32),
      ('n_tasks', C.c_int32),
      ('alternatives', SwbAlternative * SWB_MAX_ALTERNATIVES),
      ('alternative_cdf', C.c_double * SWB_MAX_ALTERNATIVES),
      ('deg_cos', C.c_double * 360),
      ('deg_sin', C.c_double * 360),
      ('groups', SwbTreeGroup * SWB_MAX_GROUPS),
      ('tasks', SwbTreeTask * SWB_MAX_TASKS),
      ('choices', SwbTreeChoice * SWB_TREE_MAX_CHOICES),
      ('preds', SwbTreePred * SWB_TREE_MAX_PREDS),
      ('pred_nodes', SwbPredNode * SWB_TREE_MAX_PRED_NODES),
      ('ops', SwbTreeOp * SWB_TREE_MAX_OPS),
      ('leaves', SwbTreeLeaf * SWB_TREE_MAX_LEAVES),
  ]


_P, _h, _p, _i32, _u64, _f64 = C.POINTER, C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_double

# Every function include/swb.h declares: name -> (restype, or None for the int status; argtypes).  `_h` is the handle or
# a stream, `_p` a caller's host or device array.  The one table every loader of the C ABI applies (`declare`).
PROTOTYPES = {
    'swb_last_error': (C.c_char_p, []),
    'swb_version': (None, []),
    'swb_create': (None, [_P(SwbConfig), C.c_int, _P(C.c_void_p)]),
    'swb_destroy': (None, [_h]),
    'swb_upload_shapes': (None, [_h, _p, _p, _i32]),
    'swb_upload_resample': (None, [_h, _i32, _i32, _i32, _p, _p]),
    'swb_set_pool': (None, [_h, _P(SwbPool)]),
    'swb_sample_pool': (None, [_h, _P(SwbSampler), _i32, _p, _p, _u64, _u64, _h]),
    'swb_resample_pool': (None, [_h, _u64, _u64, _h]),
    'swb_sample_pool_tree': (None, [_h, _P(SwbTreeSampler), _i32, _p, _p, _u64, _u64, _h]),
    'swb_sampler_exhausted': (None, [_h, _P(C.c_int64), _h]),
    'swb_get_pool': (None, [_h, _P(SwbPool)]),
    'swb_reset_all': (None, [_h, _h]),
    'swb_step': (None, [_h, _p, _P(SwbOutputs), _h]),
    'swb_step_masked': (None, [_h, _p, _p, _P(SwbOutputs), _h]),
    'swb_reset_envs': (None, [_h, _p, _h]),
    'swb_render': (None, [_h, _p, _h]),
    'swb_evaluate': (None, [_h, _p, _h]),
    'swb_rollout': (None, [_h, _p, _i32, _i32, _P(SwbRolloutOutputs), _h]),
    'swb_rollout_frames': (None, [_h, _i32, _p, _p, _p, _h]),
    'swb_rollout_trajectory': (None, [_h, _p, _i32, _i32, _P(SwbRolloutOutputs), _P(SwbRolloutStepOutputs), _h]),
    'swb_rollout_step_frames': (None, [_h, _i32, _i32, _p, _p, _p, _h]),
    'swb_sample_actions': (None, [_h, _i32, _u64, _u64, _P(SwbSampledActions), _h]),
    'swb_rollout_sampled': (None, [_h, _i32, _u64, _u64, _i32, _i32, _i32, _P(SwbRolloutOutputs), _P(SwbRolloutStepOutputs),
                                   _P(SwbRolloutSampledOutputs), _h]),
    'swb_rollout_guided': (None, [_h, _P(SwbRolloutPlan), _u64, _u64, _i32, _i32, _i32, _P(SwbRolloutOutputs), _P(SwbRolloutStepOutputs),
                                  _P(SwbRolloutSampledOutputs), _h]),
    'swb_trim_run_lists': (None, [_h, _P(_i32), _h]),
    'swb_list_stats': (None, [_h, _P(C.c_int64), _P(C.c_int64), _h]),
    'swb_task_stats': (None, [_h, _P(C.c_int64), _P(C.c_int64), _h]),
    'swb_frame_stats': (None, [_h, _P(C.c_int64), _P(C.c_int64), _P(C.c_int64), _h]),
    'swb_split_stats': (None, [_h, _P(C.c_int64), _P(C.c_int64), _P(C.c_int64), _h]),
    'swb_frame_cycles': (None, [_h, _P(C.c_int64), _h]),
    'swb_spec_copy_stats': (None, [_h, _P(C.c_int64), _h]),
    'swb_factors': (None, [_h, _p, _h]),
    'swb_get_env_state': (None, [_h, _i32, _p, _h]),
    'swb_get_sprite_types': (None, [_h, _i32, _i32, _P(_i32), _h]),
    'swb_get_state': (None, [_h, _P(SwbState), _h]),
    'swb_set_positions': (None, [_h, _p, _p, _h]),
    'swb_pool_id': (None, [_h, _P(_u64)]),
    'swb_save_state': (None, [_h, _i32, _p, _i32, _P(SwbSnapshot), _h]),
    'swb_load_state': (None, [_h, _P(SwbSnapshot), _i32, _p, _u64, _p, _h]),
    'swb_copy_pool': (None, [_h, _h, _p, _p, _h]),
    'swb_set_task_sets': (None, [_h, _i32, _P(SwbTaskSet)]),
    'swb_set_entry_task_sets': (None, [_h, _p, _h]),
    'swb_get_entry_task_sets': (None, [_h, _p]),
    'swb_env_task_sets': (None, [_h, _p, _h]),
    'swb_set_sprite_attr': (None, [_h, _i32, _i32, _i32, _f64, _p, _p, _h]),
    'swb_set_sprite_cell_labels': (None, [_h, _i32, _i32, _p, _h]),
    'swb_get_sprite': (None, [_h, _i32, _i32, _p, _p, _p, _p, _p, _h]),
    'swb_sprite_path_op': (None, [_i32, _f64, _f64, _i32, _p, _p]),
    'swb_variant': (None, [_h, _P(SwbVariantInfo)]),
    'swb_build_id': (C.c_char_p, []),
    'swb_timing_enable': (None, [_h, _i32]),
    'swb_step_time_ms': (None, [_h, _P(_f64), _P(C.c_int64)]),
    'swb_kernel_times_ms': (None, [_h, _P(_f64), _P(_f64), _P(C.c_int64)]),
}


def declare(lib, tolerate_missing=False):
  """Applies PROTOTYPES to a loaded library and returns it.  A symbol the library lacks is an AttributeError, unless
  `tolerate_missing`: an alternative build or source copy of an older revision, whose callers ask `hasattr` first."""
  for name, (restype, argtypes) in PROTOTYPES.items():
    if tolerate_missing and not hasattr(lib, name):
      continue
    fn = getattr(lib, name)
    fn.argtypes = argtypes
    if restype is not None:
      fn.restype = restype
  return lib


del _P, _h, _p, _i32, _u64, _f64
