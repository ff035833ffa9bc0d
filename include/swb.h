/*
 * swb.h -- C ABI of the MI355X-native batched Spriteworld step/render engine.
 *
 * The reference (google-deepmind/spriteworld) has no FFI / plugin registry: its
 * hot path is one duck-typed Python call chain.  This
 * header is therefore the boundary a maintainer would bind from Python
 * (ctypes) to replace, for N environments at once:
 *
 *   spriteworld/environment.py:74-78    Environment.reset
 *   spriteworld/environment.py:88-108   Environment.step
 *   spriteworld/environment.py:80-86    Environment.success / should_terminate
 *   spriteworld/action_spaces.py:65-104 SelectMove.step (+ DragAndDrop :133-137)
 *   spriteworld/action_spaces.py:172-214 Embodied.step
 *   spriteworld/tasks.py:70-81,126-158,196-245,248-296  NoReward /
 *                                       FindGoalPosition / Clustering /
 *                                       MetaAggregated reward + success
 *   spriteworld/renderers/pil_renderer.py:67-91  PILRenderer.render
 *   spriteworld/sprite.py:96-138        Sprite geometry, move, contains_point
 *
 * Conventions: every function returns 0 on success and a negative swb_status on
 * error (message via swb_last_error()); no exceptions cross the boundary; plain
 * pointers and sizes only.  "dev" pointers are HIP device pointers owned by the
 * caller (e.g. torch tensors' data_ptr()); "host" pointers are ordinary host
 * memory.  `stream` is a hipStream_t passed as void* (NULL = default stream).
 * One caller thread per handle; all launches are asynchronous w.r.t. `stream`.
 *
 * The same structs (swb_config, swb_task) are consumed by the CPU oracle
 * (oracle/sw_oracle.c) so that tests feed both sides identical inputs.
 */
#ifndef SWB_H_
#define SWB_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWB_MAX_SPRITES 64   /* per environment: one lane of a wave per sprite. Handles of up to 16 sprites run the tuned
                              * kernels; more take the many-sprite path (swb_variant_info::many_sprites) */
#define SWB_MAX_TASKS 8      /* sub-tasks of a MetaAggregated task              */
#define SWB_MAX_SHAPES 32
#define SWB_MAX_SHAPE_VERTS 64 /* per shape (reference max is 30, the "circle") */
#define SWB_MAX_CUTS 4       /* thresholds per axis of a task filter that keys on position (see swb_task)          */
#define SWB_MAX_CELLS ((SWB_MAX_CUTS + 1) * (SWB_MAX_CUTS + 1))

enum swb_status {
  SWB_OK = 0,
  SWB_ERR_INVALID = -1,   /* bad argument / unsupported configuration */
  SWB_ERR_HIP = -2,       /* HIP runtime error                        */
  SWB_ERR_NO_DEVICE = -3, /* no usable gfx950 device                  */
  SWB_ERR_STATE = -4      /* call order (e.g. step before set_pool)   */
};

/* action_spaces.py: which class the `actions` buffer is interpreted as. */
enum swb_action_space {
  SWB_ACTION_SELECT_MOVE = 0,   /* f64[N,4] (or f32, see action_is_f32)  action_spaces.py:29-111  */
  SWB_ACTION_DRAG_AND_DROP = 1, /* f64[N,4] (or f32)                     action_spaces.py:114-137 */
  SWB_ACTION_EMBODIED = 2       /* i32[N,2]  action_spaces.py:140-221 */
};

enum swb_task_kind {
  SWB_TASK_NO_REWARD = 0,  /* tasks.py:70-81   */
  SWB_TASK_FIND_GOAL = 1,  /* tasks.py:84-158  */
  SWB_TASK_CLUSTERING = 2  /* tasks.py:161-245 */
};

/* tasks.py:250-256 MetaAggregated.REWARD_AGGREGATOR / TERMINATION_CRITERION. */
enum swb_meta_aggregator { SWB_AGG_SUM = 0, SWB_AGG_MAX = 1, SWB_AGG_MIN = 2, SWB_AGG_MEAN = 3 };
enum swb_meta_termination { SWB_TERM_ALL = 0, SWB_TERM_ANY = 1 };

/* dm_env.StepType values (environment.py:78,105-108). */
enum swb_step_type { SWB_STEP_FIRST = 0, SWB_STEP_MID = 1, SWB_STEP_LAST = 2 };

/* Per-environment error bits.  swb_outputs.error is STICKY: a step ORs its bits into the buffer and
 * never clears it, so a caller that polls every k steps misses nothing; the caller zeroes the buffer
 * after reading it.  (Where the reference raises -- Davies-Bouldin ValueError / ZeroDivisionError --
 * the reward of that step is NaN and success is 0.) */
enum swb_env_error {
  SWB_ENV_OK = 0,
  SWB_ENV_ERR_DB_ZERO = 1,       /* Davies-Bouldin score exactly 0.0, by sklearn's early-outs or its regular path => reference raises
                                    ZeroDivisionError (tasks.py:215); reward NaN, success 0 */
  SWB_ENV_ERR_DB_LABELS = 2,     /* sklearn check_number_of_labels => reference raises ValueError            */
  SWB_ENV_ERR_SPAN_OVERFLOW = 4  /* internal raster span list overflow (never expected); ALSO: a sprite of the frame has a vertex whose
                                    canvas coordinate (int)(canvas size * vertex, pil_renderer.py:81-83) lies outside
                                    +-SWB_TUNED_COORD_LIMIT (tuned paths) / +-SWB_LF_COORD_LIMIT (large-frame and many-sprite paths,
                                    swb_variant_info::large_frames), or is not finite (a NaN / inf position: a diverged policy,
                                    keep_in_frame = 0).  The test is made on the double, before the conversion.  The state, rewards
                                    and step types of the step are the reference's; the FRAME of a flagged environment is
                                    unspecified (its bytes stay inside the environment's own frame) */
};
/* The canvas coordinates a render path takes.  Tuned paths: the cover kernel's edge records hold int16.  Large frames / many
 * sprites: int32 vertices whose differences must fit an int and be exact in float32. */
#define SWB_TUNED_COORD_LIMIT 32000.0
#define SWB_LF_COORD_LIMIT 16777216.0

/* One (sub-)task.  Field names follow the reference attributes they lower
 * (tasks.py:118-124 FindGoalPosition, tasks.py:189-194 Clustering). */
typedef struct swb_task {
  int32_t kind;               /* swb_task_kind                                        */
  int32_t sparse_reward;      /* _sparse_reward                                       */
  double goal_position[2];    /* FindGoal: _goal_position                             */
  double weights_dimensions[2];/* FindGoal: _weights_dimensions                       */
  double terminate_distance;  /* FindGoal: _terminate_distance                        */
  double raw_reward_multiplier;/* FindGoal: _raw_reward_multiplier                    */
  double terminate_bonus;     /* both: _terminate_bonus                               */
  double termination_threshold;/* Clustering: _termination_threshold                  */
  double reward_range;        /* Clustering: _reward_range                            */
  /* Filters / cluster distributions that key on POSITION (factors x, y): the reference evaluates
   * `contains(sprite.factors)` at every step (tasks.py:134-137, 196-205) and a sprite's membership changes as it moves.
   * Every position test of the reference's factor distributions is an interval test `lo <= v < hi`
   * (factor_distributions.py:105-112), so membership is constant on the cells of the grid the tests' bounds cut the plane
   * into: xcuts / ycuts are those bounds (ascending, as values of the position dtype: a bound compared with a float32
   * position is rounded the way numpy compares it), a sprite at (x, y) is in cell
   *   cy * (n_xcuts + 1) + cx,   cx = #{k : x >= xcuts[k]},  cy = #{k : y >= ycuts[k]},
   * and its label this step is swb_pool::cell_label[entry][task][sprite][cell].  n_xcuts = n_ycuts = 0: the task does not
   * key on position and swb_pool::label holds its labels. */
  int32_t n_xcuts, n_ycuts;
  double xcuts[SWB_MAX_CUTS];
  double ycuts[SWB_MAX_CUTS];
} swb_task;

typedef struct swb_config {
  int32_t n_envs;             /* N                                                    */
  int32_t max_sprites;        /* S <= SWB_MAX_SPRITES (per-episode count may be less); S > 16 takes the many-sprite path */
  int32_t image_h;            /* PILRenderer image_size[0]: a multiple of 4, <= 1024  */
  int32_t image_w;            /* PILRenderer image_size[1]                            */
  int32_t anti_aliasing;      /* PILRenderer anti_aliasing (>= 1).  Canvas AA*image_size[0] x AA*image_size[1]:
                               * the tuned kernels take canvases up to 640 px wide and images up to 256 columns;
                               * larger frames (canvases up to 4096 px either way, images up to 1024 columns)
                               * take the large-frame path (swb_variant_info::large_frames) */
  uint8_t bg_rgb[4];          /* PILRenderer bg_color (4th byte unused)               */
  int32_t action_space;       /* swb_action_space                                     */
  double action_scale;        /* SelectMove/DragAndDrop _scale ; Embodied _step_size  */
  double motion_cost;         /* _motion_cost                                         */
  int32_t keep_in_frame;      /* Environment keep_in_frame                            */
  int32_t max_episode_length; /* Environment max_episode_length                       */
  int32_t pos_is_f32;         /* 1: sprite positions are np.float32 arrays (config-   */
                              /* sampled sprites); 0: float64             */
  int32_t n_tasks;            /* 1 for a plain task; >=1 with is_meta                 */
  int32_t is_meta;            /* task is tasks.MetaAggregated                         */
  int32_t meta_aggregator;    /* swb_meta_aggregator                                  */
  int32_t meta_termination;   /* swb_meta_termination                                 */
  int32_t action_is_f32;      /* 1: actions are float32[N,4] (the dtype action_spec()  */
                              /* declares, action_spaces.py:62-63): motion, click point*/
                              /* and cost then follow numpy's float32 arithmetic       */
  double meta_terminate_bonus;/* MetaAggregated _terminate_bonus                      */
  swb_task tasks[SWB_MAX_TASKS];
} swb_config;

/* A pool of initial states ("what init_sprites() returned"), host memory,
 * entry-major: element e*S + s.  Entry e holds n_sprites[e] <= S sprites in
 * back-to-front order (sprite_generators.py / environment.py:75).
 * Everything static per episode is resolved on the host by the caller:
 *   cos_a/sin_a = math.cos/sin(math.radians(angle))     (sprite.py:96-101)
 *   rgb         = renderer _color_to_rgb(sprite.color)  (pil_renderer.py:82)
 *   label[t]    = FindGoal: filter_distrib.contains(factors) (tasks.py:134-137)
 *                 Clustering: first matching cluster index or -1 (tasks.py:196-205)
 *                 (evaluated once per episode: exact for every factor that cannot change inside an episode)
 *   cell_label  for tasks whose filter / cluster distributions key on x or y (swb_task::n_xcuts / n_ycuts): the same label
 *                 for every cell of the task's position grid, evaluated with the sprite's other factors -- the kernel
 *                 looks the sprite's cell up at every step, as the reference re-evaluates contains() at every step.
 *                 (Velocities are constant inside an episode: a filter on x_vel / y_vel is an ordinary label.)
 * Environment n draws entries pool_base[n] + (k mod pool_len[n]), k = 0,1,2...
 */
typedef struct swb_pool {
  int32_t n_entries;          /* P                                                    */
  const int32_t* n_sprites;   /* [P]                                                  */
  const double* x;            /* [P,S]                                                */
  const double* y;            /* [P,S]                                                */
  const double* x_vel;        /* [P,S]                                                */
  const double* y_vel;        /* [P,S]                                                */
  const double* scale;        /* [P,S]                                                */
  const double* cos_a;        /* [P,S]                                                */
  const double* sin_a;        /* [P,S]                                                */
  const int32_t* shape;       /* [P,S]  index into the uploaded shape table           */
  const uint8_t* rgb;         /* [P,S,4] (r,g,b,unused)                               */
  const int8_t* label;        /* [P,n_tasks,S]                                        */
  const int8_t* cell_label;   /* [P,n_tasks,S,SWB_MAX_CELLS]; may be NULL when no task keys on position */
  const int32_t* pool_base;   /* [N]                                                  */
  const int32_t* pool_len;    /* [N]                                                  */
  const double* angle;        /* [P,S]   degrees; only for swb_factors (may be NULL)  */
  const double* color;        /* [P,S,3] c0,c1,c2; only for swb_factors (may be NULL) */
  const uint8_t* attr_f32;    /* [P,S]   bit 0 / bit 1: the sprite's angle / scale is an np.float32 in the reference (what
                               * factor distributions draw; Discrete candidates and constructor arguments are Python numbers),
                               * so that a setter takes `a - self._angle` / `s - self._scale` in that type (sprite.py:163,173
                               * under NEP 50).  May be NULL (= all Python numbers).  swb_sample_pool records it per sprite. */
} swb_pool;

/* Device-side reset sampling: a declarative form of the sprite
 * generators the shipped configs build from Product-of-Continuous/Discrete factor distributions
 * (factor_distributions.py:81-158,268-310; sprite_generators.py:27-70,101-128).  Each group draws
 * `count` sprites (uniform integer in [count_min, count_max]) whose factors are independent; the
 * groups are concatenated in order and the z-order optionally shuffled.  Sampling uses a
 * counter-based Philox4x32-10 stream per pool entry: statistically, not bitwise, equivalent to the
 * reference's global MT19937 draws.  The value TYPES follow the reference exactly: a Continuous
 * factor is np.random.uniform(lo, hi) cast to its dtype (float32 by default, or an integer type),
 * a Discrete factor yields the Python object from its candidate list (a Python float). */
#define SWB_MAX_GROUPS 8
#define SWB_MAX_CANDIDATES 12
enum swb_factor_kind {
  SWB_FACTOR_UNIFORM_F32 = 0, /* Continuous(key, lo, hi)                 -> np.float32     */
  SWB_FACTOR_UNIFORM_INT = 1, /* Continuous(key, lo, hi, dtype='int32')  -> truncated int  */
  SWB_FACTOR_DISCRETE = 2     /* Discrete(key, candidates)               -> Python float   */
};
typedef struct swb_factor {
  int32_t kind;
  int32_t n;                          /* candidates (SWB_FACTOR_DISCRETE)                  */
  double lo, hi;                      /* [lo, hi)   (uniform kinds)                        */
  double cand[SWB_MAX_CANDIDATES];
} swb_factor;
enum swb_factor_index {
  SWB_F_X = 0, SWB_F_Y, SWB_F_SCALE, SWB_F_ANGLE, SWB_F_C0, SWB_F_C1, SWB_F_C2, SWB_F_XVEL, SWB_F_YVEL, SWB_N_FACTORS
};
/* SetMinus(base, hold_out) (factor_distributions.py:313-344): the factors in `redraw_mask` (base.keys)
 * are redrawn until they leave the box  AND_k lo[k] <= value_k < hi[k]  over `box_mask`. */
#define SWB_MAX_HOLDOUTS 2
typedef struct swb_holdout {
  uint32_t redraw_mask, box_mask;     /* bit i = factor index i                            */
  double lo[SWB_N_FACTORS], hi[SWB_N_FACTORS];
} swb_holdout;
typedef struct swb_sprite_group {
  int32_t count_min, count_max;
  /* x, y: UNIFORM_F32 only (float32 positions); angle: DISCRETE, or UNIFORM_INT within [0, 360] */
  swb_factor factors[SWB_N_FACTORS];
  int32_t n_holdouts, reserved;
  swb_holdout holdouts[SWB_MAX_HOLDOUTS];
  int32_t n_shapes, shapes[SWB_MAX_CANDIDATES];                /* shape table indices      */
  double cos_a[SWB_MAX_CANDIDATES], sin_a[SWB_MAX_CANDIDATES]; /* of angle.cand (radians)  */
  int8_t label[SWB_MAX_TASKS];                                 /* task label of the group  */
} swb_sprite_group;
/* sprite_generators.sample_generator (sprite_generators.py:73-98, uniform p): each episode uses ONE
 * alternative, a list of groups (indices into swb_sampler.groups) generated in that order. */
#define SWB_MAX_ALTERNATIVES 16
typedef struct swb_alternative {
  int32_t n;
  int32_t group[SWB_MAX_GROUPS];
} swb_alternative;
typedef struct swb_sampler {
  int32_t n_groups;
  int32_t shuffle;          /* sprite_generators.shuffle over the sprites of the first `shuffle`
                             * generated groups (0: none, >= the number generated: all); later
                             * groups keep their place, e.g. the agent body of
                             * examples/goal_finding_embodied.py:88-93                        */
  int32_t color_map;        /* 0: (c0,c1,c2) are RGB ints; 1: renderers.color_maps.hsv_to_rgb */
  int32_t n_alternatives;   /* 0: every group, in order; else one of alternatives[] per episode */
  swb_alternative alternatives[SWB_MAX_ALTERNATIVES];
  double deg_cos[360], deg_sin[360]; /* math.cos/sin(math.radians(d)) for integer degrees  */
  swb_sprite_group groups[SWB_MAX_GROUPS];
} swb_sampler;

/* The general device sampler (swb_sample_pool_tree): any tree of the reference's factor distributions
 * (factor_distributions.py: Continuous, Discrete, Product, Mixture, Intersection, SetMinus, Selection), lowered by the caller to
 *   LEAVES      one Continuous / Discrete distribution each, over one factor: what a DRAW samples and what a predicate tests;
 *   PREDICATES  `distribution.contains(factors)` as a postfix program over leaf tests; and
 *   PROGRAMS    one linear bytecode per sprite group that visits the tree in the order the reference's sample() does.
 * Groups, counts, the z-order shuffle, sample_generator alternatives (optionally weighted), the colour map, attr_f32 and the
 * Philox streams are swb_sampler's.  Task labels are evaluated PER SPRITE from the values drawn (and per cell of the position
 * grid for tasks that key on position: keyed handles are accepted).
 *
 * Types (numpy under NEP 50, as everywhere in the engine): a drawn value is an np.float32 (UNIFORM_F32), a Python number (a
 * DISCRETE candidate, a Sprite default) or an integer (UNIFORM_INT).  A leaf TEST compares an np.float32 value with its bounds /
 * candidates rounded to float32 (lo32 / hi32 / cand32, prepared by the caller) and every other value in float64 (lo / hi / cand):
 *   INTERVAL  lo <= v < hi            (Continuous.contains)
 *   MEMBER    v == one of cand[0..n)  (Discrete.contains); for the factor SWB_F_SHAPE: bit `shape index` of shape_mask.
 * A DRAW of a leaf: UNIFORM_* as swb_factor; DISCRETE index = u32 % n, or with `weighted` one uniform() u and
 * index = #{i : cdf[i] <= u} (numpy's choice(p=...): cdf = p.cumsum() / sum, computed by the caller).  For SWB_F_SHAPE cand[] holds
 * shape table indices; for SWB_F_ANGLE cos_a / sin_a those of the candidates. */
#define SWB_TREE_MAX_LEAVES 64
#define SWB_TREE_MAX_PRED_NODES 128
#define SWB_TREE_MAX_PREDS 64
#define SWB_TREE_MAX_OPS 128
#define SWB_TREE_MAX_CHOICES 16
#define SWB_TREE_MAX_STACK 32      /* predicate evaluation stack: the bits of one 32-bit word */
#define SWB_TREE_MAX_CLUSTERS 16   /* predicates per (sub-)task */
#define SWB_F_SHAPE SWB_N_FACTORS  /* `shape` as a tree factor: its value is the shape table index */
#define SWB_TREE_N_FACTORS (SWB_N_FACTORS + 1)
#define SWB_TREE_DEFAULT_MAX_TRIES 10000   /* the reference's _MAX_TRIES */
typedef struct swb_tree_leaf {
  int32_t factor;                     /* swb_factor_index, or SWB_F_SHAPE                              */
  int32_t kind;                       /* swb_factor_kind: UNIFORM_* = INTERVAL, DISCRETE = MEMBER      */
  int32_t n;                          /* candidates (DISCRETE)                                         */
  int32_t weighted;                   /* DISCRETE: draw through cdf[]                                  */
  uint32_t shape_mask, reserved;      /* SWB_F_SHAPE: bit i = shape table index i is a candidate       */
  double lo, hi, lo32, hi32;
  double cand[SWB_MAX_CANDIDATES], cand32[SWB_MAX_CANDIDATES], cdf[SWB_MAX_CANDIDATES];
  double cos_a[SWB_MAX_CANDIDATES], sin_a[SWB_MAX_CANDIDATES];
} swb_tree_leaf;
/* Predicates: nodes [first, first + n) evaluated left to right on a stack of bits.  LEAF pushes the test of leaf `leaf`, TRUE
 * pushes 1 (an empty Product); AND / OR / ANDNOT pop b, then a, and push a & b / a | b / a & ~b.  The program leaves one bit. */
enum swb_pred_op { SWB_PRED_LEAF = 0, SWB_PRED_AND = 1, SWB_PRED_OR = 2, SWB_PRED_ANDNOT = 3, SWB_PRED_TRUE = 4 };
typedef struct swb_pred_node { int16_t op, leaf; } swb_pred_node;
typedef struct swb_tree_pred { int16_t first, n; } swb_tree_pred;
/* Sampling programs.  DRAW a: draw leaf a into its factor.  CHOOSE a (Mixture): one uniform() u against choices[a].cdf, jump to
 * its target[#{i : cdf[i] <= u}].  JUMP a: forward only.  TEST a, b, c closes a rejection loop: predicate a is evaluated on the
 * factors as drawn so far; when its value equals b the program goes on, else it jumps BACK to c (Intersection: b = 1 over all
 * components; SetMinus: b = 0 over hold_out; Selection: b = 1 over filtering) -- an outer loop restarts its inner loops.
 * Every failed TEST of one sprite counts against ONE budget, swb_tree_sampler::max_tries: when it is used up the last draw is
 * kept, every later TEST of the sprite passes, and the sprite is counted in swb_sampler_exhausted (the reference raises
 * ValueError after _MAX_TRIES per loop).  The budget bounds the work of a sprite at max_tries x program length. */
enum swb_tree_op_kind { SWB_OP_DRAW = 0, SWB_OP_CHOOSE = 1, SWB_OP_JUMP = 2, SWB_OP_TEST = 3 };
typedef struct swb_tree_op { int16_t kind, a, b, c; } swb_tree_op;
typedef struct swb_tree_choice {
  int32_t n, reserved;
  int32_t target[SWB_MAX_CANDIDATES];  /* op index (absolute), inside the group's program */
  double cdf[SWB_MAX_CANDIDATES];
} swb_tree_choice;
typedef struct swb_tree_group {
  int32_t count_min, count_max;
  int32_t first_op, n_ops;             /* the group's program: ops[first_op .. first_op + n_ops), ends by running off its end */
  /* factors the tree does not mention: the Sprite defaults (Python numbers; `shape` as its table index) */
  double defaults[SWB_TREE_N_FACTORS];
  double default_cos, default_sin;     /* math.cos / sin(math.radians(defaults[SWB_F_ANGLE])) */
} swb_tree_group;
/* Labels of (sub-)task t from its predicates: FIND_GOAL: pred[0] (n_preds = 0: no filter, label 1); CLUSTERING: the index of
 * the first predicate that holds, else -1; NO_REWARD: 0.  For a task of the handle with n_xcuts + n_ycuts > 0 the same is
 * evaluated once per cell of its grid with x / y replaced by the cell's representative (-inf below the first cut, else the
 * cut, as an np.float32) into swb_pool::cell_label. */
typedef struct swb_tree_task {
  int32_t kind;                        /* swb_task_kind */
  int32_t n_preds;
  int16_t pred[SWB_TREE_MAX_CLUSTERS];
} swb_tree_task;
typedef struct swb_tree_sampler {
  int32_t n_groups, shuffle, color_map, n_alternatives;       /* as swb_sampler */
  int32_t alternatives_weighted;       /* 1: one uniform() against alternative_cdf; 0: u32 % n_alternatives */
  int32_t max_tries;                   /* failed TESTs per sprite (>= 1; SWB_TREE_DEFAULT_MAX_TRIES) */
  int32_t n_leaves, n_pred_nodes, n_preds, n_ops, n_choices, n_tasks;   /* n_tasks must equal the handle's */
  swb_alternative alternatives[SWB_MAX_ALTERNATIVES];
  double alternative_cdf[SWB_MAX_ALTERNATIVES];
  double deg_cos[360], deg_sin[360];
  swb_tree_group groups[SWB_MAX_GROUPS];
  swb_tree_task tasks[SWB_MAX_TASKS];
  swb_tree_choice choices[SWB_TREE_MAX_CHOICES];
  swb_tree_pred preds[SWB_TREE_MAX_PREDS];
  swb_pred_node pred_nodes[SWB_TREE_MAX_PRED_NODES];
  swb_tree_op ops[SWB_TREE_MAX_OPS];
  swb_tree_leaf leaves[SWB_TREE_MAX_LEAVES];
} swb_tree_sampler;

/* Per-step outputs, device memory, caller-owned.  Any pointer may be NULL. */
typedef struct swb_outputs {
  uint8_t* obs;        /* u8 [N, H, W, 3]  PILRenderer.render (pil_renderer.py:67-91)      */
  double* reward;      /* f64[N]  NaN on FIRST steps (dm_env reward=None)                  */
  float* discount;     /* f32[N]  NaN on FIRST, 1 on MID, 0 on LAST                        */
  uint8_t* step_type;  /* u8 [N]  swb_step_type                                            */
  uint8_t* success;    /* u8 [N]  task.success(sprites) (renderers Success, handcrafted.py:115-131) */
  uint8_t* error;      /* u8 [N]  swb_env_error bits                                       */
} swb_outputs;

/* Live state snapshot (host memory, caller-allocated) for parity tests and
 * checkpointing (Environment.state(), environment.py:128-134). */
typedef struct swb_state {
  double* x;            /* [N,S] */
  double* y;            /* [N,S] */
  int32_t* n_sprites;   /* [N]   */
  int32_t* pool_entry;  /* [N]   current episode's pool entry */
  int32_t* step_count;  /* [N]   */
  uint8_t* reset_next;  /* [N]   */
  int32_t* episode;     /* [N]   number of resets so far */
} swb_state;

typedef struct swb_engine* swb_handle;

const char* swb_last_error(void);
int swb_version(void);

/* Lifecycle. `device` is the HIP device ordinal. */
int swb_create(const swb_config* cfg, int device, swb_handle* out);
int swb_destroy(swb_handle h);

/* constants.SHAPES (constants.py:27-40): vertices f64 [total,2], offsets[n_shapes+1]. */
int swb_upload_shapes(swb_handle h, const double* verts, const int32_t* offsets, int32_t n_shapes);

/* PIL ImagingResample 8bpc coefficient tables for one axis (host-computed, see
 * spriteworld_amd/lanczos.py): bounds i32[out,2] (xmin,len), coeffs i32[out,ksize].  A large-frame handle keeps the
 * tables as they are, with per-output prefix sums of the horizontal coefficients.
 * Accepted: the tables of any Pillow 8bpc filter (BOX, BILINEAR, HAMMING, BICUBIC, LANCZOS) and source box -- Pillow holds
 * the box as float[4]: compute the tables from float32 box coordinates -- with windows inside the canvas, len <= ksize, and,
 * on the tuned path, vertical windows of at least one pixel whose first and last rows never decrease from one output row to
 * the next, at most 8 output rows in flight at any canvas row (rows whose window is open, counted from the oldest that is
 * not complete; up to 6 run swb_resample_kernel<6>, 7 and 8 swb_resample_kernel<8>), and a horizontal prefix table -- len + 1
 * running sums per DISTINCT vector of them -- under 32 KB.  Large-frame handles take any number of rows in flight.
 * Everything else is refused with SWB_ERR_INVALID and a message (out_size other than the image's, axis, "bad horizontal /
 * vertical bounds", "vertical windows are not monotone", "more than 8 output rows in flight", "horizontal prefix table too
 * large"), and a refused upload leaves the handle's tables as they were.  An upload onto a live handle -- of the tables it
 * already holds, too -- makes the kept run lists and the cached frames stale: the next launch lists and resamples every
 * environment.  (tests/_resample_tables_cases.py uploads every such family.) */
int swb_upload_resample(swb_handle h, int32_t axis /*0=horizontal,1=vertical*/, int32_t out_size,
                        int32_t ksize, const int32_t* bounds, const int32_t* coeffs);

/* Install the reset pool and mark every environment "reset on next step"
 * (Environment.__init__, environment.py:68-70). */
int swb_set_pool(swb_handle h, const swb_pool* pool);

/* Fills a pool of `n_entries` episodes on the device from `spec` (no host sampling, no upload) and
 * marks every environment "reset on next step", like swb_set_pool.  pool_base/pool_len: i32[N].
 * Entry e draws from the Philox stream (seed, first_entry + e): shards of one job pass their global
 * offset and get the episodes a single process would have drawn for the same entries. */
int swb_sample_pool(swb_handle h, const swb_sampler* spec, int32_t n_entries, const int32_t* pool_base_host,
                    const int32_t* pool_len_host, uint64_t seed, uint64_t first_entry, void* stream);

/* Redraws the pool with the spec and layout of the last swb_sample_pool and a new seed, WITHOUT
 * resetting anything: entries an environment is currently playing are left untouched, so a long
 * run calls this every few episodes and never sees an episode twice.  Asynchronous on `stream`
 * (the same stream as swb_step, or ordered with it). */
int swb_resample_pool(swb_handle h, uint64_t seed, uint64_t first_entry, void* stream);

/* swb_sample_pool for a swb_tree_sampler (swb_sample_tree_kernel: one thread per entry, the same Philox streams): the same
 * contract, and handles with a task that keys on position are accepted -- swb_pool::cell_label is filled on the device.
 * swb_resample_pool afterwards redraws with the tree kernel (with whichever sampler filled the pool last).
 * The whole program is validated on the host before anything is launched (SWB_ERR_INVALID): every index in range; jumps and
 * choice targets inside the group's program; backward jumps only from TEST, forward ones only from JUMP / CHOOSE; predicate
 * stacks at most SWB_TREE_MAX_STACK deep and left with one bit; x and y drawn, and only by UNIFORM_F32 leaves; angle DISCRETE or
 * integer degrees within [0, 360]; no UNIFORM_INT colour channel under the hsv colour map; cdfs non-decreasing. */
int swb_sample_pool_tree(swb_handle h, const swb_tree_sampler* spec, int32_t n_entries, const int32_t* pool_base_host,
                         const int32_t* pool_len_host, uint64_t seed, uint64_t first_entry, void* stream);

/* Sprites of the last swb_sample_pool_tree / swb_resample_pool whose retry budget (swb_tree_sampler::max_tries) ran out: the
 * reference would have raised ValueError.  Each (re)sample call clears the counter first.  Synchronous (synchronises `stream`);
 * 0 on a handle that never sampled a tree. */
int swb_sampler_exhausted(swb_handle h, int64_t* sprites, void* stream);

/* Copies the device pool into caller-allocated HOST arrays laid out like swb_set_pool's input
 * (pool->n_entries must equal the device pool's; angle/color may be NULL; cell_label, when given, is copied on handles with a
 * task that keys on position).  Synchronous. */
int swb_get_pool(swb_handle h, const swb_pool* pool_host);

/* Environment.reset() for all envs: the next swb_step is a FIRST step. */
int swb_reset_all(swb_handle h, void* stream);

/* Environment.step(): actions_dev is f64[N,4] (f32[N,4] when cfg.action_is_f32) for
 * SelectMove/DragAndDrop, or i32[N,2] for Embodied. */
int swb_step(swb_handle h, const void* actions_dev, const swb_outputs* out, void* stream);

/* swb_step for a subset of the batch: active_dev is u8[N] in device memory, NULL means every environment (swb_step is exactly
 * that call).  An environment n with active_dev[n] == 0 takes no part in the step:
 *   - none of its state changes (positions, sprite count, pool entry, step count, episode, setter overrides), a pending reset
 *     STAYS pending -- it is not reset, and does not start an episode it was not asked to --, and no task is evaluated;
 *   - row n of actions_dev is never read (it may hold NaN or integers out of range);
 *   - entry n of out->reward, discount, step_type, success and error is not written: the caller's buffers keep what the
 *     environment's last active step left there (a held reward must not be summed twice);
 *   - out->obs[n] IS written, with the frame of the environment's state as it is -- byte for byte what swb_render gives.  On the
 *     two-kernel path the environment's cover wave keeps its run lists and its frame is copied from the frame cache like that of
 *     any environment whose sprites did not move -- by the copy workgroups of the cover launch, which know nothing of the mask
 *     (swb_list_stats counts it as kept, swb_frame_stats as filled, then copied);
 *     painting builds, large frames and many-sprite handles draw the unchanged state again.
 * One case is unspecified: the frame of an environment that has had no FIRST step since its pool was installed (swb_set_pool,
 * swb_sample_pool, swb_copy_pool) and is inactive -- it has no sprites of its own yet.
 * Everything else is swb_step's: the same kernels and launches, a counted step of swb_timing_enable, the same dispatch
 * bookkeeping.  The mask is read by the launch: keep it alive and unchanged until the launch has run. */
int swb_step_masked(swb_handle h, const void* actions_dev, const uint8_t* active_dev, const swb_outputs* out, void* stream);

/* Environment.reset() for the environments n with mask_dev[n] != 0 (u8[N] in device memory; NULL is refused with
 * SWB_ERR_INVALID): the next step in which such an environment is ACTIVE is a FIRST step from pool entry pool_base + episode %
 * pool_len, exactly as after a LAST.  One small kernel (swb_reset_envs_kernel), asynchronous on `stream`; nothing else is
 * touched.  Unlike swb_reset_all it leaves the kept run lists and cached frames of the other environments valid. */
int swb_reset_envs(swb_handle h, const uint8_t* mask_dev, void* stream);

/* observation() only (no state change): obs_dev u8[N,H,W,3].  Reports no swb_env_error flags: a sprite beyond the render path's
 * coordinate limit (SWB_ENV_ERR_SPAN_OVERFLOW) leaves its environment's frame unspecified without a sign; the next swb_step
 * that renders raises the flag. */
int swb_render(swb_handle h, uint8_t* obs_dev, void* stream);

/* Environment.success() (/root/reference/spriteworld/environment.py:80-81: `task.success(self._sprites)` of the sprites AS
 * THEY ARE -- after sprite setters or swb_set_positions, not as the last step left them): success_dev u8[N].  Evaluates the
 * task (tasks.py:153-158, :239-245, :289-296) in the cover kernel's state phase; no state change, no time step, no frame. */
int swb_evaluate(swb_handle h, uint8_t* success_dev, void* stream);

/* Rollouts: from where every environment is NOW, what would M candidate action sequences of K steps earn?
 * actions_dev is [K, N, M, 4] f64 (f32 when cfg.action_is_f32) for SelectMove / DragAndDrop, or [K, N, M, 2] i32 for Embodied.
 * For environment n and candidate m, out->*[k, n, m] holds exactly what swb_step number k + 1 would have written for
 * environment n had the next K steps been taken with actions[k, n, m]: the same bits of reward (NaN on FIRST), discount, step
 * type and success, and the same auto-reset -- a candidate that reaches LAST plays FIRST on the next step, from pool entry
 * pool_base + (episode mod pool_len), as the live environment would (it is not stopped at its first LAST).
 * The handle is left as it was: positions, step counts, episodes, entries, reset flags, the pool, and the run lists and
 * dispatch bookkeeping of the render path; nothing is rendered (swb_rollout_frames below draws the end states,
 * swb_rollout_trajectory and swb_rollout_step_frames the states after every step).
 * N * M virtual environments step on a scratch copy of the state (N * M * (16 * max_sprites + 32) bytes, owned by the handle, grown on demand); two kernels, asynchronous on `stream`
 * -- only growing the scratch (or, when K grows, the K per-step parameter blocks of 2 KB kept beside it) blocks.
 * Limits: M, K >= 1, N * M <= 2^24, K <= 65536; SWB_ERR_INVALID beyond them.
 * The scratch belongs to the handle: ONE stream at a time per handle.  A rollout must not be issued on another stream while an
 * earlier rollout of the same handle may still run (order the streams with an event first); calls on one stream need nothing.
 * SWB_ERR_STATE on a handle on which swb_set_sprite_attr has been called (the override buffers exist): the state phase indexes
 * overrides by environment, and replicating the 1 KiB centred paths per candidate is out of scope. */
typedef struct swb_rollout_outputs {   /* device memory, caller-owned; any pointer may be NULL */
  double* reward;      /* f64[K,N,M]  as swb_outputs::reward                                          */
  float* discount;     /* f32[K,N,M]                                                                   */
  uint8_t* step_type;  /* u8 [K,N,M]                                                                   */
  uint8_t* success;    /* u8 [K,N,M]                                                                   */
  uint8_t* error;      /* u8 [N,M]    swb_env_error bits of the K steps, ORed INTO the buffer (sticky) */
  double* x;           /* f64[N,M,S]  positions after step K                                           */
  double* y;           /* f64[N,M,S]                                                                   */
  int32_t* n_sprites;  /* i32[N,M]    sprites of the episode the candidate ends in                     */
} swb_rollout_outputs;
int swb_rollout(swb_handle h, const void* actions_dev, int32_t M, int32_t K, const swb_rollout_outputs* out, void* stream);

/* Frames of a rollout: what the agent would SEE after step K of every candidate.  Renders the states the LAST swb_rollout of
 * this handle left in its scratch; asynchronous on `stream`, which must be that rollout's stream or ordered with it (the
 * scratch belongs to the handle).
 *   cand_dev == NULL   obs_dev is u8[N, M, H, W, 3]: frame [n, m] is, to the byte, what swb_step number K would have written to
 *                      swb_outputs::obs for environment n had the K steps been taken with actions[:, n, m].  A candidate whose
 *                      step K was LAST shows its terminal sprites (as swb_render does of a live environment about to reset), one
 *                      whose step K was FIRST the fresh episode.  error_dev: u8[N, M].
 *   cand_dev i32[N]    (device) obs_dev is u8[N, H, W, 3]: the frame of candidate cand[n] of environment n only -- a planner's
 *                      argmax, for the cost of one step's rendering.  A value outside [0, M) is CLAMPED into it (negative: 0,
 *                      M and above: M - 1).  error_dev: u8[N].  One gather kernel (swb_rollout_pick_kernel) into a staging block
 *                      of N environments owned by the handle, then one render launch; only growing that block blocks.
 * error_dev may be NULL; else the swb_env_error bits of the render phases (SWB_ENV_ERR_SPAN_OVERFLOW) are ORed INTO it (sticky).
 * M must equal the M of that rollout: it guards the size of the caller's buffers.
 * How: the render path of the handle (tuned two-kernel, painting cover kernel, fill kernel, large frames, many sprites) with
 * its state pointers moved to the scratch, in M chunks of N consecutive virtual environments v = n * M + m -- each chunk one
 * launch like swb_render's: N is what the run lists, dispatch tables and overflow slots are sized for.  No kernel differs.
 * Untouched: the live state, the pool, the caller's step outputs and sticky error buffer, any frame buffer but obs_dev.  The
 * render path's dispatch bookkeeping (parity, phase, cost lists, which launch listed runs) advances as for swb_render --
 * results never depend on it --, so swb_trim_run_lists called straight afterwards sizes the lists from candidate scenes: a
 * list that outgrows its part moves to the arena, an exhausted arena is flagged in error_dev.  Never a counted step of
 * swb_timing_enable.  The scratch holds the end states only: frames of the steps k < K are swb_rollout_step_frames', after a
 * swb_rollout_trajectory.
 * SWB_ERR_INVALID: null handle, obs_dev NULL, M different from the last rollout's.  SWB_ERR_STATE: no rollout has run on the
 * handle; swb_set_pool, swb_sample_pool or swb_resample_pool was called since (a candidate may sit in an entry that was just
 * redrawn: roll out again); swb_set_sprite_attr has been called on the handle (overrides are indexed by live environment, as
 * for swb_rollout); shapes, pool or resampling tables missing. */
int swb_rollout_frames(swb_handle h, int32_t M, const int32_t* cand_dev, uint8_t* obs_dev, uint8_t* error_dev, void* stream);

/* A rollout that keeps every step: swb_rollout in every respect -- arguments, outputs, limits, refusals, the one-stream rule,
 * what it leaves untouched, and the end states in the scratch (swb_rollout_frames works after it unchanged) -- that also keeps
 * the state of every virtual environment after each of the K steps, for swb_rollout_step_frames below and for `steps`:
 * per environment n, candidate m and step k the positions and the sprite count after step k + 1, the per-step targets of a
 * state-space model (steps may be NULL, and so may any pointer in it).  What swb_rollout's x, y, n_sprites are for step K.
 * The K states live in a trajectory block owned by the handle, K * N * M * (16 * max_sprites + 24) bytes, laid out like the
 * scratch with [K][N * M] in front of every array (positions, sprite count, pool entry, step count, episode, reset flag;
 * pool_base / pool_len do not change during a rollout and stay in the scratch); grown on demand behind a stream synchronise,
 * like the scratch.  One kernel differs from swb_rollout's: the build of the rollout kernel that copies the state out after
 * every step.
 * SWB_ERR_INVALID besides swb_rollout's: K * N * M * max_sprites does not fit an int.  SWB_ERR_HIP with the byte count in the
 * message when the block cannot be allocated: the handle stays usable, and holds no rollout (swb_rollout_frames refuses).
 * A plain swb_rollout afterwards keeps no steps: it invalidates the trajectory. */
typedef struct swb_rollout_step_outputs {   /* device memory, caller-owned; any pointer may be NULL */
  double* x;           /* f64[K,N,M,S]  positions after step k + 1                                     */
  double* y;           /* f64[K,N,M,S]                                                                 */
  int32_t* n_sprites;  /* i32[K,N,M]    sprites of the episode the candidate is in after step k + 1    */
} swb_rollout_step_outputs;
int swb_rollout_trajectory(swb_handle h, const void* actions_dev, int32_t M, int32_t K, const swb_rollout_outputs* out,
                           const swb_rollout_step_outputs* steps, void* stream);

/* Frames of the steps inside a rollout: what the agent would SEE after step `step` + 1 of the candidates of the last
 * swb_rollout_trajectory of this handle.  swb_rollout_frames in every respect but where the states come from (the trajectory
 * block) -- the stream, error_dev ORed into, the clamping of cand, M as a guard, the render path re-pointed in chunks of N, what
 * is untouched, the dispatch bookkeeping advancing per chunk, never a counted step of swb_timing_enable.
 *   step in [0, K), cand_dev == NULL   obs_dev u8[N, M, H, W, 3], error_dev u8[N, M]: every candidate after step `step` + 1
 *   step in [0, K), cand_dev i32[N]    obs_dev u8[N, H, W, 3],    error_dev u8[N]:    candidate cand[n] after step `step` + 1
 *   SWB_ALL_STEPS,  cand_dev i32[N]    obs_dev u8[K, N, H, W, 3], error_dev u8[K, N]: candidate cand[n] after every step -- the
 *                                      K frames of the plan an agent has chosen: one gather kernel
 *                                      (swb_rollout_pick_steps_kernel) into the staging block, K render launches
 * Each frame is, to the byte, what swb_step number `step` + 1 would have written to swb_outputs::obs under that candidate: a
 * step that was LAST shows the terminal sprites, one that was FIRST the fresh episode.  step = K - 1 is swb_rollout_frames.
 * SWB_ERR_INVALID: null handle, obs_dev NULL, M different from the last rollout's, step outside [-1, K), SWB_ALL_STEPS with
 * cand_dev NULL (loop over the steps for that).  SWB_ERR_STATE: no rollout has run on the handle; the last one was a plain
 * swb_rollout, which kept no steps; the pool has changed since; swb_set_sprite_attr has been called on the handle; shapes,
 * pool or resampling tables missing. */
#define SWB_ALL_STEPS (-1)
int swb_rollout_step_frames(swb_handle h, int32_t M, int32_t step, const int32_t* cand_dev, uint8_t* obs_dev, uint8_t* error_dev,
                            void* stream);

/* Random-agent actions drawn on the device: one action per environment, ready for swb_step, without a host round trip.
 * SWB_SAMPLE_UNIFORM is action_space.sample() (uniform in [0, 1)^4; Embodied: carry in {0, 1}, direction in {0 .. 3}).
 * SWB_SAMPLE_ON_SPRITE is the batched Environment.sample_contained_position() (environment.py:110-126, sprite.py:117-126): a
 * sprite of the environment drawn uniformly by index, then a point of its bounding box redrawn until the sprite contains it
 * (sprite.py:113-115 on the centred path, setter overrides included); SelectMove / DragAndDrop actions click there.
 * One kernel, one wave per environment, asynchronous on `stream`.  The handle is only READ -- the sprites as they are now, what
 * swb_render would draw; an environment about to reset keeps its terminal sprites (its next action is ignored anyway) -- and
 * nothing of it is written: live state, the outputs of the last step, error flags, pool, run lists, dispatch bookkeeping.
 * Random numbers: Philox4x32-10, key = seed, counter = (entry lo, block, entry hi, 0) with entry = first_env + environment --
 * the streams of swb_sample_pool.  Draw order per environment (tests/_random_agent_model.py restates it, bit for bit):
 *   UNIFORM    SelectMove / DragAndDrop: a[0..3] = uniform (two u32 each).  Embodied: a[0] = u32 % 2, a[1] = u32 % 4.
 *   ON_SPRITE  n sprites.  n == 0: sprite = -1, tries = 0, position = (uniform, uniform).  Else s = u32 % n; low / high = the
 *              exact min / max over the vertices of its centred path; per try ux, uy = uniform, d = low + (high - low) * u,
 *              sample = position of s + d, accepted when the path contains sample - position of s (float64 throughout; a
 *              float32 position enters as its float64 value).  Then SelectMove / DragAndDrop: a[0], a[1] = sample, a[2], a[3] =
 *              uniform; Embodied: the two integer draws of UNIFORM (the contained position goes to `position` only).
 * Float32-action handles store (float) of the float64 values: containment is guaranteed for FLOAT64 actions (and `position`)
 * only -- a click rounded to float32 may leave the sprite at its edge.
 * DEVIATION from the reference: it gives up after 10^6 tries and raises; the kernel gives up after SWB_CONTAINED_MAX_TRIES
 * tries, then writes tries = -1 and the sprite's own position.  The worst acceptance rate of a shipped shape over all rotations
 * is 0.3536 (star_4: area over bounding box), so 1024 consecutive misses have probability below 1e-190; the cap bounds the time
 * a degenerate sprite (a zero scale through a setter) can take.
 * SWB_ERR_INVALID: unknown mode; every output NULL; position / sprite / tries given with SWB_SAMPLE_UNIFORM. */
#define SWB_CONTAINED_MAX_TRIES 1024
enum swb_action_sampling { SWB_SAMPLE_UNIFORM = 0, SWB_SAMPLE_ON_SPRITE = 1 };
typedef struct swb_sampled_actions {   /* device memory, caller-owned */
  void* actions;      /* [N][4] f64 or f32 (the handle's action dtype), or [N][2] i32 (Embodied); may be NULL            */
  double* position;   /* [N][2] the contained position, always f64; ON_SPRITE only, may be NULL                           */
  int32_t* sprite;    /* [N] index of the chosen sprite, -1 if the environment has none; ON_SPRITE only, may be NULL      */
  int32_t* tries;     /* [N] draws used (>= 1); 0: no sprite; -1: cap reached; ON_SPRITE only, may be NULL                */
} swb_sampled_actions;
int swb_sample_actions(swb_handle h, int32_t mode, uint64_t seed, uint64_t first_env, const swb_sampled_actions* out, void* stream);

/* A rollout that draws its own candidates: swb_rollout (keep_steps == 0) or swb_rollout_trajectory (keep_steps != 0) in every
 * respect -- outputs, limits, refusals, the one-stream rule, the scratch and the trajectory block, what is left untouched, and
 * the handle "holding a rollout" afterwards (swb_rollout_frames works; with keep_steps swb_rollout_step_frames too; the
 * stale-pool refusals apply) -- except that the K * N * M actions are not the caller's: the rollout kernel draws the action of
 * step k of candidate m from the state that candidate has REACHED, and hands it back in sampled->actions, in swb_rollout's own
 * layout: feeding that buffer to swb_rollout (swb_rollout_trajectory) reproduces every output bit for bit, and
 * actions[0, n, m] is what to give swb_step to execute the first step of the chosen plan.
 * mode (enum swb_action_sampling) is swb_sample_actions' per step: SWB_SAMPLE_UNIFORM, or SWB_SAMPLE_ON_SPRITE -- a click
 * inside a sprite drawn by index among those the candidate's step acts on, where they are at that step (inside a rollout the
 * sprites move per candidate: no sequence of swb_sample_actions and swb_rollout calls can place such a click).
 * Random numbers: Philox4x32-10, key = seed, counter = (entry lo, block, entry hi, 1 + m) with entry = first_env + n: ONE stream
 * per virtual environment for the whole rollout, consumed step by step, k = 0 .. K - 1.  The fourth counter word is 0 in
 * swb_sample_pool and swb_sample_actions, so no candidate replays those streams under the same seed, and a candidate's stream
 * depends neither on M nor on K: the first K' steps of the first M' candidates of a larger call are the smaller call's.
 * Per step the draw order is swb_sample_actions' for the mode, taken after the step's state is loaded: on a FIRST step from the
 * fresh episode's sprites -- the draw is made although the dynamics ignore a FIRST step's action, so the stream's position never
 * depends on step types.  A float32-action handle stores (float) of the float64 draw and steps with that float; containment is
 * guaranteed for FLOAT64 actions only.  The cap of SWB_CONTAINED_MAX_TRIES holds as documented above.  A SelectMove
 * noise_scale is the caller's, as for swb_rollout: none is applied.
 * Two kernels, asynchronous on `stream`: the fork kernel of swb_rollout and the builds of the rollout kernel that draw
 * (swb_rollout_kernel<KEEP, SAMPLE>: the same step code, a register budget of its own).
 * SWB_ERR_INVALID besides swb_rollout's / swb_rollout_trajectory's: unknown mode; sampled or sampled->actions NULL; sprite / tries
 * given with SWB_SAMPLE_UNIFORM; steps given with keep_steps == 0.  SWB_ERR_STATE after swb_set_sprite_attr, as for swb_rollout. */
typedef struct swb_rollout_sampled_outputs {  /* device memory, caller-owned */
  void*    actions;  /* REQUIRED. [K,N,M,4] f64 (f32 when cfg.action_is_f32) or [K,N,M,2] i32 (Embodied): what was drawn, in
                        swb_rollout's own layout -- feeding it to swb_rollout reproduces every output bit for bit            */
  int32_t* sprite;   /* [K,N,M] ON_SPRITE only, may be NULL: index of the chosen sprite, -1 if the environment had none      */
  int32_t* tries;    /* [K,N,M] ON_SPRITE only, may be NULL: as swb_sampled_actions::tries (>= 1; 0 no sprite; -1 cap)        */
} swb_rollout_sampled_outputs;
int swb_rollout_sampled(swb_handle h, int32_t mode /* enum swb_action_sampling */, uint64_t seed, uint64_t first_env,
                        int32_t M, int32_t K, int32_t keep_steps, const swb_rollout_outputs* out,
                        const swb_rollout_step_outputs* steps, const swb_rollout_sampled_outputs* sampled, void* stream);

/* A rollout that draws its candidates from a PLAN: swb_rollout_sampled in every respect -- outputs, limits, refusals, the
 * one-stream rule, the scratch and the trajectory block, the handle "holding a rollout" afterwards, sampled->actions required,
 * in swb_rollout's layout and reproducing every output bit for bit when replayed through swb_rollout (swb_rollout_trajectory),
 * (float) stored on a float32-action handle, SWB_ERR_STATE after a setter -- except that step k of every candidate of
 * environment n is drawn from the caller's distribution of (k, n): a categorical over sprite indices, a uniform point inside the
 * chosen sprite WHERE THAT CANDIDATE HAS IT at that step, and a bell-shaped motion around a mean.  It is what an iterative
 * planner (CEM, MPPI) refits between its rounds: a click distribution that survives a refit has to name the sprite, not the
 * place, because every candidate has moved its sprites somewhere else.
 * Random numbers: swb_rollout_sampled's streams -- Philox4x32-10, key = seed, counter = (entry lo, block, entry hi, 1 + m), entry
 * = first_env + n, one stream per virtual environment consumed step by step, independent of M and K.  Per step the position in
 * the stream depends on the rejected tries only, as in SWB_SAMPLE_ON_SPRITE: never on step types (a FIRST step draws from the
 * fresh episode's sprites), on choice_cdf being NULL, or on a fallback.
 * Draw order per step, SelectMove / DragAndDrop, on the n sprites the step acts on (float64, one rounding per operation;
 * tests/_rollout_guided_model.py restates it bit for bit):
 *   1. u_c = uniform -- always drawn.
 *   2. n == 0: sprite = -1, tries = 0, click = (uniform, uniform).
 *   3. else W' = min(n, width), total = cdf[k, n, W' - 1].  choice_cdf NULL, or total not both finite and > 0:
 *      s = min((int)(u_c * n), n - 1).  Else t = u_c * total and s = the first j < W' with cdf[j] > t; if there is none (t
 *      rounded up to total), the first j with cdf[j] >= total.  A sprite of weight 0 is therefore never chosen while total > 0,
 *      and sprites at index >= width have weight 0.
 *   4. the click: SWB_SAMPLE_ON_SPRITE's tries for sprite s, unchanged (bounding box of the centred path, the containment test,
 *      the cap SWB_CONTAINED_MAX_TRIES with tries = -1 and the sprite's own position).
 *   5. motion, c = 0, 1: z = (((u1 + u2) + (u3 + u4)) - 2.0) * 1.7320508075688772 from four uniforms; v = mean[c] + std[c] * z;
 *      a[2 + c] = v > 0 ? (v < 1 ? v : 1) : 0 -- a NaN gives 0: always in [0, 1].
 *   Embodied: u_c = uniform, idx by rule 3 over exactly 8 weights (fallback (int)(u_c * 8)); carry = idx / 4, direction =
 *   idx % 4; no click, no motion draws.
 * DEVIATION from "Gaussian": z is Irwin-Hall with n = 4 (a sum of four uniforms, centred and scaled): mean 0, variance exactly 1,
 * support +-2 sqrt(3) = +-3.46, kurtosis 2.7.  Every operation of it is an IEEE add or multiply, so a numpy model reproduces
 * the draws bit for bit, which is how this library pins its samplers; Box-Muller's log and cos would not be.
 * The weights are NOT validated (that would synchronise): the rules above make every value safe -- negative, NaN or infinite
 * entries change which sprite is chosen, never what memory is read; nothing is indexed by a floating-point value beyond the
 * clamps stated.
 * sampled->sprite (may be NULL) receives s (Embodied: idx); sampled->tries is SWB_SAMPLE_ON_SPRITE's and must be NULL for Embodied.
 * Two kernels, asynchronous on `stream`: the fork kernel of swb_rollout and swb_rollout_guided_kernel<KEEP> (the rollout
 * kernel's step code, a drawer and a register budget of its own).
 * SWB_ERR_INVALID besides swb_rollout's / swb_rollout_trajectory's, each message naming swb_rollout_guided: plan NULL; width
 * outside its range; motion_mean / motion_std NULL on a click space, or given on Embodied; tries given on Embodied; sampled or
 * sampled->actions NULL; steps given with keep_steps == 0. */
typedef struct swb_rollout_plan {     /* device memory, caller-owned, only read */
  const double* choice_cdf;   /* f64[K,N,W] running sums of non-negative weights along W, or NULL (uniform choice)              */
  int32_t       width;        /* W: 1..max_sprites for SelectMove / DragAndDrop; exactly 8 for Embodied (index = carry*4 + direction) */
  const double* motion_mean;  /* f64[K,N,2]  SelectMove / DragAndDrop: REQUIRED; Embodied: must be NULL                          */
  const double* motion_std;   /* f64[K,N,2]  likewise                                                                           */
} swb_rollout_plan;
int swb_rollout_guided(swb_handle h, const swb_rollout_plan* plan, uint64_t seed, uint64_t first_env, int32_t M, int32_t K,
                       int32_t keep_steps, const swb_rollout_outputs* out, const swb_rollout_step_outputs* steps,
                       const swb_rollout_sampled_outputs* sampled, void* stream);

/* Memory of the hand-off lists (what the cover kernel hands the resample / fill kernel: swb_variant_info::run_list_bytes).
 * A handle starts with a list of max(4, max_sprites + 1) units of 8 bytes per canvas row for every environment and group of 64
 * output columns -- enough for ANY scene of convex sprites, about ten times what the usual scene needs (133 KB per environment
 * for 12 sprites at 128x128 with anti_aliasing 5).  This call, made once the handle has rendered a few typical steps, cuts every
 * list's own part down to 1.25 x the longest list of the last launch and adds a shared arena (half of the parts together) into
 * which a list that outgrows its part moves (a segment twice as large); a scene that finds the arena exhausted too is flagged
 * SWB_ENV_ERR_SPAN_OVERFLOW (never silent).  Results do not change.  Blocking (synchronises `stream`, reallocates); no-op when
 * called again.  swb_set_pool / swb_sample_pool restore the full reservation (the new pool may hold denser scenes).
 * run_cap_out (may be NULL): the units of a list's own part afterwards.  The Python engine calls it after its third
 * rendering step.  A large-frame handle (swb_variant_info::large_frames) has no run lists: a successful no-op, run_cap_out 0. */
int swb_trim_run_lists(swb_handle h, int32_t* run_cap_out, void* stream);

/* Kept hand-off lists.  A run list is a pure function of an environment's sprites and of the handle's geometry, and the lists
 * stay in device memory from launch to launch.  A cover wave whose environment was not reset by the launch and whose sprites
 * all stand, bit for bit, where they stood before it hands the second kernel the lists that are there already instead of
 * building them again; the second kernel still writes every frame of every environment at every rendering launch.  Every call
 * other than a step that changes what a list depends on, or where it lives, makes all lists stale (the pool calls,
 * swb_reset_all, swb_set_positions, the sprite setters, the table uploads, swb_trim_run_lists, frames of rollout states, a
 * step without an observation buffer).  Lists built with an error flag raised, or that moved to the arena, are never kept.
 * Two switches of the environment, read at swb_create:
 *   SWB_NO_KEEP_LISTS  every wave builds its lists (tests, A/B runs); results are identical either way
 *   SWB_LIST_STATS     the cover waves of rendering launches count themselves for swb_list_stats (one atomic per wave)
 * swb_list_stats: the cover waves since swb_create that kept / built their lists.  Blocking (synchronises `stream`);
 * SWB_ERR_STATE on a handle created without SWB_LIST_STATS.  Handles whose cover kernel paints the frame itself and
 * large-frame handles have no lists and count nothing. */
int swb_list_stats(swb_handle h, int64_t* kept, int64_t* built, void* stream);

/* Frame cache.  A frame is a pure function of the run lists, their header's colour words, the background and the resampling
 * tables.  A handle whose frames come from the resample kernel (anti_aliasing > 1, not the large-frame or many-sprite path, not
 * SWB_NO_KEEP_LISTS) owns one frame per environment of device memory (swb_variant_info::frame_cache_bytes: 12 KB per environment
 * at 64x64, 49 KB at 128x128).  The first launch that keeps an environment's lists leaves its frame there as well; every
 * further launch that keeps them copies the caller's frame from it instead of resampling the lists again.  The copies are made
 * in the COVER launch, speculatively: a rendering launch on the live state has one more workgroup per (environment, column
 * group), which copies the cached frame of every environment whose cache may hold it before it is known whether the environment
 * keeps its lists in this launch -- beside the waves that build lists, while the memory system is idle.  An environment that
 * keeps files no task for the resample kernel; one that builds, or keeps for the first time, has its frame overwritten in full
 * by the resample kernel, one launch boundary later.  (A handle without cost order -- SWB_NO_COST_ORDER -- copies in the
 * resample kernel as before.)  The caller's buffer
 * is written in full at every rendering launch either way and is never read back across launches: it may be another buffer at
 * every step, and the caller may do with it what it likes.  Whatever makes the lists stale (see above) makes the cache stale.
 * A handle that cannot get the memory runs without a cache.  Switches of the environment, read at swb_create:
 *   SWB_NO_FRAME_CACHE  no cache: every wave resamples (tests, A/B runs); results are identical either way
 *   SWB_SPEC_COPY       `behind` (the default): the copy workgroups stand behind the cover workgroups; `first` (tests): in
 *                       front of them, the order in which every copy workgroup sees the word of the previous launch.  Results
 *                       are identical either way; any other value is SWB_ERR_INVALID
 * swb_frame_stats: frames taken from the cache, counted as the tasks of the resample kernel that would have copied them -- one
 * per (environment, column group[, band]) and launch -- / tasks of the resample kernel that resampled and filled the cache /
 * only resampled, since swb_create.  Blocking; needs SWB_LIST_STATS like
 * swb_list_stats.  swb_frame_cycles (measurement): out3 = wave cycles of the copy workgroups that copied, of the resample
 * kernel's tasks, and the list bytes those walked.  swb_spec_copy_stats (measurement): the copy workgroups -- one per
 * (environment, column group) and launch -- that copied; those whose environment then built or filled are the wasted copies. */
int swb_frame_stats(swb_handle h, int64_t* copied, int64_t* filled, int64_t* resampled, void* stream);
int swb_frame_cycles(swb_handle h, int64_t* out3, void* stream);
int swb_spec_copy_stats(swb_handle h, int64_t* copy_groups, void* stream);

/* Task cache.  The task's reward, success and error bits are a pure function of the sprites' positions, the episode's labels,
 * the sprite count and the task configuration.  The handle owns one 16-byte record per environment
 * (swb_variant_info::task_cache_bytes), on every path (tuned, painting, large frames, many sprites; with or without an
 * observation buffer).  A step that is no reset of the environment and moves none of its sprites, bit for bit -- a missed
 * click, a zero motion, a move clipped back onto the same value -- takes the three from the record instead of evaluating the
 * task again; every other step evaluates and leaves the record.  The error bits come back at every such step as a fresh
 * evaluation would raise them (the caller may have cleared `error`).  Every call other than a step that may change what the
 * task reads makes all records stale (the pool calls, swb_copy_pool, swb_set_positions, the sprite setters, swb_load_state,
 * swb_upload_shapes); swb_reset_all / swb_reset_envs need not: a reset step evaluates.  swb_evaluate, swb_render, rollouts and
 * their frames neither read nor write a record.  A handle that cannot get the memory runs without a cache.  Switch of the
 * environment, read at swb_create:
 *   SWB_NO_TASK_CACHE  no cache: every step evaluates the task (tests, A/B runs); results are identical either way
 * swb_task_stats: the environment-steps since swb_create -- environments that took part in a swb_step / swb_step_masked -- that
 * reused the record / evaluated the task.  Blocking (synchronises `stream`); needs SWB_LIST_STATS at swb_create like
 * swb_list_stats (SWB_ERR_STATE otherwise); one atomic per stepping wave. */
int swb_task_stats(swb_handle h, int64_t* reused, int64_t* evaluated, void* stream);

/* Split bands.  A batch that the band rule leaves at one band per frame, but whose resample launch is at most two rounds of
 * resident waves, ends with its last resampling wave while most tasks only copy (frame cache).  Such a handle builds its lists
 * and tables for swb_variant_info::split_bands bands and decides at every launch, on the device, which environments use them:
 * one whose frame is copied files no task (the cover launch's copy workgroups copied its whole rows: one whole copy per column
 * group); one that resamples or fills files its band tasks when the previous
 * launch had at most SWB_SPLIT_WHEN frames that resampled or filled, else one whole task that walks the whole list.  Results
 * never depend on it.  swb_variant_info::n_bands keeps reporting the nominal 1.  Switches of the environment, read at swb_create:
 *   SWB_SPLIT_BANDS=n  0: never the mode; n >= 2: the mode with n bands at any batch size (tests, A/B runs)
 *   SWB_SPLIT_WHEN=k   the threshold in frames (default: two per SIMD of the device); 0 never splits, a huge value always does
 * Not by itself in the Embodied action space (the agent moves at nearly every step: nothing is kept, nothing copied; a proxy --
 * a batch of another action space whose sprites all move at every step takes the mode, never splits, and pays for the band starts).
 * Not under SWB_BANDS, SWB_NO_FRAME_CACHE, SWB_NO_KEEP_LISTS, SWB_NO_COST_ORDER, anti_aliasing = 1, the large-frame paths.
 * swb_frame_stats keeps counting frames -- (environment, column group) pairs -- on such a handle, not waves.
 * swb_split_stats: the tasks of the resample kernel since swb_create that were whole and resampled or filled / band tasks /
 * the whole copies of kept frames (one per column group, counted by the keeping wave).  Blocking; needs SWB_LIST_STATS; SWB_ERR_STATE on a handle that is not in the mode. */
int swb_split_stats(swb_handle h, int64_t* whole, int64_t* bands, int64_t* whole_copies, void* stream);

/* SpriteFactors observation (renderers/handcrafted.py:29-82): factors_dev f64[N,S,10] in
 * sprite.FACTOR_NAMES order (x, y, shape, angle, scale, c0, c1, c2, x_vel, y_vel), `shape` as its
 * constants.ShapeType value (1-based); rows >= n_sprites[env] are zero. */
int swb_factors(swb_handle h, double* factors_dev, void* stream);

/* Scalars of ONE environment (environment.py:74-108 keeps them as attributes): out5 = { sprites in the current
 * episode, pool entry it plays, step count, episodes started, 1 if the next step is a reset }.  Synchronises
 * `stream`; five 4-byte copies whatever the batch size (swb_get_state copies every environment). */
int swb_get_env_state(swb_handle h, int32_t env, int32_t* out5, void* stream);
/* swb_pool::attr_f32 of one sprite of the episode environment `env` is playing (bit 0: angle, bit 1: scale). */
int swb_get_sprite_types(swb_handle h, int32_t env, int32_t sprite, int32_t* flags, void* stream);

/* Blocking state access (synchronises `stream`). */
int swb_get_state(swb_handle h, const swb_state* host_state, void* stream);
int swb_set_positions(swb_handle h, const double* x_host, const double* y_host, void* stream);

/* Snapshots: the state of environments saved to, and loaded from, DEVICE memory of the caller's -- nine small arrays of C slots,
 * everything of an environment that a step changes plus the pool range it resets through.  What a closed-loop planner puts a
 * batch back with, what seeds a larger batch from a smaller one (swb_copy_pool below), what adopts the end state of a rollout
 * candidate without replaying it, and, copied to the host, a checkpoint.  Everything static (shapes, colours, labels, velocities)
 * stays in the pool and is found through pool_entry: a snapshot means something only beside the pool it was saved under.
 * Not in a snapshot: sprite overrides (swb_set_sprite_attr) -- all three calls below return SWB_ERR_STATE on a handle whose
 * override buffers exist, as the rollouts do --, the caller's output and error buffers, and anything the host keeps (random
 * generators, seeds).
 *
 * swb_pool_id: every call that installs or redraws a pool (swb_set_pool, swb_sample_pool, swb_sample_pool_tree,
 * swb_resample_pool) gives the handle a fresh id, unique in the process and never 0; swb_copy_pool hands on the source's.
 * *id is 0 on a handle without a pool.
 *
 * swb_save_state: slot c of `snap` takes the state of environment index_dev[c] (i32[C], device); index_dev == NULL: slot c takes
 * environment c, and C must be N.  source = SWB_STATE_ROLLOUT_END: the states the handle's last rollout ended in -- index
 * n * M + m is candidate m of environment n, NULL all N * M of them in that order (C must be N * M) --, refused with
 * SWB_ERR_STATE where swb_rollout_frames is (no rollout has run, the pool has changed since).  A slot whose index is outside the
 * source is left untouched.  One kernel, asynchronous on `stream`; the handle is only read.  pool_base / pool_len travel with
 * the state: an environment that is loaded with it auto-resets through the entries its source would have played.
 *
 * swb_load_state: environment n takes slot slot_dev[n] (i32[N], device); -1 leaves the environment exactly as it is; any other
 * value outside [0, C) leaves it alone too and adds one to *rejected_dev (a device word, may be NULL; the call never reads it).
 * slot_dev == NULL: environment n takes slot n, and C must be N.  pool_id: the id the snapshot was saved under, checked against
 * the handle's (SWB_ERR_STATE when they differ); 0 skips the check -- the caller vouches that the handle's pool holds, entry for
 * entry, what the snapshot's did (a run resumed from swb_get_pool + swb_set_pool after a restart).  One kernel, asynchronous on
 * `stream`, no synchronisation, no allocation.  From the next launch on a loaded environment behaves bit for bit as its source
 * would have.  The kept run lists and the cached frame of the loaded environments are dropped (per environment: the others keep
 * theirs); the caller's sticky error buffer, the outputs of the last step and a held rollout are not touched.  The pool ranges
 * of the environments may have moved: swb_resample_pool, which relies on pool_base[n] = n * pool_len, is refused afterwards
 * until a pool call lays the ranges out again.
 *
 * SWB_ERR_INVALID, with the function's name in the message: a null handle, a null snapshot or a null pointer in it, C < 1,
 * C * max_sprites beyond an int, an unknown source, NULL index / slot with C different from the source's size.  SWB_ERR_STATE:
 * no pool, override buffers, and the cases named above. */
typedef struct swb_snapshot {      /* DEVICE memory, caller-owned, C slots; every pointer required */
  double *x, *y;                   /* f64[C, S]  S = cfg.max_sprites of the handle that saves / loads */
  int32_t *n_sprites, *pool_entry, *step_count, *episode, *pool_base, *pool_len;   /* i32[C] */
  uint8_t *reset_next;             /* u8[C] */
} swb_snapshot;
enum swb_state_source { SWB_STATE_LIVE = 0, SWB_STATE_ROLLOUT_END = 1 };
int swb_pool_id(swb_handle h, uint64_t* id);
int swb_save_state(swb_handle h, int32_t source, const int32_t* index_dev, int32_t C, const swb_snapshot* snap, void* stream);
int swb_load_state(swb_handle h, const swb_snapshot* snap, int32_t C, const int32_t* slot_dev, uint64_t pool_id,
                   int32_t* rejected_dev, void* stream);

/* The device pool of `src` copied into `dst`, device to device on `stream`: every array swb_set_pool uploads, cell_label on
 * handles with a task that keys on position, and the angle / colour columns of the SpriteFactors observation.  dst takes
 * pool_base_host / pool_len_host (i32[N of dst], ranges inside src's pool) as its environments' ranges, takes over src's pool
 * id -- snapshots of src load into dst --, and is marked "reset on next step" like after swb_set_pool (swb_load_state then puts
 * states in); its run lists get their full reservation back and a rollout it holds becomes stale.  The copies are made into
 * fresh allocations that replace dst's only when all of them succeeded: a failure leaves dst's pool as it was.  Blocking
 * (synchronises the device before the old arrays are freed).
 * SWB_ERR_INVALID: a null argument, dst == src, handles that differ in device, max_sprites, n_tasks, position dtype or in whether
 * a task keys on position, a range outside the pool, a pool whose scenes the large-frame raster kernel of dst cannot hold.
 * Task sets (swb_set_task_sets): the set of every entry is copied with the pool; SWB_ERR_INVALID when the handles' tables differ.
 * SWB_ERR_STATE: src has no pool; override buffers exist on either handle.  dst cannot redraw the pool (the sampler's
 * specification stays with src): swb_resample_pool on it is refused until it is given a pool of its own. */
int swb_copy_pool(swb_handle dst, swb_handle src, const int32_t* pool_base_host, const int32_t* pool_len_host, void* stream);

/* Task sets: the task an episode is played under travels with its pool entry.  A task set is a
 * contiguous range of the sub-task table swb_config::tasks with the aggregation and the time limit of ONE reference task:
 * a plain task is one sub-task with is_meta = 0, a MetaAggregated its sub-tasks with is_meta = 1 (tasks.py:248-296).  Every
 * pool entry names one set (a byte per entry); a step looks the set of the environment's entry up and
 *   - evaluates the sub-tasks of that set only (tasks[first_task .. first_task + n_tasks), their labels at rows
 *     first_task .. of swb_pool::label / cell_label: the rows of other sets are never read),
 *   - aggregates them with the set's meta_aggregator, meta_termination and meta_terminate_bonus (is_meta = 1) or takes the one
 *     sub-task's reward and success as they are (is_meta = 0),
 *   - adds a float32 motion cost in float32 when the set's task returns a Python float (is_meta = 0 and not FIND_GOAL), and
 *   - ends the episode at the set's max_episode_length.
 * So an environment's consecutive episodes may be played under different tasks; resets, masked steps, snapshots, swb_copy_pool
 * and swb_evaluate need to know nothing of it: the set follows swb_state::pool_entry. */
#define SWB_MAX_TASK_SETS 8
typedef struct swb_task_set {
  int32_t first_task, n_tasks;      /* sub-tasks cfg.tasks[first_task .. first_task + n_tasks), n_tasks >= 1, inside [0, cfg.n_tasks); sets may overlap */
  int32_t is_meta, meta_aggregator, meta_termination;   /* as swb_config's */
  int32_t max_episode_length;
  double  meta_terminate_bonus;
} swb_task_set;

/* Installs the handle's table of 1 .. SWB_MAX_TASK_SETS task sets.  Once, after swb_create and before any pool is installed:
 * SWB_ERR_STATE on a handle that has a pool or a table already.  SWB_ERR_INVALID: a count outside [1, SWB_MAX_TASK_SETS], a
 * sub-task range outside cfg.tasks[0 .. cfg.n_tasks), an unknown aggregator or termination rule, max_episode_length < 0.
 * From then on cfg.n_tasks is only the stride T of the label arrays, and cfg.is_meta, cfg.meta_* and cfg.max_episode_length
 * are unused.  A handle that never calls this behaves exactly as before, and launches the same kernels.
 * A handle with task sets runs builds of the step kernels of its own (swb_cover_sets_kernel, swb_ms_state_sets_kernel: the
 * only ones that carry the lookup; they honour setter overrides too); table and entry bytes live in device memory owned by the
 * handle, not in the kernel arguments.  Rollouts are out of scope on such a handle: swb_rollout, swb_rollout_trajectory,
 * swb_rollout_sampled, swb_rollout_guided, swb_rollout_frames and swb_rollout_step_frames return SWB_ERR_STATE. */
int swb_set_task_sets(swb_handle h, int32_t n_sets, const swb_task_set* sets);

/* The set of every pool entry: set_of_entry_host is u8[P], P the entries of the pool the handle holds.  swb_set_pool,
 * swb_sample_pool and swb_sample_pool_tree put every entry in set 0; swb_copy_pool copies the source's assignment (and refuses
 * with SWB_ERR_INVALID when the two handles' tables differ); swb_resample_pool keeps it.
 * Validated first: a value >= the number of sets returns SWB_ERR_INVALID and changes nothing.  Uploaded on `stream`
 * (synchronous with respect to the host array: it may be freed on return).  Takes effect at once, also for running episodes
 * -- the set is looked up by entry at every step --, and makes every task record stale (swb_task_stats: one evaluation per
 * environment at its next step); run lists and cached frames stay valid.  SWB_ERR_STATE: no task sets, no pool. */
int swb_set_entry_task_sets(swb_handle h, const uint8_t* set_of_entry_host /* [P] */, void* stream);

/* ... and back, into u8[P] of host memory.  Synchronous.  SWB_ERR_STATE: no task sets, no pool. */
int swb_get_entry_task_sets(swb_handle h, uint8_t* set_of_entry_host /* [P] */);

/* What an agent conditions on: set_dev[n] = the set of the entry environment n is in (i32[N], device memory).  One small
 * kernel (swb_env_task_sets_kernel), asynchronous on `stream`; the handle is only read.  Unspecified (but a valid set index)
 * for an environment that has had no FIRST step since its pool was installed.  SWB_ERR_STATE: no task sets, no pool. */
int swb_env_task_sets(swb_handle h, int32_t* set_dev /* i32[N], device */, void* stream);

/* Sprite attribute setters on a LIVE sprite (sprite.py:152-175; pinned by the reference's
 * tests/sprite_test.py:138-174), for sprite `sprite` of environment `env` in its current episode:
 *   SWB_ATTR_SHAPE  value = index into the uploaded shape table: _shape = s; _reset_centered_path()
 *                   (a fresh path from the new shape and the CURRENT scale and angle, :96-101)
 *   SWB_ATTR_ANGLE  value = degrees: the current centred path is rotated by (value - angle)   (:161-165)
 *   SWB_ATTR_SCALE  value = scale:   the current centred path is scaled by (value - scale) -- the
 *                   DIFFERENCE, as the reference does (:171-175), not the ratio
 * The transforms are incremental, exactly like the reference's (matplotlib Affine2D + transform_path,
 * restated on the host): after a setter the sprite's centred path is no longer a function of its
 * factors, so the library keeps the path itself (device memory, allocated at the first call: N x S x
 * SWB_MAX_SHAPE_VERTS x 16 B) and the engine switches to the kernel build that reads it.  hit-tests
 * (contains_point), rendering and the SpriteFactors observation all see the new attribute; the
 * overrides end with the episode (the next reset draws fresh sprites, environment.py:74-78).
 *   delta  NULL: the difference (value - old) is taken in float64 from the stored factor.  Non-NULL:
 *          the difference the caller computed (e.g. in float32, when the sprite's factor is an
 *          np.float32 and numpy's promotion rules keep `a - self._angle` in float32).
 *   label  NULL: the sprite keeps its task labels.  Non-NULL: i8[n_tasks] new labels (the caller
 *          re-evaluated `filter.contains(sprite.factors)`, tasks.py:134-137,196-205, for filters that
 *          key on the changed attribute).
 * Blocking (synchronises `stream`); SWB_ERR_STATE when the environment has no live episode (never
 * reset, or its episode just ended).  Not part of the step path: call rates of a few per second. */
enum swb_sprite_attr { SWB_ATTR_SHAPE = 0, SWB_ATTR_ANGLE = 1, SWB_ATTR_SCALE = 2 };
int swb_set_sprite_attr(swb_handle h, int32_t env, int32_t sprite, int32_t attr, double value, const double* delta,
                        const int8_t* label, void* stream);

/* The sprite as the engine currently sees it: shape index, angle, scale, and its centred path
 * (Sprite._centered_path.vertices, sprite.py:96-101) -- path_xy f64[SWB_MAX_SHAPE_VERTS][2], n_verts
 * entries written.  Any output pointer may be NULL.  Blocking. */
/* After swb_set_sprite_attr on a handle with tasks that key on position (swb_task::n_xcuts / n_ycuts): the sprite's labels
 * per cell of each task's grid, re-evaluated by the caller with the new attribute -- cells i8[n_tasks][SWB_MAX_CELLS], laid
 * out as swb_pool::cell_label.  Without the call the sprite keeps the per-cell labels of its pool entry.  Blocking. */
int swb_set_sprite_cell_labels(swb_handle h, int32_t env, int32_t sprite, const int8_t* cells, void* stream);

int swb_get_sprite(swb_handle h, int32_t env, int32_t sprite, int32_t* shape, double* angle, double* scale, int32_t* n_verts,
                   double* path_xy, void* stream);

/* The host arithmetic of the setters alone (no device access; for tests against matplotlib):
 *   SWB_ATTR_SHAPE  out = _reset_centered_path of the unit-scale vertices `in_xy` with scale = a, angle = b (degrees)
 *   SWB_ATTR_ANGLE  out = Affine2D().rotate_deg(a - b).transform_path(in)
 *   SWB_ATTR_SCALE  out = Affine2D().scale(a - b).transform_path(in) */
int swb_sprite_path_op(int32_t attr, double a, double b, int32_t n, const double* in_xy, double* out_xy);

/* Which kernels swb_step launches for this handle -- a step is two kernels on the caller's stream: "cover" (state,
 * geometry, coverage -> run lists; swb_cover_kernel<NW>, NW = 32-pixel canvas words per row, one wave per environment)
 * and "resample" (swb_resample_kernel<VS>, VS output rows in flight; swb_fill_kernel when anti_aliasing = 1), one wave
 * per (environment, group of 64 output columns, band of output rows) -- so that measurement code can label a
 * run by what actually ran.  swb_build_id(): content hash of the sources and flags the library was
 * built from (spriteworld_amd/build.py), "unknown" for a hand build. */
typedef struct swb_variant_info {
  int32_t nw;                 /* cover kernel: 32-pixel words per canvas row it is built for */
  int32_t ncol;               /* output columns per lane of the second kernel (always 1: wider images are column groups) */
  int32_t vs;                 /* resample kernel: output rows in flight (0: anti_aliasing = 1, the fill kernel) */
  int32_t lds_bytes_per_wave; /* cover kernel, = per environment */
  int32_t waves_per_simd;     /* register budget the cover kernel was compiled for */
  int32_t resample_waves_per_simd; /* ... the resample / fill kernel */
  int32_t n_bands;            /* bands of output rows: waves of the second kernel per (environment, column group) */
  int32_t n_column_groups;    /* groups of 64 output columns */
  int32_t run_cap;            /* a run list's own part (8-byte units per environment and column group): max(4, max_sprites + 1) per
                               * canvas row until swb_trim_run_lists, then 1.25 x the longest list written; a list that outgrows
                               * it moves to a segment of the shared arena */
  int32_t paint_in_cover;     /* 1: anti_aliasing = 1 and an image of up to 64 columns -- the cover kernel writes the frame
                               * itself and no second kernel is launched */
  int32_t arena_units;        /* units of the arena the run lists of all environments share for their overflow (0 until the first
                               * launch allocates it); a scene that finds it exhausted flags its environment */
  int32_t large_frames;       /* 1: a frame the tuned kernels cannot take (canvas wider than 640 px, image wider than 256
                               * columns; or SWB_LARGE_FRAMES=1 at swb_create): a step is the cover kernel's state phase
                               * (nw = 2, obs = NULL) followed by swb_lf_raster_kernel (rasterisation + horizontal pass)
                               * and swb_lf_vertical_kernel (vertical pass; not at anti_aliasing = 1); no run lists */
  int32_t many_sprites;       /* 1: more than 16 sprites (or SWB_MANY_SPRITES=1 at swb_create): the state phase is
                               * swb_ms_state_kernel (one wave per environment, lane s = sprite s), the frame is rendered by
                               * the large-frame kernels (large_frames is 1 too); no run lists */
  int32_t reserved_;
  int64_t run_list_bytes;     /* device memory of the hand-off lists: fixed parts + arena (0 until the first launch) */
  int64_t frame_cache_bytes;  /* device memory of the frame cache (swb_frame_stats): one frame per environment, 0 on a handle
                               * without one */
  int32_t split_bands;        /* split-bands mode (swb_split_stats): the bands a frame that resamples is cut into when its launch
                               * splits -- the count asked for until the first launch has placed them --, 0: the mode is off */
  int32_t split_pad_;
  int64_t task_cache_bytes;   /* device memory of the task cache (swb_task_stats): 16 bytes per environment, 0 on a handle
                               * without one */
} swb_variant_info;
int swb_variant(swb_handle h, swb_variant_info* out);
const char* swb_build_id(void);

/* Kernel timing: three HIP events recorded on `stream` per swb_step launch while enabled (before the cover kernel, between the
 * two kernels, after the second); swb_step_time_ms returns (total ms, launches) since enable.  A diagnostic: every event is a
 * completion signal between two kernels that would otherwise follow each other directly -- measured on MI355X, a run of
 * back-to-back steps is 6 % slower with it on.  To time a run, bracket it with ONE pair of events of your own. */
int swb_timing_enable(swb_handle h, int32_t enable);
int swb_step_time_ms(swb_handle h, double* total_ms, int64_t* launches);
/* The same interval split at the event between the two kernels of a step: cover (state, geometry,
 * coverage -> run lists) and resample / fill (run lists -> frames). */
int swb_kernel_times_ms(swb_handle h, double* cover_ms, double* resample_ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* SWB_H_ */
