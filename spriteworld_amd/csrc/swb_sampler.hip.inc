// swb_sampler.hip.inc -- device-side reset sampling (swb_sample_pool, include/swb.h).
//
// One thread per pool entry draws a whole episode: the declarative form of
// sprite_generators.generate_sprites / chain_generators / shuffle over Product-of-Continuous/Discrete
// factor distributions (reference sprite_generators.py:27-70,101-128, factor_distributions.py:81-158).
// Random numbers: Philox4x32-10 (Salmon et al., SC'11), key = seed, counter = (entry lo, block, entry hi, 0)
// with entry = first_entry + pool index.  (The fourth counter word, philox_stream::word3, is 0 here and in swb_sample_actions;
// swb_rollout_sampled's candidate m draws with 1 + m.)
//
// Draw order per entry (tests/_sampler_model.py restates it and is compared bit for bit):
//   0. if n_alternatives > 1: alternative = u32 % n_alternatives (the groups generated, in order)
//   1. per group: count = count_min + u32 % (count_max - count_min + 1)
//   2. Fisher-Yates over the m sprites of the first `shuffle` groups, i = m-1 .. 1: j = u32 % (i + 1)
//   3. per sprite, in generation order: x, y, shape (u32 % n), scale, angle, c0, c1, c2, x_vel, y_vel;
//      then per hold-out: while the sprite is inside its box, redraw the factors of redraw_mask in
//      index order.
//      A Discrete factor uses one u32 (index = u32 % n); a uniform factor uses two:
//      u = ((a >> 5) * 2^26 + (b >> 6)) * 2^-53, value = lo + (hi - lo) * u cast to the factor's dtype.
#pragma once

struct philox_stream {
  uint32_t key0, key1, entry, entry_hi, block;
  uint32_t out[4];
  int have;
  uint32_t word3 = 0u;

  __device__ void refill() {
    uint32_t c0 = entry, c1 = block, c2 = entry_hi, c3 = word3, k0 = key0, k1 = key1;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
      const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
      const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
      c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
      k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
    block += 1u;
    have = 4;
  }
  __device__ uint32_t u32() {
    if (have == 0) refill();
    const int i = 4 - have;
    have -= 1;
    return i == 0 ? out[0] : (i == 1 ? out[1] : (i == 2 ? out[2] : out[3]));
  }
  __device__ double uniform() {
    const uint32_t a = u32() >> 5, b = u32() >> 6;
    return __dmul_rn(__dadd_rn(__dmul_rn((double)a, 67108864.0), (double)b), 1.0 / 9007199254740992.0);
  }
};

// A sampled factor value with the type the reference would hold: np.float32 (py = 0), a Python
// float from a Discrete candidate list (py = 1) or an integer from Continuous(dtype=int) (py = 2).
struct factor_value { double v; int py; };

// One draw (factor_distributions.py:98-101,139-143).  UNIFORM kinds use two u32, DISCRETE one.
__device__ inline factor_value draw_factor(philox_stream& rng, const swb_factor& f, int* index = nullptr) {
  if (f.kind == SWB_FACTOR_DISCRETE) {
    const int i = (int)(rng.u32() % (uint32_t)f.n);
    if (index) *index = i;
    return {f.cand[i], 1};
  }
  const double val = __dadd_rn(f.lo, __dmul_rn(__dsub_rn(f.hi, f.lo), rng.uniform()));  // np.random.uniform
  if (f.kind == SWB_FACTOR_UNIFORM_INT) return {trunc(val), 2};                          // .astype(int)
  return {(double)(float)val, 0};                                                        // .astype(float32)
}

// NEP 50 arithmetic of colorsys.hsv_to_rgb on mixed np.float32 / Python-float operands: two Python
// floats combine in float64 and stay Python floats; anything with an np.float32 is a float32 operation
// (the Python operand is first rounded to float32).
__device__ inline factor_value ws_mul(factor_value a, factor_value b) {
  if (a.py && b.py) return {__dmul_rn(a.v, b.v), 1};
  return {(double)__fmul_rn((float)a.v, (float)b.v), 0};
}
__device__ inline factor_value ws_sub(factor_value a, factor_value b) {
  if (a.py && b.py) return {__dsub_rn(a.v, b.v), 1};
  return {(double)__fsub_rn((float)a.v, (float)b.v), 0};
}

// renderers/color_maps.py:24-38: (255 * np.array(colorsys.hsv_to_rgb(h, s, v))).astype(np.uint8).
__device__ inline uint32_t swb_hsv_to_rgb(factor_value h, factor_value s, factor_value v) {
  factor_value r, g, b;
  if (s.v == 0.0) {
    r = g = b = v;
  } else {
    const factor_value one{1.0, 1};
    const factor_value h6 = ws_mul(h, factor_value{6.0, 1});
    int i = (int)h6.v;
    const factor_value f = ws_sub(h6, factor_value{(double)i, 1});
    const factor_value p = ws_mul(v, ws_sub(one, s));
    const factor_value q = ws_mul(v, ws_sub(one, ws_mul(s, f)));
    const factor_value t = ws_mul(v, ws_sub(one, ws_mul(s, ws_sub(one, f))));
    i = i % 6;
    switch (i) {
      case 0: r = v; g = t; b = p; break;
      case 1: r = q; g = v; b = p; break;
      case 2: r = p; g = v; b = t; break;
      case 3: r = p; g = q; b = v; break;
      case 4: r = t; g = p; b = v; break;
      default: r = v; g = p; b = q; break;
    }
  }
  uint32_t R, G, B;
  if (r.py || g.py || b.py) {  // np.array of mixed scalars is float64
    R = (uint32_t)(int)__dmul_rn(255.0, r.v); G = (uint32_t)(int)__dmul_rn(255.0, g.v); B = (uint32_t)(int)__dmul_rn(255.0, b.v);
  } else {
    R = (uint32_t)(int)__fmul_rn(255.0f, (float)r.v); G = (uint32_t)(int)__fmul_rn(255.0f, (float)g.v);
    B = (uint32_t)(int)__fmul_rn(255.0f, (float)b.v);
  }
  return (R & 255u) | ((G & 255u) << 8) | ((B & 255u) << 16);
}

struct swb_sampler_args {
  const swb_sampler* spec;  // device copy
  int32_t P, S, T;
  uint64_t seed, first_entry;
  // swb_resample_pool: skip the entry each environment is playing (null: draw everything)
  const int32_t *live_entry, *env_pool_base, *env_pool_len;
  int32_t N;
  int32_t* p_n;
  double *p_x, *p_y, *p_xv, *p_yv, *p_scale, *p_ca, *p_sa, *p_angle, *p_color;
  int32_t* p_shape;
  uint32_t* p_rgb;
  int8_t* p_label;
  uint8_t* p_attr;          // [P][S] bit 0 / 1: angle / scale is an np.float32 (swb_pool::attr_f32)
};

__global__ void __launch_bounds__(256) swb_sample_pool_kernel(const swb_sampler_args a) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.P) return;
  if (a.live_entry) {
    // pools are laid out env-major with a fixed length (pool_base[n] = n * pool_len[0])
    const int k = a.env_pool_len[0];
    const int env = e / k;
    if (env < a.N && a.env_pool_base[env] == env * k && a.live_entry[env] == e) return;
  }
  const swb_sampler* __restrict__ sp = a.spec;
  philox_stream rng;
  rng.key0 = (uint32_t)a.seed; rng.key1 = (uint32_t)(a.seed >> 32); rng.block = 0u; rng.have = 0;
  const uint64_t ge = a.first_entry + (uint64_t)e;
  rng.entry = (uint32_t)ge; rng.entry_hi = (uint32_t)(ge >> 32);
  const int S = a.S, T = a.T;

  // sample_generator: which list of groups this episode generates
  int list[SWB_MAX_GROUPS];
  int G = sp->n_groups;
  if (sp->n_alternatives > 0) {
    const swb_alternative& alt = sp->alternatives[sp->n_alternatives > 1 ? (int)(rng.u32() % (uint32_t)sp->n_alternatives) : 0];
    G = alt.n;
    for (int g = 0; g < SWB_MAX_GROUPS; ++g) list[g] = alt.group[g < G ? g : 0];
  } else {
    for (int g = 0; g < SWB_MAX_GROUPS; ++g) list[g] = g;
  }
  int counts[SWB_MAX_GROUPS];
  int n = 0;
  for (int g = 0; g < G; ++g) {
    const swb_sprite_group& grp = sp->groups[list[g]];
    int c = grp.count_min + (int)(rng.u32() % (uint32_t)(grp.count_max - grp.count_min + 1));
    if (n + c > S) c = S - n;
    counts[g] = c;
    n += c;
  }
  // z-order: slot[k] = where the k-th generated sprite lands (sprite_generators.shuffle:124-126)
  uint8_t slot[SWB_MAX_SPRITES];
  for (int k = 0; k < SWB_MAX_SPRITES; ++k) slot[k] = (uint8_t)k;
  int n_shuffled = 0;
  for (int g = 0; g < G && g < sp->shuffle; ++g) n_shuffled += counts[g];
  if (n_shuffled > 1)
    for (int i = n_shuffled - 1; i >= 1; --i) {
      const int j = (int)(rng.u32() % (uint32_t)(i + 1));
      const uint8_t t = slot[i]; slot[i] = slot[j]; slot[j] = t;
    }
  a.p_n[e] = n;
  int k = 0;
  for (int g = 0; g < G; ++g) {
    const swb_sprite_group& grp = sp->groups[list[g]];
    for (int c = 0; c < counts[g]; ++c, ++k) {
      const size_t o = (size_t)e * S + slot[k];
      factor_value fv[SWB_N_FACTORS];
      int ian = 0;
      fv[SWB_F_X] = draw_factor(rng, grp.factors[SWB_F_X]);
      fv[SWB_F_Y] = draw_factor(rng, grp.factors[SWB_F_Y]);
      const int ish = (int)(rng.u32() % (uint32_t)grp.n_shapes);
#pragma unroll
      for (int i = SWB_F_SCALE; i < SWB_N_FACTORS; ++i) fv[i] = draw_factor(rng, grp.factors[i], i == SWB_F_ANGLE ? &ian : nullptr);
      for (int hh = 0; hh < grp.n_holdouts; ++hh) {  // SetMinus rejection (at most _MAX_TRIES = 10000 redraws)
        const swb_holdout& ho = grp.holdouts[hh];
        for (int tries = 1; tries < 10000; ++tries) {
          bool inside = true;
#pragma unroll
          for (int i = 0; i < SWB_N_FACTORS; ++i)
            if ((ho.box_mask >> i) & 1u) inside = inside && (ho.lo[i] <= fv[i].v) && (fv[i].v < ho.hi[i]);
          if (!inside) break;
#pragma unroll
          for (int i = 0; i < SWB_N_FACTORS; ++i)
            if ((ho.redraw_mask >> i) & 1u) fv[i] = draw_factor(rng, grp.factors[i], i == SWB_F_ANGLE ? &ian : nullptr);
        }
      }
      const factor_value x = fv[SWB_F_X], y = fv[SWB_F_Y], scale = fv[SWB_F_SCALE], angle = fv[SWB_F_ANGLE], c0 = fv[SWB_F_C0],
                         c1 = fv[SWB_F_C1], c2 = fv[SWB_F_C2], xv = fv[SWB_F_XVEL], yv = fv[SWB_F_YVEL];
      a.p_x[o] = x.v; a.p_y[o] = y.v; a.p_xv[o] = xv.v; a.p_yv[o] = yv.v;
      a.p_shape[o] = grp.shapes[ish];
      a.p_scale[o] = scale.v;
      a.p_angle[o] = angle.v;
      if (grp.factors[SWB_F_ANGLE].kind == SWB_FACTOR_DISCRETE) {
        a.p_ca[o] = grp.cos_a[ian]; a.p_sa[o] = grp.sin_a[ian];
      } else {  // integer degrees in [0, 360]
        const int d = ((int)angle.v) % 360;
        a.p_ca[o] = sp->deg_cos[d]; a.p_sa[o] = sp->deg_sin[d];
      }
      a.p_color[3 * o] = c0.v; a.p_color[3 * o + 1] = c1.v; a.p_color[3 * o + 2] = c2.v;
      uint32_t rgb;
      if (sp->color_map == 1) rgb = swb_hsv_to_rgb(c0, c1, c2);
      else rgb = ((uint32_t)(int)c0.v & 255u) | (((uint32_t)(int)c1.v & 255u) << 8) | (((uint32_t)(int)c2.v & 255u) << 16);
      a.p_rgb[o] = rgb;
      for (int t = 0; t < T; ++t) a.p_label[((size_t)e * T + t) * S + slot[k]] = grp.label[t];
      a.p_attr[o] = (uint8_t)((angle.py == 0 ? 1 : 0) | (scale.py == 0 ? 2 : 0));
    }
  }
  // unused slots: neutral values (never read: every loop is bounded by n_sprites)
  for (int q = n; q < S; ++q) {
    const size_t o = (size_t)e * S + q;
    a.p_x[o] = 0.0; a.p_y[o] = 0.0; a.p_xv[o] = 0.0; a.p_yv[o] = 0.0; a.p_shape[o] = 0; a.p_scale[o] = 1.0;
    a.p_angle[o] = 0.0; a.p_ca[o] = 1.0; a.p_sa[o] = 0.0; a.p_rgb[o] = 0u;
    a.p_color[3 * o] = 0.0; a.p_color[3 * o + 1] = 0.0; a.p_color[3 * o + 2] = 0.0;
    a.p_attr[o] = 0;
    for (int t = 0; t < T; ++t) a.p_label[((size_t)e * T + t) * S + q] = 0;
  }
}

// --------------------------------------------------------------------------------------------
// The general sampler (swb_sample_pool_tree, include/swb.h): any tree of factor distributions, as a bytecode program per sprite
// group, with `contains()` as postfix predicates over leaf tests -- so rejection loops close on the device, labels are evaluated
// per sprite from the values drawn, and per cell of the position grid for tasks that key on position.
// The launch shape, the Philox streams, the live-entry skip and steps 0 - 2 of the draw order are swb_sample_pool_kernel's
// (with `alternatives_weighted`, step 0 is one uniform() against alternative_cdf).  Then per sprite, in generation order, the
// group's program from its first op until it runs off its end (tests/_sampler_tree_model.py restates it, bit for bit):
//   DRAW    UNIFORM_*: two u32, as draw_factor.  DISCRETE: u32 % n, or weighted: u = uniform(), index = #{i : cdf[i] <= u}.
//   CHOOSE  u = uniform(), go to target[#{i : cdf[i] <= u}].
//   JUMP    forward.
//   TEST    predicate == accept_if: go on; else one more of the sprite's max_tries is spent and the program goes back to
//           retry_pc -- when none is left the draw is kept, every later TEST passes and the sprite is counted as exhausted.
// Every jump was checked on the host: backward only from TEST, so a sprite takes at most (max_tries + 1) * n_ops ops.
// --------------------------------------------------------------------------------------------
struct swb_tree_dev {            // what the kernel reads: the caller's spec and the position grids of the handle's tasks
  swb_tree_sampler spec;
  int32_t n_xcuts[SWB_MAX_TASKS], n_ycuts[SWB_MAX_TASKS];
  double xcuts[SWB_MAX_TASKS][SWB_MAX_CUTS], ycuts[SWB_MAX_TASKS][SWB_MAX_CUTS];
};

struct swb_tree_args {
  swb_sampler_args pool;         // (spec unused)
  const swb_tree_dev* tree;
  int8_t* p_cell_label;          // [P][T][S][SWB_MAX_CELLS], or null: no task of the handle keys on position
  unsigned long long* exhausted; // sprites whose retry budget ran out
};

// The factors of the sprite being drawn, each with the type the reference would hold (factor_value::py; `shape`: its table index).
struct tree_values {
  double v[SWB_TREE_N_FACTORS];
  int py[SWB_TREE_N_FACTORS];
};

// numpy's choice(p=...): cdf.searchsorted(u, side='right')
__device__ inline int tree_cdf_index(const double* cdf, int n, double u) {
  int i = 0;
  for (int k = 0; k < n; ++k) i += (cdf[k] <= u) ? 1 : 0;
  return i < n ? i : n - 1;
}

// Continuous.contains / Discrete.contains of one leaf (factor_distributions.py:105-112,146-148) under NEP 50: an np.float32
// value meets the bound rounded to float32, every other value is compared in float64.
__device__ inline bool tree_leaf_test(const swb_tree_leaf& lf, const tree_values& tv) {
  const double v = tv.v[lf.factor];
  if (lf.factor == SWB_F_SHAPE) return ((lf.shape_mask >> ((uint32_t)(int)v & 31u)) & 1u) != 0u;
  const bool f32 = tv.py[lf.factor] == 0;
  if (lf.kind != SWB_FACTOR_DISCRETE) return f32 ? (v >= lf.lo32 && v < lf.hi32) : (v >= lf.lo && v < lf.hi);
  bool in = false;
  for (int i = 0; i < lf.n; ++i) in = in || (v == (f32 ? lf.cand32[i] : lf.cand[i]));
  return in;
}

// A predicate: postfix over leaf tests, the stack is the bits of one word (at most SWB_TREE_MAX_STACK deep: checked on the host).
__device__ inline bool tree_pred(const swb_tree_sampler& sp, int pi, const tree_values& tv) {
  const swb_tree_pred pr = sp.preds[pi];
  uint32_t st = 0u;
  for (int k = pr.first; k < pr.first + pr.n; ++k) {
    const swb_pred_node nd = sp.pred_nodes[k];
    if (nd.op == SWB_PRED_LEAF) {
      st = (st << 1) | (tree_leaf_test(sp.leaves[nd.leaf], tv) ? 1u : 0u);
    } else if (nd.op == SWB_PRED_TRUE) {
      st = (st << 1) | 1u;
    } else {
      const uint32_t b = st & 1u, a = (st >> 1) & 1u;
      const uint32_t r = nd.op == SWB_PRED_AND ? (a & b) : (nd.op == SWB_PRED_OR ? (a | b) : (a & (b ^ 1u)));
      st = ((st >> 2) << 1) | r;
    }
  }
  return (st & 1u) != 0u;
}

// tasks.py:134-137 (FindGoalPosition filter), :196-205 (first cluster that contains the sprite, else -1)
__device__ inline int tree_label(const swb_tree_sampler& sp, const swb_tree_task& tk, const tree_values& tv) {
  if (tk.kind == SWB_TASK_FIND_GOAL) return tk.n_preds == 0 ? 1 : (tree_pred(sp, tk.pred[0], tv) ? 1 : 0);
  if (tk.kind == SWB_TASK_CLUSTERING) {
    for (int k = 0; k < tk.n_preds; ++k)
      if (tree_pred(sp, tk.pred[k], tv)) return k;
    return -1;
  }
  return 0;
}

__global__ void __launch_bounds__(256) swb_sample_tree_kernel(const swb_tree_args ta) {
  const swb_sampler_args& a = ta.pool;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.P) return;
  if (a.live_entry) {
    // pools are laid out env-major with a fixed length (pool_base[n] = n * pool_len[0])
    const int k = a.env_pool_len[0];
    const int env = e / k;
    if (env < a.N && a.env_pool_base[env] == env * k && a.live_entry[env] == e) return;
  }
  const swb_tree_dev* __restrict__ td = ta.tree;
  const swb_tree_sampler& sp = td->spec;
  philox_stream rng;
  rng.key0 = (uint32_t)a.seed; rng.key1 = (uint32_t)(a.seed >> 32); rng.block = 0u; rng.have = 0;
  const uint64_t ge = a.first_entry + (uint64_t)e;
  rng.entry = (uint32_t)ge; rng.entry_hi = (uint32_t)(ge >> 32);
  const int S = a.S, T = a.T;

  // sample_generator: which list of groups this episode generates
  int list[SWB_MAX_GROUPS];
  int G = sp.n_groups;
  if (sp.n_alternatives > 0) {
    int ai = 0;
    if (sp.alternatives_weighted) ai = tree_cdf_index(sp.alternative_cdf, sp.n_alternatives, rng.uniform());
    else if (sp.n_alternatives > 1) ai = (int)(rng.u32() % (uint32_t)sp.n_alternatives);
    const swb_alternative& alt = sp.alternatives[ai];
    G = alt.n;
    for (int g = 0; g < SWB_MAX_GROUPS; ++g) list[g] = alt.group[g < G ? g : 0];
  } else {
    for (int g = 0; g < SWB_MAX_GROUPS; ++g) list[g] = g;
  }
  int counts[SWB_MAX_GROUPS];
  int n = 0;
  for (int g = 0; g < G; ++g) {
    const swb_tree_group& grp = sp.groups[list[g]];
    int c = grp.count_min + (int)(rng.u32() % (uint32_t)(grp.count_max - grp.count_min + 1));
    if (n + c > S) c = S - n;
    counts[g] = c;
    n += c;
  }
  // z-order: slot[k] = where the k-th generated sprite lands (sprite_generators.shuffle:124-126)
  uint8_t slot[SWB_MAX_SPRITES];
  for (int k = 0; k < SWB_MAX_SPRITES; ++k) slot[k] = (uint8_t)k;
  int n_shuffled = 0;
  for (int g = 0; g < G && g < sp.shuffle; ++g) n_shuffled += counts[g];
  if (n_shuffled > 1)
    for (int i = n_shuffled - 1; i >= 1; --i) {
      const int j = (int)(rng.u32() % (uint32_t)(i + 1));
      const uint8_t t = slot[i]; slot[i] = slot[j]; slot[j] = t;
    }
  a.p_n[e] = n;
  unsigned long long n_spent = 0ull;
  int k = 0;
  for (int g = 0; g < G; ++g) {
    const swb_tree_group& grp = sp.groups[list[g]];
    for (int c = 0; c < counts[g]; ++c, ++k) {
      const size_t o = (size_t)e * S + slot[k];
      tree_values tv;
      for (int i = 0; i < SWB_TREE_N_FACTORS; ++i) { tv.v[i] = grp.defaults[i]; tv.py[i] = 1; }
      double ca = grp.default_cos, sa = grp.default_sin;
      int tries = 0;
      bool spent = false;
      const int end = grp.first_op + grp.n_ops;
      for (int pc = grp.first_op; pc < end;) {
        const swb_tree_op op = sp.ops[pc];
        if (op.kind == SWB_OP_DRAW) {
          const swb_tree_leaf& lf = sp.leaves[op.a];
          if (lf.kind == SWB_FACTOR_DISCRETE) {
            const int i = lf.weighted ? tree_cdf_index(lf.cdf, lf.n, rng.uniform()) : (int)(rng.u32() % (uint32_t)lf.n);
            tv.v[lf.factor] = lf.cand[i]; tv.py[lf.factor] = 1;
            if (lf.factor == SWB_F_ANGLE) { ca = lf.cos_a[i]; sa = lf.sin_a[i]; }
          } else {
            const double val = __dadd_rn(lf.lo, __dmul_rn(__dsub_rn(lf.hi, lf.lo), rng.uniform()));  // np.random.uniform
            if (lf.kind == SWB_FACTOR_UNIFORM_INT) {                                                 // .astype(int)
              tv.v[lf.factor] = trunc(val); tv.py[lf.factor] = 2;
              if (lf.factor == SWB_F_ANGLE) {   // integer degrees in [0, 360]
                const int d = ((int)tv.v[lf.factor]) % 360;
                ca = sp.deg_cos[d]; sa = sp.deg_sin[d];
              }
            } else {                                                                                 // .astype(float32)
              tv.v[lf.factor] = (double)(float)val; tv.py[lf.factor] = 0;
            }
          }
          ++pc;
        } else if (op.kind == SWB_OP_CHOOSE) {
          const swb_tree_choice& ch = sp.choices[op.a];
          pc = ch.target[tree_cdf_index(ch.cdf, ch.n, rng.uniform())];
        } else if (op.kind == SWB_OP_JUMP) {
          pc = op.a;
        } else {  // SWB_OP_TEST
          if (spent || tree_pred(sp, op.a, tv) == (op.b != 0)) {
            ++pc;
          } else if (++tries >= sp.max_tries) {
            spent = true;
            ++pc;
          } else {
            pc = op.c;
          }
        }
      }
      if (spent) n_spent += 1ull;
      const factor_value x{tv.v[SWB_F_X], tv.py[SWB_F_X]}, y{tv.v[SWB_F_Y], tv.py[SWB_F_Y]};
      const factor_value scale{tv.v[SWB_F_SCALE], tv.py[SWB_F_SCALE]}, angle{tv.v[SWB_F_ANGLE], tv.py[SWB_F_ANGLE]};
      const factor_value c0{tv.v[SWB_F_C0], tv.py[SWB_F_C0]}, c1{tv.v[SWB_F_C1], tv.py[SWB_F_C1]}, c2{tv.v[SWB_F_C2], tv.py[SWB_F_C2]};
      a.p_x[o] = x.v; a.p_y[o] = y.v; a.p_xv[o] = tv.v[SWB_F_XVEL]; a.p_yv[o] = tv.v[SWB_F_YVEL];
      a.p_shape[o] = (int32_t)tv.v[SWB_F_SHAPE];
      a.p_scale[o] = scale.v;
      a.p_angle[o] = angle.v;
      a.p_ca[o] = ca; a.p_sa[o] = sa;
      a.p_color[3 * o] = c0.v; a.p_color[3 * o + 1] = c1.v; a.p_color[3 * o + 2] = c2.v;
      uint32_t rgb;
      if (sp.color_map == 1) rgb = swb_hsv_to_rgb(c0, c1, c2);
      else rgb = ((uint32_t)(int)c0.v & 255u) | (((uint32_t)(int)c1.v & 255u) << 8) | (((uint32_t)(int)c2.v & 255u) << 16);
      a.p_rgb[o] = rgb;
      a.p_attr[o] = (uint8_t)((angle.py == 0 ? 1 : 0) | (scale.py == 0 ? 2 : 0));
      for (int t = 0; t < T; ++t) {
        const size_t lo = ((size_t)e * T + t) * S + slot[k];
        a.p_label[lo] = (int8_t)tree_label(sp, sp.tasks[t], tv);
        if (!ta.p_cell_label) continue;
        // lowering.cell_labels_of: the label with x / y at the representative of every cell of the task's grid
        int8_t* cells = ta.p_cell_label + lo * SWB_MAX_CELLS;
        const int nx = td->n_xcuts[t], ny = td->n_ycuts[t];
        int q = 0;
        if (nx + ny > 0) {
          tv.py[SWB_F_X] = 0; tv.py[SWB_F_Y] = 0;
          for (int cy = 0; cy <= ny; ++cy)
            for (int cx = 0; cx <= nx; ++cx, ++q) {
              tv.v[SWB_F_X] = cx == 0 ? -__builtin_huge_val() : td->xcuts[t][cx - 1];
              tv.v[SWB_F_Y] = cy == 0 ? -__builtin_huge_val() : td->ycuts[t][cy - 1];
              cells[q] = (int8_t)tree_label(sp, sp.tasks[t], tv);
            }
          tv.v[SWB_F_X] = x.v; tv.py[SWB_F_X] = x.py; tv.v[SWB_F_Y] = y.v; tv.py[SWB_F_Y] = y.py;
        }
        for (; q < SWB_MAX_CELLS; ++q) cells[q] = 0;
      }
    }
  }
  if (n_spent) atomicAdd(ta.exhausted, n_spent);
  // unused slots: neutral values (never read: every loop is bounded by n_sprites)
  for (int q = n; q < S; ++q) {
    const size_t o = (size_t)e * S + q;
    a.p_x[o] = 0.0; a.p_y[o] = 0.0; a.p_xv[o] = 0.0; a.p_yv[o] = 0.0; a.p_shape[o] = 0; a.p_scale[o] = 1.0;
    a.p_angle[o] = 0.0; a.p_ca[o] = 1.0; a.p_sa[o] = 0.0; a.p_rgb[o] = 0u;
    a.p_color[3 * o] = 0.0; a.p_color[3 * o + 1] = 0.0; a.p_color[3 * o + 2] = 0.0;
    a.p_attr[o] = 0;
    for (int t = 0; t < T; ++t) {
      const size_t lo = ((size_t)e * T + t) * S + q;
      a.p_label[lo] = 0;
      if (ta.p_cell_label)
        for (int c = 0; c < SWB_MAX_CELLS; ++c) ta.p_cell_label[lo * SWB_MAX_CELLS + c] = 0;
    }
  }
}

// --------------------------------------------------------------------------------------------
// Random-agent actions (swb_sample_actions, include/swb.h): one wave per environment draws the environment's next action
// -- uniform, or a click inside a randomly chosen sprite (environment.py:110-126, sprite.py:117-126) -- from the sprites as
// they are now.  The handle is only read, and everything read was written by earlier launches (as_const: scalar loads).
// Every lane runs the same Philox stream (key = seed, entry = first_env + environment), so every drawn value is wave-uniform,
// as the ballot of contains_point_wave requires.  Draw order (tests/_random_agent_model.py restates it, bit for bit):
//   UNIFORM    SelectMove / DragAndDrop: a[0..3] = uniform().  Embodied: a[0] = u32 % 2, a[1] = u32 % 4.
//   ON_SPRITE  1. n = nspr[env]; n == 0: sprite = -1, tries = 0, position = (uniform(), uniform()), on with 4.
//              2. s = u32 % n
//              3. the centred path of sprite s into LDS, lanes = vertices (ov_cpath when the environment carries setter
//                 overrides, else centered_vertex); low / high = exact min / max over the vertices (wave reduction).
//                 Per try: ux, uy = uniform(); d = low + (high - low) * u (numpy's uniform(low, high)); sample = pos + d
//                 (sprite.py:122); accepted if the path contains sample - pos (sprite.py:115) -- all float64, no FMA.
//                 After SWB_CONTAINED_MAX_TRIES misses: tries = -1, sample = pos (the reference raises after 10^6).
//              4. SelectMove / DragAndDrop: a[0], a[1] = sample, a[2], a[3] = uniform().  Embodied: the integer draws of UNIFORM.
// --------------------------------------------------------------------------------------------
#ifndef SWB_WIDE_TU
struct swb_sample_actions_args {
  int32_t mode;
  uint64_t seed, first_env;
  void* actions;               // [N][4] f64 / f32 or [N][2] i32; any output may be NULL
  double* position;            // [N][2]
  int32_t *sprite, *tries;     // [N]
};

static_assert(sizeof(swb_params) + sizeof(swb_sample_actions_args) <= 4096, "kernel arguments of swb_sample_actions_kernel");

__device__ __forceinline__ double wave_min_d(double v) {
  for (int o = 32; o > 0; o >>= 1) { const double w = __shfl_xor(v, o, 64); v = (w < v) ? w : v; }
  return v;
}
__device__ __forceinline__ double wave_max_d(double v) {
  for (int o = 32; o > 0; o >>= 1) { const double w = __shfl_xor(v, o, 64); v = (w > v) ? w : v; }
  return v;
}

__global__ void __launch_bounds__(SWB_WAVE)
swb_sample_actions_kernel(const swb_params p, const swb_sample_actions_args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double2* cpath = reinterpret_cast<double2*>(smem);    // SWB_MAX_SHAPE_VERTS vertices: 1 KiB
  const int l = lane_id();
  const int env = blockIdx.x;
  const int S = p.S;
  philox_stream rng;
  rng.key0 = (uint32_t)a.seed; rng.key1 = (uint32_t)(a.seed >> 32); rng.block = 0u; rng.have = 0;
  const uint64_t ge = a.first_env + (uint64_t)env;
  rng.entry = (uint32_t)ge; rng.entry_hi = (uint32_t)(ge >> 32);
  const bool embodied = p.action_space == SWB_ACTION_EMBODIED;
  double a0 = 0.0, a1 = 0.0;
  if (a.mode == SWB_SAMPLE_ON_SPRITE) {
    const int n = min(max(as_const(p.nspr)[env], 0), S);
    int sprite = -1, tries = 0;
    if (n == 0) {
      a0 = rng.uniform(); a1 = rng.uniform();
    } else {
      sprite = (int)(rng.u32() % (uint32_t)n);
      const size_t o = (size_t)env * S + sprite, pe = (size_t)as_const(p.entry)[env] * S + sprite;
      const bool ov = p.ov_flag != nullptr && as_const(p.ov_flag)[env] != 0;   // sprite.py:152-175 setters were applied to this episode
      const int shape = ov ? as_const(p.ov_shape)[o] : as_const(p.p_shape)[pe];
      const int sh_idx = (int)min((uint32_t)shape, (uint32_t)(SWB_MAX_SHAPES - 1));
      const int so = as_const(p.shape_off)[sh_idx];
      const int nv = min(as_const(p.shape_off)[sh_idx + 1] - so, SWB_MAX_SHAPE_VERTS);
      const double px = as_const(p.x)[o], py = as_const(p.y)[o];
      double cx = 0.0, cy = 0.0;
      if (l < nv) {
        if (ov) {                                       // the path the setters left (host arithmetic, swb.hip)
          const double* q = p.ov_cpath + (o * SWB_MAX_SHAPE_VERTS + l) * 2;
          cx = q[0]; cy = q[1];
        } else {
          centered_vertex(p, so, l, as_const(p.p_scale)[pe], as_const(p.p_ca)[pe], as_const(p.p_sa)[pe], cx, cy);
        }
        cpath[l] = make_double2(cx, cy);
      }
      wave_sync();
      // sprite.py:119-120: np.min / np.max over the vertices (lanes beyond the path repeat vertex 0)
      const double fx = readlane_d(cx, 0), fy = readlane_d(cy, 0);
      const double vx = (l < nv) ? cx : fx, vy = (l < nv) ? cy : fy;
      const double lo_x = wave_min_d(vx), lo_y = wave_min_d(vy), hi_x = wave_max_d(vx), hi_y = wave_max_d(vy);
      const double w_x = __dsub_rn(hi_x, lo_x), w_y = __dsub_rn(hi_y, lo_y);
      a0 = px; a1 = py; tries = -1;
      for (int t = 1; t <= SWB_CONTAINED_MAX_TRIES; ++t) {
        const double ux = rng.uniform(), uy = rng.uniform();
        const double sx = __dadd_rn(px, __dadd_rn(lo_x, __dmul_rn(w_x, ux)));
        const double sy = __dadd_rn(py, __dadd_rn(lo_y, __dmul_rn(w_y, uy)));
        if (contains_point_wave(cpath, nv, __dsub_rn(sx, px), __dsub_rn(sy, py))) {   // (the test point is sample - pos)
          a0 = sx; a1 = sy; tries = t;
          break;
        }
      }
    }
    if (l == 0) {
      if (a.position) { a.position[2 * (size_t)env] = a0; a.position[2 * (size_t)env + 1] = a1; }
      if (a.sprite) a.sprite[env] = sprite;
      if (a.tries) a.tries[env] = tries;
    }
  } else if (!embodied) {
    a0 = rng.uniform(); a1 = rng.uniform();
  }
  if (embodied) {
    const int carry = (int)(rng.u32() % 2u), dir = (int)(rng.u32() % 4u);
    if (l == 0 && a.actions) {
      int32_t* q = reinterpret_cast<int32_t*>(a.actions) + 2 * (size_t)env;
      q[0] = carry; q[1] = dir;
    }
    return;
  }
  const double a2 = rng.uniform(), a3 = rng.uniform();
  if (l == 0 && a.actions) {
    if (p.action_is_f32) {
      float* q = reinterpret_cast<float*>(a.actions) + 4 * (size_t)env;
      q[0] = (float)a0; q[1] = (float)a1; q[2] = (float)a2; q[3] = (float)a3;
    } else {
      double* q = reinterpret_cast<double*>(a.actions) + 4 * (size_t)env;
      q[0] = a0; q[1] = a1; q[2] = a2; q[3] = a3;
    }
  }
}

// --------------------------------------------------------------------------------------------
// Rollouts that draw their own candidates (swb_rollout_sampled, include/swb.h): what the SAMPLE builds of swb_rollout_kernel
// (swb_kernels.hip.inc) call.  After every load_env_state, draw() replaces the step's action by one drawn from the sprites the
// step acts on -- `es`, the registers of the wave: on a FIRST step the fresh episode's (the dynamics ignore that action; it is
// drawn all the same, so the stream's position never depends on step types).  Virtual environment (n, m) owns ONE stream for the
// K steps: key = seed, counter = (entry lo, block, entry hi, 1 + m), entry = first_env + n -- every lane reads the same values
// of it (rollout_rng below), so the draws are wave-uniform.
// Per step the draw order is swb_sample_actions_kernel's above, with es.n for nspr, cross-lane reads of es for the chosen
// sprite's position, scale, rotation and shape, and the path buffer of the hit test (its first wave_sync() orders our reads).
// Lanes 0..3 (0..1: Embodied) keep the drawn component in es.act / es.acti and store it to slot [k][v] of `actions`; a float32
// handle stores (float) of the float64 draw and steps with that float, what swb_rollout would load back.  Nothing stored here
// is read again by this launch.  The stream's state is wave-uniform and lives across the K steps.
// The draw is written out beside swb_sample_actions_kernel's, not shared with it: that kernel reads memory (as_const, setter
// overrides), this one registers.
// --------------------------------------------------------------------------------------------
// The stream is philox_stream's, value for value, but generated 64 values at a time by the lanes: lane l computes block
// (next / 4 + l / 4) and keeps its word l % 4, a draw is a cross-lane read with a wave-uniform index.  philox_stream itself, run
// by every lane on wave-uniform values, is compiled to scalar multiplies -- 40 per block, two blocks per uniform step --, and
// the scalar unit, one for the four SIMDs of a compute unit, then bounds the kernel: measured at N = 1024, M = 64, K = 16 and 5
// waves per SIMD, 1.80 ms against 1.22 ms for a torch.rand tensor and swb_rollout; this form takes 1.49 ms
// (profiles/r15_rollout_random.md, section 2).
struct rollout_rng {
  uint32_t key0, key1, entry, entry_hi, word3;
  uint32_t next;               // (uniform) values of the stream consumed so far
  uint32_t word;               // lane l: value number (next rounded down to 64) + l of the stream

  __device__ __forceinline__ uint32_t u32() {
    const uint32_t i = next & 63u;
    if (i == 0u) {                                      // (wave-uniform)
      const int l = lane_id();
      uint32_t c0 = entry, c1 = (next >> 2) + (uint32_t)(l >> 2), c2 = entry_hi, c3 = word3, k0 = key0, k1 = key1;
#pragma unroll
      for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
      }
      const int w = l & 3;
      word = w == 0 ? c0 : (w == 1 ? c1 : (w == 2 ? c2 : c3));
    }
    next += 1u;
    return (uint32_t)__builtin_amdgcn_readlane((int)word, (int)i);
  }
  __device__ __forceinline__ double uniform() {
    const uint32_t a = u32() >> 5, b = u32() >> 6;
    return __dmul_rn(__dadd_rn(__dmul_rn((double)a, 67108864.0), (double)b), 1.0 / 9007199254740992.0);
  }
};

template <>
struct rollout_drawer<true> {
  rollout_rng rng;

  __device__ __forceinline__ void start(const swb_rollout_sample_args& sa, int n_env, int m) {
    rng.key0 = (uint32_t)sa.seed; rng.key1 = (uint32_t)(sa.seed >> 32); rng.next = 0u; rng.word = 0u;
    const uint64_t ge = sa.first_env + (uint64_t)n_env;
    rng.entry = (uint32_t)ge; rng.entry_hi = (uint32_t)(ge >> 32);
    rng.word3 = 1u + (uint32_t)m;
  }

  __device__ __forceinline__ void draw(const swb_rollout_sample_args& sa, const swb_params& q, int k, env_state& es, double2* cpath) {
    const int l = lane_id();
    const int v = blockIdx.x;
    const size_t slot = (size_t)k * gridDim.x + v;      // (one workgroup per virtual environment: gridDim.x = N * M)
    const bool embodied = q.action_space == SWB_ACTION_EMBODIED;
    double a0 = 0.0, a1 = 0.0;
    if (sa.mode == SWB_SAMPLE_ON_SPRITE) {
      const int n = es.n;
      int sprite = -1, tries = 0;
      if (n == 0) {
        a0 = rng.uniform(); a1 = rng.uniform();
      } else {
        sprite = (int)(rng.u32() % (uint32_t)n);
        const int nv = min(__builtin_amdgcn_readlane(es.nv_l, sprite), SWB_MAX_SHAPE_VERTS), so = __builtin_amdgcn_readlane(es.so_l, sprite);
        const double sc = readlane_d(es.scale_l, sprite), ca = readlane_d(es.ca_l, sprite), sn = readlane_d(es.sa_l, sprite);
        const double px = readlane_d(es.px, sprite), py = readlane_d(es.py, sprite);
        double cx = 0.0, cy = 0.0;
        wave_sync();                                    // (the previous step's hit tests have read the path)
        if (l < nv) {
          centered_vertex(q, so, l, sc, ca, sn, cx, cy);
          cpath[l] = make_double2(cx, cy);
        }
        wave_sync();
        // sprite.py:119-120: np.min / np.max over the vertices (lanes beyond the path repeat vertex 0)
        const double fx = readlane_d(cx, 0), fy = readlane_d(cy, 0);
        const double vx = (l < nv) ? cx : fx, vy = (l < nv) ? cy : fy;
        const double lo_x = wave_min_d(vx), lo_y = wave_min_d(vy), hi_x = wave_max_d(vx), hi_y = wave_max_d(vy);
        const double w_x = __dsub_rn(hi_x, lo_x), w_y = __dsub_rn(hi_y, lo_y);
        a0 = px; a1 = py; tries = -1;
        for (int t = 1; t <= SWB_CONTAINED_MAX_TRIES; ++t) {
          const double ux = rng.uniform(), uy = rng.uniform();
          const double sx = __dadd_rn(px, __dadd_rn(lo_x, __dmul_rn(w_x, ux)));
          const double sy = __dadd_rn(py, __dadd_rn(lo_y, __dmul_rn(w_y, uy)));
          if (contains_point_wave(cpath, nv, __dsub_rn(sx, px), __dsub_rn(sy, py))) {   // (the test point is sample - pos)
            a0 = sx; a1 = sy; tries = t;
            break;
          }
        }
      }
      if (l == 0) {
        if (sa.sprite) sa.sprite[slot] = sprite;
        if (sa.tries) sa.tries[slot] = tries;
      }
    } else if (!embodied) {
      a0 = rng.uniform(); a1 = rng.uniform();
    }
    if (embodied) {
      const int carry = (int)(rng.u32() % 2u), dir = (int)(rng.u32() % 4u);
      es.acti = (l == 0) ? carry : dir;
      if (l < 2) reinterpret_cast<int32_t*>(sa.actions)[2 * slot + l] = es.acti;
      return;
    }
    const double a2 = rng.uniform(), a3 = rng.uniform();
    const double mine = (l == 0) ? a0 : ((l == 1) ? a1 : ((l == 2) ? a2 : a3));
    if (q.action_is_f32) {
      const float f = (float)mine;
      es.act = (double)f;
      if (l < 4) reinterpret_cast<float*>(sa.actions)[4 * slot + l] = f;
    } else {
      es.act = mine;
      if (l < 4) reinterpret_cast<double*>(sa.actions)[4 * slot + l] = mine;
    }
  }
};

// --------------------------------------------------------------------------------------------
// Rollouts that draw their candidates from a plan (swb_rollout_guided, include/swb.h): what swb_rollout_guided_kernel calls, in
// the place and under the rules of rollout_drawer<true> above -- the same stream per virtual environment, the same registers
// read, the same path buffer and wave_sync()s, the same stores.  The plan's row of (step k, environment n) is only read, and
// was written by earlier launches: its wave-uniform words (the row's total, the four motion parameters) are scalar loads
// (as_const) made once per step ahead of the tries loop, the running sum of lane l's sprite a plain vector load.
// Draw order per step (tests/_rollout_guided_model.py restates it, bit for bit; float64, no contraction):
//   SelectMove / DragAndDrop, n = es.n sprites, W' = min(n, W):
//     1. u_c = uniform(), always.
//     2. n == 0: sprite = -1, tries = 0, click = (uniform(), uniform()).
//     3. total = cdf[W' - 1].  No cdf, or total not finite and > 0: s = min((int)(u_c * n), n - 1).  Else t = u_c * total and
//        s = the first j < W' with cdf[j] > t; none (t rounded up to total): the first j with cdf[j] >= total -- lanes =
//        sprites, two ballots, a find-first.  A sprite of weight 0 has the running sum of its predecessor and is never first.
//     4. the click: ON_SPRITE's tries loop on sprite s.
//     5. c = 0, 1: z = (((u1 + u2) + (u3 + u4)) - 2) * sqrt(3) of four uniform()s (Irwin-Hall, n = 4: mean 0, variance 1,
//        |z| <= 2 sqrt(3)); v = mean[c] + std[c] * z; a[2 + c] = v > 0 ? (v < 1 ? v : 1) : 0 (a NaN gives 0).
//   Embodied: u_c = uniform(); idx by rule 3 with n = W' = 8; carry = idx / 4, direction = idx % 4.
// Nothing is indexed by a drawn or loaded floating-point value: s comes out of a ballot over lanes < W' <= n, or is clamped.
// --------------------------------------------------------------------------------------------
struct rollout_guided_drawer {
  rollout_rng rng;
  int n_env;

  __device__ __forceinline__ void start(const swb_rollout_guided_args& ga, int n_env_, int m) {
    rng.key0 = (uint32_t)ga.seed; rng.key1 = (uint32_t)(ga.seed >> 32); rng.next = 0u; rng.word = 0u;
    const uint64_t ge = ga.first_env + (uint64_t)n_env_;
    rng.entry = (uint32_t)ge; rng.entry_hi = (uint32_t)(ge >> 32);
    rng.word3 = 1u + (uint32_t)m;
    n_env = n_env_;
  }

  // rule 3 over the first `wp` running sums of the row at `cdf` (NULL: none), for `n` choices: wave-uniform
  __device__ __forceinline__ int choose(const double* cdf, int wp, int n, double u_c) {
    const int l = lane_id();
    double total = 0.0;
    if (cdf) total = as_const(cdf)[wp - 1];
    if (!(total > 0.0 && total < __builtin_huge_val())) return min((int)__dmul_rn(u_c, (double)n), n - 1);
    const double t = __dmul_rn(u_c, total);
    const double c = (l < wp) ? cdf[l] : 0.0;
    const unsigned long long above = __ballot(l < wp && c > t), reach = __ballot(l < wp && c >= total);
    return above ? __builtin_ctzll(above) : (reach ? __builtin_ctzll(reach) : wp - 1);
  }

  __device__ __forceinline__ void draw(const swb_rollout_guided_args& ga, const swb_params& q, int k, env_state& es, double2* cpath) {
    const int l = lane_id();
    const int v = blockIdx.x;
    const size_t slot = (size_t)k * gridDim.x + v;      // (one workgroup per virtual environment: gridDim.x = N * M)
    const size_t row = (size_t)k * ga.N + n_env;
    const double* cdf = ga.cdf ? ga.cdf + row * ga.W : nullptr;
    const double u_c = rng.uniform();
    if (q.action_space == SWB_ACTION_EMBODIED) {
      const int idx = choose(cdf, 8, 8, u_c);
      es.acti = (l == 0) ? idx / 4 : idx % 4;
      if (l < 2) reinterpret_cast<int32_t*>(ga.actions)[2 * slot + l] = es.acti;
      if (l == 0 && ga.sprite) ga.sprite[slot] = idx;
      return;
    }
    const double mean0 = as_const(ga.mean)[2 * row], mean1 = as_const(ga.mean)[2 * row + 1];
    const double std0 = as_const(ga.std)[2 * row], std1 = as_const(ga.std)[2 * row + 1];
    const int n = es.n;
    double a0 = 0.0, a1 = 0.0;
    int sprite = -1, tries = 0;
    if (n == 0) {
      a0 = rng.uniform(); a1 = rng.uniform();
    } else {
      sprite = choose(cdf, min(n, ga.W), n, u_c);
      const int nv = min(__builtin_amdgcn_readlane(es.nv_l, sprite), SWB_MAX_SHAPE_VERTS), so = __builtin_amdgcn_readlane(es.so_l, sprite);
      const double sc = readlane_d(es.scale_l, sprite), ca = readlane_d(es.ca_l, sprite), sn = readlane_d(es.sa_l, sprite);
      const double px = readlane_d(es.px, sprite), py = readlane_d(es.py, sprite);
      double cx = 0.0, cy = 0.0;
      wave_sync();                                      // (the previous step's hit tests have read the path)
      if (l < nv) {
        centered_vertex(q, so, l, sc, ca, sn, cx, cy);
        cpath[l] = make_double2(cx, cy);
      }
      wave_sync();
      // sprite.py:119-120: np.min / np.max over the vertices (lanes beyond the path repeat vertex 0)
      const double fx = readlane_d(cx, 0), fy = readlane_d(cy, 0);
      const double vx = (l < nv) ? cx : fx, vy = (l < nv) ? cy : fy;
      const double lo_x = wave_min_d(vx), lo_y = wave_min_d(vy), hi_x = wave_max_d(vx), hi_y = wave_max_d(vy);
      const double w_x = __dsub_rn(hi_x, lo_x), w_y = __dsub_rn(hi_y, lo_y);
      a0 = px; a1 = py; tries = -1;
      for (int t = 1; t <= SWB_CONTAINED_MAX_TRIES; ++t) {
        const double ux = rng.uniform(), uy = rng.uniform();
        const double sx = __dadd_rn(px, __dadd_rn(lo_x, __dmul_rn(w_x, ux)));
        const double sy = __dadd_rn(py, __dadd_rn(lo_y, __dmul_rn(w_y, uy)));
        if (contains_point_wave(cpath, nv, __dsub_rn(sx, px), __dsub_rn(sy, py))) {   // (the test point is sample - pos)
          a0 = sx; a1 = sy; tries = t;
          break;
        }
      }
    }
    if (l == 0) {
      if (ga.sprite) ga.sprite[slot] = sprite;
      if (ga.tries) ga.tries[slot] = tries;
    }
    const double a2 = motion(mean0, std0), a3 = motion(mean1, std1);
    const double mine = (l == 0) ? a0 : ((l == 1) ? a1 : ((l == 2) ? a2 : a3));
    if (q.action_is_f32) {
      const float f = (float)mine;
      es.act = (double)f;
      if (l < 4) reinterpret_cast<float*>(ga.actions)[4 * slot + l] = f;
    } else {
      es.act = mine;
      if (l < 4) reinterpret_cast<double*>(ga.actions)[4 * slot + l] = mine;
    }
  }

  // rule 5: one motion component
  __device__ __forceinline__ double motion(double mean, double std) {
    const double u1 = rng.uniform(), u2 = rng.uniform(), u3 = rng.uniform(), u4 = rng.uniform();
    const double z = __dmul_rn(__dsub_rn(__dadd_rn(__dadd_rn(u1, u2), __dadd_rn(u3, u4)), 2.0), 1.7320508075688772);
    const double v = __dadd_rn(mean, __dmul_rn(std, z));
    return v > 0.0 ? (v < 1.0 ? v : 1.0) : 0.0;
  }
};
#endif  // SWB_WIDE_TU
