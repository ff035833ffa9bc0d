// host_task_cache.cc -- drives the C ABI (include/swb.h) of the EMULATED library through the host side of the task cache, for
// tests/test_host_task_cache.py: create -> steps -> each call that moves the task epoch -> steps -> the calls that must not
// -> destroy, with swb_task_stats held at every stage.  Three handles: with the cache, with SWB_NO_TASK_CACHE, and without the
// counters.  Built with -fsanitize=address / undefined together with the host sources.  "Device" pointers are host memory here
// (tests/emu/README.md).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "swb.h"

namespace {

int g_failures = 0;

#define EXPECT_RC(want, expr)                                                                                   \
  do {                                                                                                          \
    const int rc_ = (expr);                                                                                     \
    if (rc_ != (want)) {                                                                                        \
      fprintf(stderr, "%s:%d: %s returned %d (%s), expected %d\n", __FILE__, __LINE__, #expr, rc_, swb_last_error(), (int)(want)); \
      ++g_failures;                                                                                             \
    }                                                                                                           \
  } while (0)
#define EXPECT_OK(expr) EXPECT_RC(SWB_OK, expr)

const int N = 3, S = 2, IMAGE = 16;

enum mode { CACHE, NO_CACHE, NO_COUNTERS };

struct model { int64_t reused = 0, evaluated = 0; };

void expect_stats(swb_handle h, const model& m, const char* when) {
  int64_t reused = -1, evaluated = -1;
  EXPECT_OK(swb_task_stats(h, &reused, &evaluated, nullptr));
  if (reused != m.reused || evaluated != m.evaluated) {
    fprintf(stderr, "%s: reused %lld evaluated %lld, expected %lld / %lld\n", when, (long long)reused, (long long)evaluated,
            (long long)m.reused, (long long)m.evaluated);
    ++g_failures;
  }
}

struct scene {
  std::vector<int32_t> n, shape, base, len;
  std::vector<double> x, y, zero, scale, one;
  std::vector<uint8_t> rgb;
  std::vector<int8_t> label;
  swb_pool pool;
  scene() : n(N, S), shape(N * S, 0), base(N), len(N, 1), x(N * S), y(N * S), zero(N * S, 0.0), scale(N * S, 0.15), one(N * S, 1.0),
            rgb(N * S * 4, 200), label(N * S, 1) {
    for (int e = 0; e < N; ++e) {
      base[e] = e;
      for (int s = 0; s < S; ++s) { x[e * S + s] = 0.3 + 0.1 * e + 0.2 * s; y[e * S + s] = 0.4 + 0.1 * s; }
    }
    memset(&pool, 0, sizeof(pool));
    pool.n_entries = N; pool.n_sprites = n.data(); pool.x = x.data(); pool.y = y.data(); pool.x_vel = zero.data();
    pool.y_vel = zero.data(); pool.scale = scale.data(); pool.cos_a = one.data(); pool.sin_a = zero.data();
    pool.shape = shape.data(); pool.rgb = rgb.data(); pool.label = label.data(); pool.pool_base = base.data();
    pool.pool_len = len.data(); pool.angle = zero.data();
  }
};

swb_handle create(mode m, const scene& sc, bool with_pool) {
  swb_config c;
  memset(&c, 0, sizeof(c));
  c.n_envs = N; c.max_sprites = S; c.image_h = IMAGE; c.image_w = IMAGE; c.anti_aliasing = 2;
  c.action_space = SWB_ACTION_SELECT_MOVE; c.action_scale = 0.5; c.keep_in_frame = 1;
  c.max_episode_length = 1000;
  c.n_tasks = 1;
  c.tasks[0].kind = SWB_TASK_FIND_GOAL;
  c.tasks[0].goal_position[0] = c.tasks[0].goal_position[1] = 3.0;      // (out of reach: no episode ends)
  c.tasks[0].terminate_distance = 0.01;
  c.tasks[0].weights_dimensions[0] = c.tasks[0].weights_dimensions[1] = 1.0;
  c.tasks[0].raw_reward_multiplier = 1.0;
  if (m != NO_COUNTERS) setenv("SWB_LIST_STATS", "1", 1);
  if (m == NO_CACHE) setenv("SWB_NO_TASK_CACHE", "1", 1);
  swb_handle h = nullptr;
  EXPECT_OK(swb_create(&c, 0, &h));
  unsetenv("SWB_LIST_STATS");                           // (both are read at swb_create)
  unsetenv("SWB_NO_TASK_CACHE");
  if (!h) return nullptr;
  const double verts[6] = {-0.5, -0.4, 0.5, -0.4, 0.0, 0.6};
  const int32_t offsets[2] = {0, 3};
  EXPECT_OK(swb_upload_shapes(h, verts, offsets, 1));
  std::vector<int32_t> bounds(2 * IMAGE), coeffs(2 * IMAGE, 1 << 21);     // anti_aliasing = 2: box tables (no pixel is compared)
  for (int o = 0; o < IMAGE; ++o) { bounds[2 * o] = 2 * o; bounds[2 * o + 1] = 2; }
  EXPECT_OK(swb_upload_resample(h, 0, IMAGE, 2, bounds.data(), coeffs.data()));
  EXPECT_OK(swb_upload_resample(h, 1, IMAGE, 2, bounds.data(), coeffs.data()));
  if (with_pool) EXPECT_OK(swb_set_pool(h, &sc.pool));
  return h;
}

void run(mode m) {
  scene sc;
  swb_handle h = create(m, sc, true);
  if (!h) return;
  swb_variant_info info;
  EXPECT_OK(swb_variant(h, &info));
  if (info.task_cache_bytes != (m == NO_CACHE ? 0 : 16 * N)) {
    fprintf(stderr, "task_cache_bytes %lld in mode %d\n", (long long)info.task_cache_bytes, (int)m);
    ++g_failures;
  }
  std::vector<uint8_t> obs((size_t)N * IMAGE * IMAGE * 3), step_type(N), success(N), error(N, 0);
  std::vector<double> reward(N), actions(N * 4), first_reward(N);
  std::vector<float> discount(N);
  for (int e = 0; e < N; ++e) { actions[4 * e] = 0.98; actions[4 * e + 1] = 0.02; actions[4 * e + 2] = 0.6; actions[4 * e + 3] = 0.4; }   // a click no sprite is under
  swb_outputs o;
  o.obs = obs.data(); o.reward = reward.data(); o.discount = discount.data(); o.step_type = step_type.data();
  o.success = success.data(); o.error = error.data();
  model want;
  // a step of handle `g` on which every environment must reuse (cached) or evaluate
  auto step = [&](swb_handle g, bool cached, bool render, const char* what) {
    o.obs = render ? obs.data() : nullptr;
    EXPECT_OK(swb_step(g, actions.data(), &o, nullptr));
    for (int e = 0; e < N; ++e)
      if (error[e]) { fprintf(stderr, "%s: environment %d has error flags %d\n", what, e, error[e]); ++g_failures; }
    if (g != h) return;
    if (cached && m != NO_CACHE) want.reused += N; else want.evaluated += N;
    if (m != NO_COUNTERS) expect_stats(h, want, what);
  };
  if (m == NO_COUNTERS) {                               // no counter without the switch; the cache works all the same
    int64_t a = 0, b = 0;
    step(h, false, true, "the reset step");
    step(h, true, true, "a miss");
    EXPECT_RC(SWB_ERR_STATE, swb_task_stats(h, &a, &b, nullptr));
    EXPECT_OK(swb_destroy(h));
    return;
  }
  step(h, false, true, "the reset step");
  step(h, true, true, "a miss");
  first_reward = reward;
  step(h, true, false, "a miss without a frame");
  step(h, true, true, "a miss after a step without a frame (the list epoch moved, the task epoch did not)");
  for (int e = 0; e < N; ++e)
    if (memcmp(&reward[e], &first_reward[e], sizeof(double)) != 0) { fprintf(stderr, "reward of a reused record differs\n"); ++g_failures; }
  // ---- calls that move the task epoch: the miss after each evaluates
  EXPECT_OK(swb_set_positions(h, sc.x.data(), sc.y.data(), nullptr));          // (the same positions: the host cannot know)
  step(h, false, true, "a miss after swb_set_positions");
  step(h, true, true, "a miss");
  {                                                     // save, load into the same slots
    std::vector<double> sx(N * S), sy(N * S);
    std::vector<int32_t> sn(N), se(N), ssc(N), sep(N), sb(N), sl(N);
    std::vector<uint8_t> sr(N);
    swb_snapshot snap = {sx.data(), sy.data(), sn.data(), se.data(), ssc.data(), sep.data(), sb.data(), sl.data(), sr.data()};
    EXPECT_OK(swb_save_state(h, SWB_STATE_LIVE, nullptr, N, &snap, nullptr));
    step(h, true, true, "a miss after swb_save_state");
    EXPECT_OK(swb_load_state(h, &snap, N, nullptr, 0, nullptr, nullptr));
    step(h, false, true, "a miss after swb_load_state");
    step(h, true, true, "a miss");
  }
  {                                                     // a second handle takes the pool: its own epoch moves, not this one's
    scene none;
    swb_handle g = create(m, none, false);
    if (g) {
      EXPECT_OK(swb_copy_pool(g, h, sc.base.data(), sc.len.data(), nullptr));
      step(g, false, true, "the reset step of the copy");
      step(h, true, true, "a miss after swb_copy_pool from this handle");
      EXPECT_OK(swb_destroy(g));
    }
  }
  const double verts[6] = {-0.5, -0.4, 0.5, -0.4, 0.0, 0.6};
  const int32_t offsets[2] = {0, 3};
  EXPECT_OK(swb_upload_shapes(h, verts, offsets, 1));
  step(h, false, true, "a miss after swb_upload_shapes");
  step(h, true, true, "a miss");
  EXPECT_OK(swb_set_pool(h, &sc.pool));
  step(h, false, true, "the reset step after swb_set_pool");
  step(h, true, true, "a miss");
  EXPECT_OK(swb_reset_all(h, nullptr));                   // (no epoch: the reset step evaluates by itself)
  step(h, false, true, "the reset step after swb_reset_all");
  step(h, true, true, "a miss");
  // ---- calls that must disturb nothing
  int32_t run_cap = -1;
  EXPECT_OK(swb_trim_run_lists(h, &run_cap, nullptr));
  step(h, true, true, "a miss after swb_trim_run_lists");
  EXPECT_OK(swb_render(h, obs.data(), nullptr));
  EXPECT_OK(swb_evaluate(h, success.data(), nullptr));
  expect_stats(h, want, "after swb_render and swb_evaluate");
  step(h, true, true, "a miss after swb_render and swb_evaluate");
  // ---- a sprite setter (last: snapshots refuse a handle with overrides)
  const int8_t lab = 1;
  EXPECT_OK(swb_set_sprite_attr(h, 1, 0, SWB_ATTR_SCALE, 0.2, nullptr, &lab, nullptr));
  step(h, false, true, "a miss after swb_set_sprite_attr");
  step(h, true, true, "a miss on the override build");
  EXPECT_OK(swb_destroy(h));
}

}  // namespace

int main() {
  run(CACHE);
  run(NO_CACHE);
  run(NO_COUNTERS);
  if (g_failures) { fprintf(stderr, "%d checks failed\n", g_failures); return 1; }
  fprintf(stderr, "ok\n");
  return 0;
}
