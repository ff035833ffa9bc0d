// host_lifecycle.cc -- drives the C ABI (include/swb.h) of the EMULATED library through the life of a handle, for
// tests/test_host_lifecycle.py: built with -fsanitize=address together with the host sources, it shows that every device
// buffer a handle makes, re-makes or half-makes is freed exactly once.  "Device" pointers are host memory here
// (tests/emu/README.md).  Every return code and every error flag byte is checked; nothing is asserted about pixels.
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

const int N = 3;

swb_config make_config(int sprites, int image, int aa) {
  swb_config c;
  memset(&c, 0, sizeof(c));
  c.n_envs = N; c.max_sprites = sprites; c.image_h = image; c.image_w = image; c.anti_aliasing = aa;
  c.action_space = SWB_ACTION_SELECT_MOVE; c.action_scale = 0.5; c.keep_in_frame = 1;
  c.max_episode_length = 100;            // (no episode ends inside a lifecycle: the setter needs a live one)
  c.n_tasks = 1;
  c.tasks[0].kind = SWB_TASK_FIND_GOAL;
  c.tasks[0].goal_position[0] = c.tasks[0].goal_position[1] = 0.5;
  c.tasks[0].weights_dimensions[0] = c.tasks[0].weights_dimensions[1] = 1.0;
  c.tasks[0].raw_reward_multiplier = 1.0;
  return c;
}

// One pool entry per environment, every entry `S` small triangles spread over the frame.
struct pool_data {
  std::vector<int32_t> n, shape, base, len;
  std::vector<double> x, y, zero, scale, one, angle;
  std::vector<uint8_t> rgb;
  std::vector<int8_t> label;
  swb_pool pool;
  explicit pool_data(int S) : n(N, S), shape(N * S, 0), base(N), len(N, 1), x(N * S), y(N * S), zero(N * S, 0.0),
                              scale(N * S, 0.15), one(N * S, 1.0), angle(N * S, 0.0), rgb(N * S * 4, 200), label(N * S, 1) {
    for (int e = 0; e < N; ++e) {
      base[e] = e;
      for (int s = 0; s < S; ++s) {
        x[e * S + s] = 0.1 + 0.8 * ((s * 7 + e * 3) % 11) / 10.0;
        y[e * S + s] = 0.1 + 0.8 * ((s * 5 + e) % 9) / 8.0;
      }
    }
    memset(&pool, 0, sizeof(pool));
    pool.n_entries = N; pool.n_sprites = n.data(); pool.x = x.data(); pool.y = y.data(); pool.x_vel = zero.data();
    pool.y_vel = zero.data(); pool.scale = scale.data(); pool.cos_a = one.data(); pool.sin_a = zero.data();
    pool.shape = shape.data(); pool.rgb = rgb.data(); pool.label = label.data(); pool.pool_base = base.data();
    pool.pool_len = len.data(); pool.angle = angle.data();
  }
};

// anti_aliasing = 2: box tables (no pixel is compared): bounds = {2 o, 2}, both coefficients 1 << 21
int upload_box_tables(swb_handle h, int image) {
  std::vector<int32_t> bounds(2 * image), coeffs(2 * image, 1 << 21);
  for (int o = 0; o < image; ++o) { bounds[2 * o] = 2 * o; bounds[2 * o + 1] = 2; }
  if (int rc = swb_upload_resample(h, 0, image, 2, bounds.data(), coeffs.data())) return rc;
  return swb_upload_resample(h, 1, image, 2, bounds.data(), coeffs.data());
}

int upload_triangle(swb_handle h) {
  const double verts[6] = {-0.5, -0.4, 0.5, -0.4, 0.0, 0.6};
  const int32_t offsets[2] = {0, 3};
  return swb_upload_shapes(h, verts, offsets, 1);
}

// The buffers a step writes; check() wants every error flag byte clear.
struct step_buffers {
  std::vector<uint8_t> obs, step_type, success, error;
  std::vector<double> reward, actions;
  std::vector<float> discount;
  explicit step_buffers(int image) : obs((size_t)N * image * image * 3), step_type(N), success(N), error(N, 0), reward(N),
                                     actions(N * 4), discount(N) {
    for (int e = 0; e < N; ++e) { actions[4 * e] = 0.3 + 0.2 * e; actions[4 * e + 1] = 0.5; actions[4 * e + 2] = 0.6; actions[4 * e + 3] = 0.4; }
  }
  swb_outputs outputs(bool with_obs) {
    swb_outputs o;
    o.obs = with_obs ? obs.data() : nullptr; o.reward = reward.data(); o.discount = discount.data();
    o.step_type = step_type.data(); o.success = success.data(); o.error = error.data();
    return o;
  }
  void check(const char* what) {
    for (int e = 0; e < N; ++e)
      if (error[e]) { fprintf(stderr, "%s: environment %d has error flags %d\n", what, e, error[e]); ++g_failures; }
  }
};

int step(swb_handle h, step_buffers& b, bool with_obs, const char* what) {
  const swb_outputs o = b.outputs(with_obs);
  const int rc = swb_step(h, b.actions.data(), &o, nullptr);
  b.check(what);
  return rc;
}

// has_lists: the handle hands run lists to a second kernel (neither a painting cover kernel nor the large-frame path)
void lifecycle(const char* name, int sprites, int image, int aa, bool has_lists, bool timing, const char* env_switch) {
  fprintf(stderr, "handle %s\n", name);
  if (env_switch) setenv(env_switch, "1", 1);
  const swb_config cfg = make_config(sprites, image, aa);
  swb_handle h = nullptr;
  EXPECT_OK(swb_create(&cfg, 0, &h));
  if (env_switch) unsetenv(env_switch);                 // (read at swb_create)
  if (!h) return;
  if (timing) EXPECT_OK(swb_timing_enable(h, 1));
  pool_data pd(sprites);
  step_buffers b(image);
  EXPECT_OK(upload_triangle(h));
  if (aa != 1) EXPECT_OK(upload_box_tables(h, image));
  EXPECT_OK(swb_set_pool(h, &pd.pool));
  for (int i = 0; i < 4; ++i) EXPECT_OK(step(h, b, true, "step with an observation"));
  EXPECT_OK(step(h, b, false, "step without an observation"));
  // the last launch rendered nothing: a handle with run lists has none to measure (SWB_ERR_STATE); the others have nothing to trim
  int32_t run_cap = -1;
  EXPECT_RC(has_lists ? SWB_ERR_STATE : SWB_OK, swb_trim_run_lists(h, &run_cap, nullptr));
  EXPECT_OK(step(h, b, true, "step after the first trim"));
  if (has_lists) {                                      // ... and now it has: the lists are dropped and re-made smaller
    EXPECT_OK(swb_trim_run_lists(h, &run_cap, nullptr));
    EXPECT_OK(step(h, b, true, "step on trimmed lists"));
  }
  EXPECT_OK(swb_render(h, b.obs.data(), nullptr));
  EXPECT_OK(swb_evaluate(h, b.success.data(), nullptr));
  int32_t st[5] = {0, 0, 0, 0, 0};
  EXPECT_OK(swb_get_env_state(h, 1, st, nullptr));
  if (st[0] != sprites) { fprintf(stderr, "environment 1 has %d sprites, expected %d\n", st[0], sprites); ++g_failures; }
  EXPECT_OK(swb_set_sprite_attr(h, 0, 0, SWB_ATTR_SCALE, 0.2, nullptr, nullptr, nullptr));
  EXPECT_OK(step(h, b, true, "step on the override build"));
  EXPECT_OK(swb_set_pool(h, &pd.pool));                 // restores the reservation of the run lists
  EXPECT_OK(step(h, b, true, "step on the second pool"));
  if (timing) {
    double cover = -1.0, resample = -1.0;
    int64_t launches = 0;
    EXPECT_OK(swb_kernel_times_ms(h, &cover, &resample, &launches));
    if (launches < 1) { fprintf(stderr, "timing counted %lld launches\n", (long long)launches); ++g_failures; }
  }
  EXPECT_OK(swb_destroy(h));
}

// Two rollouts on a handle without overrides, the second with more candidates and more steps: both scratch buffers regrow.
void rollouts() {
  fprintf(stderr, "rollouts\n");
  const int S = 2, image = 16;
  const swb_config cfg = make_config(S, image, 2);
  swb_handle h = nullptr;
  EXPECT_OK(swb_create(&cfg, 0, &h));
  if (!h) return;
  pool_data pd(S);
  step_buffers b(image);
  EXPECT_OK(upload_triangle(h));
  EXPECT_OK(upload_box_tables(h, image));
  EXPECT_OK(swb_set_pool(h, &pd.pool));
  EXPECT_OK(step(h, b, true, "step before the rollouts"));
  const int MK[2][2] = {{2, 2}, {3, 4}};
  for (const auto& mk : MK) {
    const int M = mk[0], K = mk[1];
    const size_t knm = (size_t)K * N * M, nm = (size_t)N * M;
    std::vector<double> actions(knm * 4), reward(knm), x(nm * S), y(nm * S);
    std::vector<float> discount(knm);
    std::vector<uint8_t> step_type(knm), success(knm), error(nm, 0);
    std::vector<int32_t> n_sprites(nm);
    for (size_t i = 0; i < knm; ++i) { actions[4 * i] = 0.1 * (i % 10); actions[4 * i + 1] = 0.5; actions[4 * i + 2] = 0.7; actions[4 * i + 3] = 0.2; }
    swb_rollout_outputs o;
    o.reward = reward.data(); o.discount = discount.data(); o.step_type = step_type.data(); o.success = success.data();
    o.error = error.data(); o.x = x.data(); o.y = y.data(); o.n_sprites = n_sprites.data();
    EXPECT_OK(swb_rollout(h, actions.data(), M, K, &o, nullptr));
    for (size_t i = 0; i < nm; ++i)
      if (error[i]) { fprintf(stderr, "rollout M = %d, K = %d: candidate %zu has error flags %d\n", M, K, i, error[i]); ++g_failures; }
    for (size_t i = 0; i < nm; ++i)
      if (n_sprites[i] != S) { fprintf(stderr, "rollout M = %d, K = %d: candidate %zu ends with %d sprites\n", M, K, i, n_sprites[i]); ++g_failures; }
  }
  EXPECT_OK(swb_destroy(h));
}

// Calls that refuse after part of the set-up has been made.
void refusals() {
  fprintf(stderr, "refusals\n");
  swb_handle h = nullptr;
  swb_config cfg = make_config(2, 16, 1);
  cfg.tasks[0].n_xcuts = 2; cfg.tasks[0].xcuts[0] = 0.6; cfg.tasks[0].xcuts[1] = 0.4;          // descending
  EXPECT_RC(SWB_ERR_INVALID, swb_create(&cfg, 0, &h));
  cfg = make_config(2, 1024, 5);                                                              // a canvas of 5120 px
  EXPECT_RC(SWB_ERR_INVALID, swb_create(&cfg, 0, &h));
  if (h) { fprintf(stderr, "a refused swb_create returned a handle\n"); ++g_failures; return; }
  cfg = make_config(2, 16, 1);
  cfg.tasks[0].n_xcuts = 1; cfg.tasks[0].xcuts[0] = 0.5;                                      // the task keys on position
  EXPECT_OK(swb_create(&cfg, 0, &h));
  if (!h) return;
  pool_data pd(2);                                                                            // (cell_label = NULL)
  EXPECT_OK(upload_triangle(h));
  EXPECT_RC(SWB_ERR_INVALID, swb_set_pool(h, &pd.pool));
  EXPECT_OK(swb_destroy(h));
}

}  // namespace

int main() {
  lifecycle("1: the cover kernel paints", 2, 16, 1, false, false, nullptr);
  lifecycle("2: resample kernel", 2, 16, 2, true, false, nullptr);
  lifecycle("3: two column groups", 2, 80, 2, true, false, nullptr);
  lifecycle("4: large-frame path", 2, 16, 2, false, false, "SWB_LARGE_FRAMES");
  lifecycle("5: many-sprite path", 20, 16, 1, false, false, nullptr);
  lifecycle("6: timing", 2, 16, 2, true, true, nullptr);
  rollouts();
  refusals();
  if (g_failures) { fprintf(stderr, "%d checks failed\n", g_failures); return 1; }
  fprintf(stderr, "ok\n");
  return 0;
}
