// host_split_bands.cc -- drives the C ABI (include/swb.h) of the EMULATED library through the host side of split bands
// (DESIGN.md section 26), for tests/test_host_split_bands.py: create -> steps -> swb_set_positions -> steps -> trim -> steps ->
// swb_render -> destroy, with swb_frame_stats (frames) and swb_split_stats (whole tasks / band tasks / whole copies) held at every
// stage, on a handle in the mode that always splits, on one in the mode that never does, on a handle with the mode switched off
// and on one without the counters.  The caller's frame buffer is filled with 0xA5 before every launch and must hold the scene's
// frame after it.  Built once with -fsanitize=address and once with -fsanitize=undefined together with the host sources.
// "Device" pointers are host memory here (tests/emu/README.md).
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

const int N = 3, S = 2, IMAGE = 16, BANDS = 2;

enum mode { SPLIT_ALWAYS, SPLIT_NEVER, MODE_OFF, NO_STATS };

void run(mode m) {
  swb_config c;
  memset(&c, 0, sizeof(c));
  c.n_envs = N; c.max_sprites = S; c.image_h = IMAGE; c.image_w = IMAGE; c.anti_aliasing = 2;
  c.action_space = SWB_ACTION_SELECT_MOVE; c.action_scale = 0.5; c.keep_in_frame = 1;
  c.max_episode_length = 100;
  c.n_tasks = 1;
  c.tasks[0].kind = SWB_TASK_FIND_GOAL;
  c.tasks[0].goal_position[0] = c.tasks[0].goal_position[1] = 3.0;      // (out of reach: no episode ends)
  c.tasks[0].terminate_distance = 0.01;
  c.tasks[0].weights_dimensions[0] = c.tasks[0].weights_dimensions[1] = 1.0;
  c.tasks[0].raw_reward_multiplier = 1.0;
  if (m != NO_STATS) setenv("SWB_LIST_STATS", "1", 1);
  setenv("SWB_SPLIT_BANDS", m == MODE_OFF ? "0" : "2", 1);
  setenv("SWB_SPLIT_WHEN", m == SPLIT_NEVER ? "0" : "2000000000", 1);
  swb_handle h = nullptr;
  EXPECT_OK(swb_create(&c, 0, &h));
  unsetenv("SWB_LIST_STATS");                           // (all read at swb_create)
  unsetenv("SWB_SPLIT_BANDS");
  unsetenv("SWB_SPLIT_WHEN");
  if (!h) return;
  const double verts[6] = {-0.5, -0.4, 0.5, -0.4, 0.0, 0.6};
  const int32_t offsets[2] = {0, 3};
  EXPECT_OK(swb_upload_shapes(h, verts, offsets, 1));
  std::vector<int32_t> bounds(2 * IMAGE), coeffs(2 * IMAGE, 1 << 21);     // anti_aliasing = 2: box tables
  for (int o = 0; o < IMAGE; ++o) { bounds[2 * o] = 2 * o; bounds[2 * o + 1] = 2; }
  EXPECT_OK(swb_upload_resample(h, 0, IMAGE, 2, bounds.data(), coeffs.data()));
  EXPECT_OK(swb_upload_resample(h, 1, IMAGE, 2, bounds.data(), coeffs.data()));
  std::vector<int32_t> n(N, S), shape(N * S, 0), base(N), len(N, 1);
  std::vector<double> x(N * S), y(N * S), zero(N * S, 0.0), scale(N * S, 0.15), one(N * S, 1.0);
  std::vector<uint8_t> rgb(N * S * 4, 200);
  std::vector<int8_t> label(N * S, 1);
  for (int e = 0; e < N; ++e) {
    base[e] = e;
    for (int s = 0; s < S; ++s) { x[e * S + s] = 0.3 + 0.1 * e + 0.2 * s; y[e * S + s] = 0.4 + 0.1 * s; }
  }
  swb_pool pool;
  memset(&pool, 0, sizeof(pool));
  pool.n_entries = N; pool.n_sprites = n.data(); pool.x = x.data(); pool.y = y.data(); pool.x_vel = zero.data();
  pool.y_vel = zero.data(); pool.scale = scale.data(); pool.cos_a = one.data(); pool.sin_a = zero.data();
  pool.shape = shape.data(); pool.rgb = rgb.data(); pool.label = label.data(); pool.pool_base = base.data();
  pool.pool_len = len.data(); pool.angle = zero.data();
  EXPECT_OK(swb_set_pool(h, &pool));
  swb_variant_info info;
  memset(&info, 0, sizeof(info));
  EXPECT_OK(swb_variant(h, &info));
  if (info.split_bands != (m == MODE_OFF ? 0 : BANDS) || (m != MODE_OFF && info.n_bands != 1)) {
    fprintf(stderr, "split_bands %d, n_bands %d in mode %d\n", info.split_bands, info.n_bands, (int)m);
    ++g_failures;
  }
  const int64_t frame_bytes = (int64_t)N * IMAGE * IMAGE * 3;
  std::vector<uint8_t> obs((size_t)frame_bytes), last, step_type(N), success(N), error(N, 0);
  std::vector<double> reward(N), actions(N * 4);
  std::vector<float> discount(N);
  for (int e = 0; e < N; ++e) { actions[4 * e] = 0.98; actions[4 * e + 1] = 0.02; actions[4 * e + 2] = 0.6; actions[4 * e + 3] = 0.4; }   // a click no sprite is under
  swb_outputs o;
  o.obs = obs.data(); o.reward = reward.data(); o.discount = discount.data(); o.step_type = step_type.data();
  o.success = success.data(); o.error = error.data();
  auto check_frame = [&](const char* what, bool same_scene) {
    bool drawn = false;
    for (uint8_t b : obs) drawn = drawn || (b != 0 && b != 0xA5);
    if (!drawn) { fprintf(stderr, "%s: no sprite in the frame\n", what); ++g_failures; }
    if (same_scene && obs != last) { fprintf(stderr, "%s: the frame of an unchanged scene differs from the last one\n", what); ++g_failures; }
    if (!same_scene && !last.empty() && obs == last) { fprintf(stderr, "%s: the frame of a changed scene is the last one\n", what); ++g_failures; }
    last = obs;
  };
  auto step = [&](const char* what, bool same_scene) {
    memset(obs.data(), 0xA5, obs.size());
    EXPECT_OK(swb_step(h, actions.data(), &o, nullptr));
    for (int e = 0; e < N; ++e)
      if (error[e]) { fprintf(stderr, "%s: environment %d has error flags %d\n", what, e, error[e]); ++g_failures; }
    check_frame(what, same_scene);
  };
  int64_t a = 0, b = 0, d = 0;
  if (m == NO_STATS) {                                  // no counter without the switch; the mode works all the same
    step("the reset step", false); step("a miss", true); step("a miss", true);
    EXPECT_RC(SWB_ERR_STATE, swb_split_stats(h, &a, &b, &d, nullptr));
    EXPECT_RC(SWB_ERR_STATE, swb_frame_stats(h, &a, &b, &d, nullptr));
    EXPECT_OK(swb_destroy(h));
    return;
  }
  // frames per launch (swb_frame_stats counts frames in the mode), and the tasks a frame that resamples or fills is
  int64_t T = (int64_t)N * info.n_bands * info.n_column_groups;
  int64_t copied = 0, filled = 0, resampled = 0, whole = 0, bands = 0, whole_copies = 0;
  // launches that copied / filled / resampled since the last call
  auto expect = [&](int c_, int f_, int r_, const char* when) {
    copied += c_ * T; filled += f_ * T; resampled += r_ * T;
    EXPECT_OK(swb_frame_stats(h, &a, &b, &d, nullptr));
    if (a != copied || b != filled || d != resampled) {
      fprintf(stderr, "%s (mode %d): copied %lld filled %lld resampled %lld, expected %lld / %lld / %lld\n", when, (int)m, (long long)a,
              (long long)b, (long long)d, (long long)copied, (long long)filled, (long long)resampled);
      ++g_failures;
    }
    if (m == MODE_OFF) {
      EXPECT_RC(SWB_ERR_STATE, swb_split_stats(h, &a, &b, &d, nullptr));
      return;
    }
    EXPECT_OK(swb_variant(h, &info));                   // (after a launch: the bands placed)
    whole_copies += c_ * T;
    if (m == SPLIT_ALWAYS) bands += (int64_t)(f_ + r_) * T * info.split_bands;
    else whole += (int64_t)(f_ + r_) * T;
    EXPECT_OK(swb_split_stats(h, &a, &b, &d, nullptr));
    if (a != whole || b != bands || d != whole_copies) {
      fprintf(stderr, "%s (mode %d): whole %lld bands %lld whole copies %lld, expected %lld / %lld / %lld\n", when, (int)m, (long long)a,
              (long long)b, (long long)d, (long long)whole, (long long)bands, (long long)whole_copies);
      ++g_failures;
    }
  };
  step("the reset step", false);
  expect(0, 0, 1, "after the reset step");
  if (m != MODE_OFF && info.split_bands != BANDS) { fprintf(stderr, "%d bands placed\n", info.split_bands); ++g_failures; }
  step("a miss", true);
  expect(0, 1, 0, "after the first miss");
  step("a miss", true); step("a miss", true);
  expect(2, 0, 0, "after three misses");
  for (int i = 0; i < N * S; ++i) y[i] += 0.2;            // a setter: every list, and with it every cached frame, is stale
  EXPECT_OK(swb_set_positions(h, x.data(), y.data(), nullptr));
  step("a miss after swb_set_positions", false);
  expect(0, 0, 1, "after the setter");
  step("a miss", true); step("a miss", true);
  expect(1, 1, 0, "two misses after the setter");
  int32_t run_cap = -1;
  EXPECT_OK(swb_trim_run_lists(h, &run_cap, nullptr));   // the lists move: stale again
  EXPECT_OK(swb_variant(h, &info));
  T = (int64_t)N * info.n_bands * info.n_column_groups;
  step("a miss on trimmed lists", true);
  expect(0, 0, 1, "after the trim");
  step("a miss", true);
  expect(0, 1, 0, "a miss after the trim");
  memset(obs.data(), 0xA5, obs.size());
  EXPECT_OK(swb_render(h, obs.data(), nullptr));
  check_frame("a render of the unchanged state", true);
  expect(1, 0, 0, "after a render that copied");
  EXPECT_OK(swb_destroy(h));
}

}  // namespace

int main() {
  run(SPLIT_ALWAYS);
  run(SPLIT_NEVER);
  run(MODE_OFF);
  run(NO_STATS);
  if (g_failures) { fprintf(stderr, "%d checks failed\n", g_failures); return 1; }
  fprintf(stderr, "ok\n");
  return 0;
}
