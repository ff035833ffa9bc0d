// host_spec_copy.cc -- drives the C ABI (include/swb.h) of the EMULATED library through the host side of the speculative copies
// of the cover launch, for tests/test_host_spec_copy.py: create -> steps -> swb_set_positions -> steps ->
// trim -> steps -> swb_render -> destroy under SWB_SPEC_COPY=first and =behind, with swb_frame_stats (the parent's counts) and
// swb_spec_copy_stats (the copy workgroups that copied: the emulator runs workgroups in index order, so the count is exact) held
// at every stage, and a refusal of any other value of the switch.  The caller's frame buffer is filled with 0xA5 before every
// launch and must hold the scene's frame after it.  Built once with -fsanitize=address and once with -fsanitize=undefined
// together with the host sources.  "Device" pointers are host memory here (tests/emu/README.md).
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

swb_config config() {
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
  return c;
}

void refused() {
  swb_config c = config();
  setenv("SWB_SPEC_COPY", "sometimes", 1);
  swb_handle h = nullptr;
  EXPECT_RC(SWB_ERR_INVALID, swb_create(&c, 0, &h));
  unsetenv("SWB_SPEC_COPY");
  if (h) { fprintf(stderr, "a handle came back from a refused swb_create\n"); ++g_failures; }
}

void run(bool first) {
  swb_config c = config();
  setenv("SWB_LIST_STATS", "1", 1);
  setenv("SWB_SPLIT_BANDS", "0", 1);
  setenv("SWB_SPEC_COPY", first ? "first" : "behind", 1);
  swb_handle h = nullptr;
  EXPECT_OK(swb_create(&c, 0, &h));
  unsetenv("SWB_LIST_STATS");                           // (all read at swb_create)
  unsetenv("SWB_SPLIT_BANDS");
  unsetenv("SWB_SPEC_COPY");
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
  if (info.frame_cache_bytes != (int64_t)N * IMAGE * IMAGE * 3) { fprintf(stderr, "no frame cache\n"); ++g_failures; }
  const int64_t frame_bytes = (int64_t)N * IMAGE * IMAGE * 3;
  // two buffers of the caller's take turns
  std::vector<uint8_t> obs_a((size_t)frame_bytes), obs_b((size_t)frame_bytes), last, step_type(N), success(N), error(N, 0);
  std::vector<double> reward(N), actions(N * 4);
  std::vector<float> discount(N);
  for (int e = 0; e < N; ++e) { actions[4 * e] = 0.98; actions[4 * e + 1] = 0.02; actions[4 * e + 2] = 0.6; actions[4 * e + 3] = 0.4; }   // a click no sprite is under
  swb_outputs o;
  o.reward = reward.data(); o.discount = discount.data(); o.step_type = step_type.data();
  o.success = success.data(); o.error = error.data();
  int launches = 0;
  auto check_frame = [&](const std::vector<uint8_t>& obs, const char* what, bool same_scene) {
    bool drawn = false, garbage = false;
    for (uint8_t b : obs) { drawn = drawn || (b != 0 && b != 0xA5); garbage = garbage || b == 0xA5; }
    if (!drawn) { fprintf(stderr, "%s: no sprite in the frame\n", what); ++g_failures; }
    if (garbage) { fprintf(stderr, "%s: bytes of the frame were not written\n", what); ++g_failures; }
    if (same_scene && obs != last) { fprintf(stderr, "%s: the frame of an unchanged scene differs from the last one\n", what); ++g_failures; }
    if (!same_scene && !last.empty() && obs == last) { fprintf(stderr, "%s: the frame of a changed scene is the last one\n", what); ++g_failures; }
    last = obs;
  };
  auto step = [&](const char* what, bool same_scene) {
    std::vector<uint8_t>& obs = (launches++ & 1) ? obs_b : obs_a;
    memset(obs.data(), 0xA5, obs.size());
    o.obs = obs.data();
    EXPECT_OK(swb_step(h, actions.data(), &o, nullptr));
    for (int e = 0; e < N; ++e)
      if (error[e]) { fprintf(stderr, "%s: environment %d has error flags %d\n", what, e, error[e]); ++g_failures; }
    check_frame(obs, what, same_scene);
  };
  int64_t T = (int64_t)N * info.n_bands * info.n_column_groups;
  const int64_t G = (int64_t)N * info.n_column_groups;     // copy workgroups of a launch
  int64_t copied = 0, filled = 0, resampled = 0, groups = 0, a = 0, b = 0, d = 0;
  // launches that copied / filled / resampled since the last call, and the launches whose copy workgroups copied: with `first`
  // those whose environments came with a word other than 0, with `behind` those whose environments left with one
  auto expect = [&](int c_, int f_, int r_, int g_first, int g_behind, const char* when) {
    copied += c_ * T; filled += f_ * T; resampled += r_ * T;
    groups += (first ? g_first : g_behind) * G;
    EXPECT_OK(swb_frame_stats(h, &a, &b, &d, nullptr));
    if (a != copied || b != filled || d != resampled) {
      fprintf(stderr, "%s (%s): copied %lld filled %lld resampled %lld, expected %lld / %lld / %lld\n", when, first ? "first" : "behind",
              (long long)a, (long long)b, (long long)d, (long long)copied, (long long)filled, (long long)resampled);
      ++g_failures;
    }
    EXPECT_OK(swb_spec_copy_stats(h, &a, nullptr));
    if (a != groups) {
      fprintf(stderr, "%s (%s): %lld copy workgroups copied, expected %lld\n", when, first ? "first" : "behind", (long long)a, (long long)groups);
      ++g_failures;
    }
  };
  step("the reset step", false);
  expect(0, 0, 1, 0, 0, "after the reset step");
  step("a miss", true);
  expect(0, 1, 0, 0, 1, "after the first miss");
  step("a miss", true); step("a miss", true);
  expect(2, 0, 0, 2, 2, "after three misses");
  for (int i = 0; i < N * S; ++i) y[i] += 0.2;            // a setter: every list, and with it every cached frame, is stale
  EXPECT_OK(swb_set_positions(h, x.data(), y.data(), nullptr));
  step("a miss after swb_set_positions", false);         // (the words still say 2: `first` copies the stale frames, the resample waves overwrite them)
  expect(0, 0, 1, 1, 0, "after the setter");
  step("a miss", true); step("a miss", true);
  expect(1, 1, 0, 1, 2, "two misses after the setter");
  int32_t run_cap = -1;
  EXPECT_OK(swb_trim_run_lists(h, &run_cap, nullptr));   // the lists move and their headers start again: every word 0
  EXPECT_OK(swb_variant(h, &info));
  T = (int64_t)N * info.n_bands * info.n_column_groups;
  step("a miss on trimmed lists", true);
  expect(0, 0, 1, 0, 0, "after the trim");
  step("a miss", true);
  expect(0, 1, 0, 0, 1, "a miss after the trim");
  std::vector<uint8_t>& obs = (launches++ & 1) ? obs_b : obs_a;
  memset(obs.data(), 0xA5, obs.size());
  EXPECT_OK(swb_render(h, obs.data(), nullptr));
  check_frame(obs, "a render of the unchanged state", true);
  expect(1, 0, 0, 1, 1, "after a render that copied");
  EXPECT_OK(swb_destroy(h));
}

}  // namespace

int main() {
  refused();
  run(true);
  run(false);
  if (g_failures) { fprintf(stderr, "%d checks failed\n", g_failures); return 1; }
  fprintf(stderr, "ok\n");
  return 0;
}
