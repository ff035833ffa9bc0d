// host_snapshot_lifecycle.cc -- drives the snapshot calls of the C ABI (include/swb.h: swb_pool_id, swb_save_state, swb_load_state,
// swb_copy_pool) on the EMULATED library through the life of two handles, for tests/test_host_snapshot_lifecycle.py: built with
// -fsanitize=address together with the host sources, it shows that the pool arrays swb_copy_pool makes, swaps in and half-makes
// are each freed exactly once, whichever handle goes first.  "Device" pointers are host memory here (tests/emu/README.md).
// Every return code and every error flag byte is checked; nothing is asserted about pixels.
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
#define EXPECT_TRUE(cond)                                                                    \
  do {                                                                                       \
    if (!(cond)) { fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); ++g_failures; } \
  } while (0)

const int S = 2, IMAGE = 16;

swb_config make_config(int n_envs, int sprites) {
  swb_config c;
  memset(&c, 0, sizeof(c));
  c.n_envs = n_envs; c.max_sprites = sprites; c.image_h = IMAGE; c.image_w = IMAGE; c.anti_aliasing = 2;
  c.action_space = SWB_ACTION_SELECT_MOVE; c.action_scale = 0.5; c.keep_in_frame = 1;
  c.max_episode_length = 3;              // (episodes end inside the run: a loaded environment resets through its source's entries)
  c.n_tasks = 1;
  c.tasks[0].kind = SWB_TASK_FIND_GOAL;
  c.tasks[0].goal_position[0] = c.tasks[0].goal_position[1] = 0.5;
  c.tasks[0].weights_dimensions[0] = c.tasks[0].weights_dimensions[1] = 1.0;
  c.tasks[0].raw_reward_multiplier = 1.0;
  return c;
}

// Two pool entries per environment, every entry S small triangles spread over the frame.
struct pool_data {
  int P;
  std::vector<int32_t> n, shape, base, len;
  std::vector<double> x, y, zero, scale, one, angle;
  std::vector<uint8_t> rgb;
  std::vector<int8_t> label;
  swb_pool pool;
  explicit pool_data(int n_envs) : P(2 * n_envs), n(P, S), shape(P * S, 0), base(n_envs), len(n_envs, 2), x(P * S), y(P * S),
                                   zero(P * S, 0.0), scale(P * S, 0.15), one(P * S, 1.0), angle(P * S, 0.0), rgb(P * S * 4, 200),
                                   label(P * S, 1) {
    for (int e = 0; e < n_envs; ++e) base[e] = 2 * e;
    for (int e = 0; e < P; ++e)
      for (int s = 0; s < S; ++s) {
        x[e * S + s] = 0.1 + 0.8 * ((s * 7 + e * 3) % 11) / 10.0;
        y[e * S + s] = 0.1 + 0.8 * ((s * 5 + e) % 9) / 8.0;
      }
    memset(&pool, 0, sizeof(pool));
    pool.n_entries = P; pool.n_sprites = n.data(); pool.x = x.data(); pool.y = y.data(); pool.x_vel = zero.data();
    pool.y_vel = zero.data(); pool.scale = scale.data(); pool.cos_a = one.data(); pool.sin_a = zero.data();
    pool.shape = shape.data(); pool.rgb = rgb.data(); pool.label = label.data(); pool.pool_base = base.data();
    pool.pool_len = len.data(); pool.angle = angle.data();
  }
};

int upload_tables(swb_handle h) {
  const double verts[6] = {-0.5, -0.4, 0.5, -0.4, 0.0, 0.6};
  const int32_t offsets[2] = {0, 3};
  if (int rc = swb_upload_shapes(h, verts, offsets, 1)) return rc;
  std::vector<int32_t> bounds(2 * IMAGE), coeffs(2 * IMAGE, 1 << 21);      // box tables (no pixel is compared)
  for (int o = 0; o < IMAGE; ++o) { bounds[2 * o] = 2 * o; bounds[2 * o + 1] = 2; }
  if (int rc = swb_upload_resample(h, 0, IMAGE, 2, bounds.data(), coeffs.data())) return rc;
  return swb_upload_resample(h, 1, IMAGE, 2, bounds.data(), coeffs.data());
}

struct step_buffers {
  int n_envs;
  std::vector<uint8_t> obs, step_type, success, error;
  std::vector<double> reward, actions;
  std::vector<float> discount;
  explicit step_buffers(int n) : n_envs(n), obs((size_t)n * IMAGE * IMAGE * 3), step_type(n), success(n), error(n, 0), reward(n),
                                 actions(n * 4), discount(n) {
    for (int e = 0; e < n; ++e) { actions[4 * e] = 0.3 + 0.1 * (e % 5); actions[4 * e + 1] = 0.5; actions[4 * e + 2] = 0.6; actions[4 * e + 3] = 0.4; }
  }
  int step(swb_handle h, const char* what) {
    swb_outputs o;
    o.obs = obs.data(); o.reward = reward.data(); o.discount = discount.data();
    o.step_type = step_type.data(); o.success = success.data(); o.error = error.data();
    const int rc = swb_step(h, actions.data(), &o, nullptr);
    for (int e = 0; e < n_envs; ++e)
      if (error[e]) { fprintf(stderr, "%s: environment %d has error flags %d\n", what, e, error[e]); ++g_failures; }
    return rc;
  }
};

// A caller's snapshot of C slots.
struct snapshot_block {
  std::vector<double> x, y;
  std::vector<int32_t> n, entry, count, episode, base, len;
  std::vector<uint8_t> reset;
  swb_snapshot snap;
  explicit snapshot_block(int C) : x((size_t)C * S), y((size_t)C * S), n(C), entry(C), count(C), episode(C), base(C), len(C, 1), reset(C, 1) {
    snap.x = x.data(); snap.y = y.data(); snap.n_sprites = n.data(); snap.pool_entry = entry.data(); snap.step_count = count.data();
    snap.episode = episode.data(); snap.pool_base = base.data(); snap.pool_len = len.data(); snap.reset_next = reset.data();
  }
};

struct host_state {
  std::vector<double> x, y;
  std::vector<int32_t> n, entry, count, episode;
  std::vector<uint8_t> reset;
  explicit host_state(swb_handle h, int n_envs) : x((size_t)n_envs * S), y((size_t)n_envs * S), n(n_envs), entry(n_envs), count(n_envs),
                                                  episode(n_envs), reset(n_envs) {
    swb_state st;
    st.x = x.data(); st.y = y.data(); st.n_sprites = n.data(); st.pool_entry = entry.data(); st.step_count = count.data();
    st.reset_next = reset.data(); st.episode = episode.data();
    EXPECT_OK(swb_get_state(h, &st, nullptr));
  }
};

void two_handles(bool destroy_source_first) {
  fprintf(stderr, "two handles, the %s destroyed first\n", destroy_source_first ? "source" : "copy");
  const int NA = 3, NB = 6;
  const swb_config cfg_a = make_config(NA, S), cfg_b = make_config(NB, S);
  swb_handle a = nullptr, b = nullptr;
  EXPECT_OK(swb_create(&cfg_a, 0, &a));
  EXPECT_OK(swb_create(&cfg_b, 0, &b));
  if (!a || !b) return;
  pool_data pa(NA), pb(NB);
  step_buffers ba(NA), bb(NB);
  EXPECT_OK(upload_tables(a));
  EXPECT_OK(upload_tables(b));
  EXPECT_OK(swb_set_pool(a, &pa.pool));
  uint64_t id_a = 0, id_b = 7;
  EXPECT_OK(swb_pool_id(a, &id_a));
  EXPECT_OK(swb_pool_id(b, &id_b));
  EXPECT_TRUE(id_a != 0 && id_b == 0);
  for (int i = 0; i < 3; ++i) EXPECT_OK(ba.step(a, "a before the copy"));

  // a -> b: every environment of b plays the range of environment n / 2 of a, in its state
  std::vector<int32_t> base_b(NB), len_b(NB, 2), slot_b(NB);
  for (int n = 0; n < NB; ++n) { base_b[n] = 2 * (n / 2); slot_b[n] = n / 2; }
  // ... but first a copy that fails half-way: b keeps what it had (nothing), and nothing leaks
  setenv("SWB_COPY_POOL_FAIL_AT", "5", 1);
  EXPECT_RC(SWB_ERR_HIP, swb_copy_pool(b, a, base_b.data(), len_b.data(), nullptr));
  unsetenv("SWB_COPY_POOL_FAIL_AT");
  EXPECT_OK(swb_pool_id(b, &id_b));
  EXPECT_TRUE(id_b == 0);
  EXPECT_RC(SWB_ERR_STATE, bb.step(b, "b without a pool"));
  EXPECT_OK(swb_copy_pool(b, a, base_b.data(), len_b.data(), nullptr));
  EXPECT_OK(swb_pool_id(b, &id_b));
  EXPECT_TRUE(id_b == id_a);
  snapshot_block sa(NA);
  EXPECT_OK(swb_save_state(a, SWB_STATE_LIVE, nullptr, NA, &sa.snap, nullptr));
  int32_t rejected = 0;
  EXPECT_OK(swb_load_state(b, &sa.snap, NA, slot_b.data(), id_a, &rejected, nullptr));
  EXPECT_TRUE(rejected == 0);
  {
    const host_state ha(a, NA), hb(b, NB);
    for (int n = 0; n < NB; ++n)
      EXPECT_TRUE(hb.entry[n] == ha.entry[n / 2] && hb.count[n] == ha.count[n / 2] && hb.episode[n] == ha.episode[n / 2] &&
                  hb.reset[n] == ha.reset[n / 2] && hb.x[n * S] == ha.x[(n / 2) * S] && hb.y[n * S + 1] == ha.y[(n / 2) * S + 1]);
  }
  for (int i = 0; i < 5; ++i) EXPECT_OK(bb.step(b, "b on the copied pool"));
  for (int i = 0; i < 2; ++i) EXPECT_OK(ba.step(a, "a after the copy"));

  // a second copy over a pool that is there: the old arrays are freed, once; a failure half-way now keeps the pool b has
  setenv("SWB_COPY_POOL_FAIL_AT", "0", 1);
  EXPECT_RC(SWB_ERR_HIP, swb_copy_pool(b, a, base_b.data(), len_b.data(), nullptr));
  setenv("SWB_COPY_POOL_FAIL_AT", "11", 1);
  EXPECT_RC(SWB_ERR_HIP, swb_copy_pool(b, a, base_b.data(), len_b.data(), nullptr));
  unsetenv("SWB_COPY_POOL_FAIL_AT");
  EXPECT_OK(bb.step(b, "b after the failed copies"));
  EXPECT_OK(swb_copy_pool(b, a, base_b.data(), len_b.data(), nullptr));
  EXPECT_OK(bb.step(b, "b on the second copy"));

  // the other way: b gets a pool of its own (a new id), a takes it over; a snapshot of the old pool is refused, one of b's is not
  EXPECT_OK(swb_set_pool(b, &pb.pool));
  EXPECT_OK(swb_pool_id(b, &id_b));
  EXPECT_TRUE(id_b != 0 && id_b != id_a);
  for (int i = 0; i < 2; ++i) EXPECT_OK(bb.step(b, "b on its own pool"));
  std::vector<int32_t> base_a(NA), len_a(NA, 2), index_a(NA), slot_a(NA);
  for (int n = 0; n < NA; ++n) { base_a[n] = 2 * (NB - 1 - n); index_a[n] = NB - 1 - n; slot_a[n] = n; }
  slot_a[1] = -1;
  EXPECT_OK(swb_copy_pool(a, b, base_a.data(), len_a.data(), nullptr));
  EXPECT_RC(SWB_ERR_STATE, swb_load_state(a, &sa.snap, NA, nullptr, id_a, nullptr, nullptr));
  snapshot_block sb(NA);
  EXPECT_OK(swb_save_state(b, SWB_STATE_LIVE, index_a.data(), NA, &sb.snap, nullptr));
  slot_a[2] = NA + 4;                                  // (out of range: left alone, counted)
  EXPECT_OK(swb_load_state(a, &sb.snap, NA, slot_a.data(), id_b, &rejected, nullptr));
  EXPECT_TRUE(rejected == 1);
  for (int i = 0; i < 5; ++i) EXPECT_OK(ba.step(a, "a on b's pool"));
  EXPECT_RC(SWB_ERR_INVALID, swb_copy_pool(a, a, base_a.data(), len_a.data(), nullptr));

  if (destroy_source_first) { EXPECT_OK(swb_destroy(b)); EXPECT_OK(ba.step(a, "a after b is gone")); EXPECT_OK(swb_destroy(a)); }
  else { EXPECT_OK(swb_destroy(a)); EXPECT_OK(bb.step(b, "b after a is gone")); EXPECT_OK(swb_destroy(b)); }
}

// End states of a rollout saved and adopted; refusals that return before anything is made.
void rollout_states_and_refusals() {
  fprintf(stderr, "rollout end states, refusals\n");
  const int NA = 3, M = 2, K = 4;
  const swb_config cfg = make_config(NA, S);
  swb_config other = make_config(NA, S + 1);
  swb_handle a = nullptr, c = nullptr;
  EXPECT_OK(swb_create(&cfg, 0, &a));
  EXPECT_OK(swb_create(&other, 0, &c));
  if (!a || !c) return;
  pool_data pa(NA);
  step_buffers ba(NA);
  EXPECT_OK(upload_tables(a));
  snapshot_block all(NA * M), one(NA);
  EXPECT_RC(SWB_ERR_STATE, swb_save_state(a, SWB_STATE_LIVE, nullptr, NA, &one.snap, nullptr));            // no pool
  EXPECT_OK(swb_set_pool(a, &pa.pool));
  EXPECT_OK(ba.step(a, "a before the rollout"));
  EXPECT_RC(SWB_ERR_STATE, swb_save_state(a, SWB_STATE_ROLLOUT_END, nullptr, NA * M, &all.snap, nullptr));  // no rollout
  std::vector<double> actions((size_t)K * NA * M * 4, 0.4);
  EXPECT_OK(swb_rollout(a, actions.data(), M, K, nullptr, nullptr));
  EXPECT_OK(swb_save_state(a, SWB_STATE_ROLLOUT_END, nullptr, NA * M, &all.snap, nullptr));
  const int32_t pick[3] = {1, 2, 5};
  EXPECT_OK(swb_save_state(a, SWB_STATE_ROLLOUT_END, pick, NA, &one.snap, nullptr));
  for (int n = 0; n < NA; ++n) EXPECT_TRUE(one.episode[n] == all.episode[pick[n]] && one.x[n * S] == all.x[pick[n] * S] && one.episode[n] >= 1);
  uint64_t id = 0;
  EXPECT_OK(swb_pool_id(a, &id));
  EXPECT_OK(swb_load_state(a, &one.snap, NA, nullptr, id, nullptr, nullptr));
  for (int i = 0; i < 3; ++i) EXPECT_OK(ba.step(a, "a on the adopted end states"));
  EXPECT_RC(SWB_ERR_INVALID, swb_save_state(a, 5, nullptr, NA, &one.snap, nullptr));
  EXPECT_RC(SWB_ERR_INVALID, swb_load_state(a, &one.snap, NA + 1, nullptr, 0, nullptr, nullptr));
  EXPECT_RC(SWB_ERR_INVALID, swb_copy_pool(c, a, pa.base.data(), pa.len.data(), nullptr));                 // unlike handles
  swb_handle d = nullptr;                                                                                  // like a, without a pool
  EXPECT_OK(swb_create(&cfg, 0, &d));
  EXPECT_RC(SWB_ERR_STATE, swb_copy_pool(a, d, pa.base.data(), pa.len.data(), nullptr));
  EXPECT_OK(swb_destroy(d));
  EXPECT_OK(swb_set_pool(a, &pa.pool));
  EXPECT_RC(SWB_ERR_STATE, swb_save_state(a, SWB_STATE_ROLLOUT_END, nullptr, NA * M, &all.snap, nullptr));  // a stale pool
  EXPECT_OK(swb_destroy(c));
  EXPECT_OK(swb_destroy(a));
}

}  // namespace

int main() {
  two_handles(true);
  two_handles(false);
  rollout_states_and_refusals();
  if (g_failures) { fprintf(stderr, "%d checks failed\n", g_failures); return 1; }
  fprintf(stderr, "ok\n");
  return 0;
}
