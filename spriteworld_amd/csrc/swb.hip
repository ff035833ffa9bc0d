// swb.hip -- C-ABI host side of the batched Spriteworld engine (see include/swb.h).
//
// Owns the device copies of the constant tables, the reset pool, the live structure-of-arrays
// state and the run lists handed from the cover kernel to the resample / fill kernel; launches the
// two kernels of a step (swb_kernels.hip.inc).
// Built only for gfx950:  hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -shared -fPIC
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "swb_kernels.hip.inc"
#include "swb_pow.hip.inc"
#include "swb_sampler.hip.inc"

// the cover kernels of canvases wider than 320 px are instantiated in swb_wide.hip (other scheduler flags)
extern template __global__ void swb_cover_kernel<20, false>(const swb_params);
extern template __global__ void swb_cover_kernel<20, true>(const swb_params);
// ... and so is every kernel of handles with task sets (swb_cover_sets_kernel), at every width: this unit's code object does
// not know of them
extern template __global__ void swb_cover_sets_kernel<2, false>(const swb_params);
extern template __global__ void swb_cover_sets_kernel<2, true>(const swb_params);
extern template __global__ void swb_cover_sets_kernel<4, false>(const swb_params);
extern template __global__ void swb_cover_sets_kernel<5, false>(const swb_params);
extern template __global__ void swb_cover_sets_kernel<10, false>(const swb_params);
extern template __global__ void swb_cover_sets_kernel<20, false>(const swb_params);

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIP_TRY(expr)                                                                      \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess) return fail(SWB_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

// A device allocation and its owner: freed with the handle that holds it, used wherever a T* is.  It never synchronises: whoever
// re-makes a buffer that work in flight may still use waits for that work first, at the call site.
template <typename T>
struct dev_buf {
  T* ptr = nullptr;
  size_t count = 0;                  // elements allocated
  dev_buf() = default;
  dev_buf(const dev_buf&) = delete;
  dev_buf& operator=(const dev_buf&) = delete;
  ~dev_buf() { release(); }
  operator T*() const { return ptr; }
  void release() {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr; count = 0;
  }
  // a new allocation of n elements (none: one) holding src[0 .. n), or zeros when src is NULL
  int fill(const T* src, size_t n) {
    release();
    if (n == 0) n = 1;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&ptr), n * sizeof(T)));
    count = n;
    if (src) HIP_TRY(hipMemcpy(ptr, src, n * sizeof(T), hipMemcpyHostToDevice));
    else HIP_TRY(hipMemset(ptr, 0, n * sizeof(T)));
    return 0;
  }
  // a new allocation holding the n elements of the device array src, copied device to device on `st`
  int clone(const T* src, size_t n, hipStream_t st) {
    release();
    if (n == 0) n = 1;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&ptr), n * sizeof(T)));
    count = n;
    HIP_TRY(hipMemcpyAsync(ptr, src, n * sizeof(T), hipMemcpyDeviceToDevice, st));
    return 0;
  }
  void swap(dev_buf& o) { std::swap(ptr, o.ptr); std::swap(count, o.count); }
};

// Pool ids (swb_pool_id): one counter for the process, never 0.
std::atomic<uint64_t> g_pool_ids{0};
uint64_t next_pool_id() { return g_pool_ids.fetch_add(1) + 1; }

}  // namespace

struct swb_engine {
  swb_config cfg;
  int device = 0;
  swb_params p;        // device pointers + config, passed by value to the kernel
  bool have_shapes = false, have_h = false, have_v = false, have_pool = false;
  int vslots = SWB_VSLOTS;
  int nbands = 1;                    // bands of output rows per (environment, column group) in the resample / fill kernel
  bool tables_dirty = true;          // band / break / column-group tables follow the resampling tables and nbands
  std::vector<int32_t> v_ymin_host, v_end_host, h_xmin_host, h_cnt_host;
  std::vector<int> shape_nverts;     // vertices per uploaded shape
  int ovf_lds_bytes = 0;             // LDS footprint the overflow slots were sized with
  void (*ovf_fn)(const swb_params) = nullptr;   // ... and the cover kernel (plain or override build)
  size_t lds_block = 0;
  // owned device buffers (dev_buf: freed with the handle)
  dev_buf<double> d_shape_verts, d_shape_dmin;
  dev_buf<int32_t> d_shape_off;
  dev_buf<int32_t> d_h_xmin, d_h_cnt, d_h_tbl, d_h_pfx;
  dev_buf<int32_t> d_v_tab, d_v_end, d_v_pfx;
  dev_buf<int32_t> d_p_n;
  dev_buf<double> d_p_x, d_p_y, d_p_xv, d_p_yv, d_p_scale, d_p_ca, d_p_sa;
  dev_buf<int32_t> d_p_shape;
  dev_buf<uint32_t> d_p_rgb;
  dev_buf<int8_t> d_p_label;
  dev_buf<int8_t> d_p_cell_label;    // swb_pool::cell_label (tasks that key on position)
  bool keyed = false;                // some task's filter keys on position (swb_task::n_xcuts / n_ycuts)
  dev_buf<uint8_t> d_p_attr;         // swb_pool::attr_f32
  dev_buf<int32_t> d_pool_base, d_pool_len;
  dev_buf<double> d_p_angle, d_p_color;
  dev_buf<swb_sampler> d_sampler;
  int pool_entries = 0;
  uint64_t pool_id = 0;              // swb_pool_id: renewed by every call that installs or redraws the pool (0: no pool yet)
  bool pool_sampled = false, pool_uniform = false;   // pool came from swb_sample_pool / env-major fixed-length layout
  // swb_sample_pool_tree: the spec with the handle's position grids, the sprites that ran out of tries, and whether the tree
  // kernel filled the pool last (swb_resample_pool redraws with it)
  dev_buf<swb_tree_dev> d_tree;
  dev_buf<unsigned long long> d_exhausted;
  bool pool_tree = false;
  dev_buf<double> d_x, d_y;
  dev_buf<int32_t> d_nspr, d_entry, d_step_count, d_episode;
  dev_buf<uint8_t> d_reset_next;
  dev_buf<uint32_t> d_ovf, d_ovf_bitmap;
  int ovf_slots = 0;
  // cost-ordered dispatch (swb_params::cost_cnt)
  dev_buf<uint32_t> d_cost_cnt;
  dev_buf<int32_t> d_cost_list;
  dev_buf<int32_t> d_ccost_list;     // ... and the environments in order of the cover kernel's cost (swb_params::cover_order)
  bool cover_lists_filed = false;    // the previous launch filed every environment (it rendered)
  int launch_phase = 0;              // launch count % 3 (swb_params::cphase)
  int launch_parity = 0;
  // hand-off cover -> resample
  dev_buf<uint32_t> d_runs, d_rhdr, d_arena_head;
  dev_buf<int32_t> d_env_state;      // swb_get_env_state's 20-byte record
  int arena_override = -1;           // SWB_ARENA_UNITS (tests): units of the shared arena; -1: sized from the batch
  int run_cap_worst = 0;             // (max(4, S + 1) canvas heights + 1: what a list reserves until swb_trim_run_lists)
  bool lists_trimmed = false;        // the lists have been cut down to what the launches so far needed
  bool lists_valid = false;          // the last launch wrote them (it rendered through the second kernel)
  // kept lists (swb_params::list_epoch): the epoch launches stamp their lists with -- never 0 --, bumped by everything but a step
  // that changes what a list depends on or where it lives; SWB_NO_KEEP_LISTS: every launch passes epoch 0, nothing is kept
  uint32_t list_epoch = 1;
  bool no_keep_lists = false;
  dev_buf<unsigned long long> d_list_stats;   // SWB_LIST_STATS: cover waves that kept / built their lists (swb_list_stats)
  // frame cache (swb_params::frame_cache): the engine's own copy of every environment's last frame, from which the resample
  // waves of an environment whose lists were kept write the caller's frame.  Only on handles whose frames come from
  // swb_resample_kernel under a live list epoch; SWB_NO_FRAME_CACHE (tests, A/B runs) and a failed allocation leave it out
  dev_buf<uint8_t> d_frame_cache;
  int spec_copy = 1;                 // where the cover launch's copy workgroups stand (swb_params::spec_copy): 1 behind, 2 first (SWB_SPEC_COPY)
  dev_buf<unsigned long long> d_frame_stats;  // SWB_LIST_STATS: frames copied, tasks that filled / resampled (swb_frame_stats)
  // task cache (swb_params::task_cache): one record per environment of its last task evaluation, stamped with task_epoch -- never
  // 0, a counter of its own beside list_epoch: a step without a frame moves the list epoch and must not empty this cache.
  // SWB_NO_TASK_CACHE (tests, A/B runs) and a failed allocation leave it out: every wave evaluates
  dev_buf<swb_task_record> d_task_cache;
  uint32_t task_epoch = 1;
  dev_buf<unsigned long long> d_task_stats;   // SWB_LIST_STATS: stepping waves that reused / evaluated the task (swb_task_stats)
  // split bands (swb_params::split_bands): nbands is then the count the lists are built for, the nominal count is one
  bool split_bands = false;
  dev_buf<unsigned long long> d_split_stats;  // SWB_LIST_STATS: whole / band / whole-copy tasks (swb_split_stats)
  dev_buf<int32_t> d_band_y0, d_band_first, d_band_lo, d_cg_lo, d_cg_hi;
  dev_buf<uint32_t> d_v_break;
  // live sprite overrides (swb_set_sprite_attr), allocated at the first call
  dev_buf<uint8_t> d_ov_flag;
  dev_buf<int32_t> d_ov_shape;
  dev_buf<double> d_ov_scale, d_ov_angle, d_ov_cpath;
  dev_buf<int8_t> d_ov_label;
  dev_buf<int8_t> d_ov_cell_label;
  bool setters = false;              // swb_set_sprite_attr has been called: the override arrays exist (d_ov_flag alone does not say
                                     // so: a handle with task sets allocates the flags to run the OV kernels)
  // task sets (swb_set_task_sets): the table, and the set of every pool entry (every entry 0 after a pool is installed).
  // n_sets == 0: the handle has none, and the pointer behind its override flags, if it has flags, stays NULL
  int n_sets = 0;
  swb_task_set sets[SWB_MAX_TASK_SETS] = {};   // the table as installed (normalised); its device copy heads d_p_set
  dev_buf<uint8_t> d_p_set;          // SWB_SET_TABLE_BYTES of table, then one byte per pool entry (allocated with every pool)
  // timing
  bool timing = false;
  struct step_events { hipEvent_t e0, e1, e2; };     // before cover, between the kernels, after resample / fill
  std::vector<step_events> events;
  std::vector<step_events> event_pool;               // events of flushed steps, reused (no hipEventCreate per step)
  // read once at swb_create (never per launch): the device's compute units and the test / A-B switches of the environment
  int cus = 0;
  bool no_paint_in_cover = false, force_cover_order = false;
  // large-frame path (canvases wider than the widest cover build, images wider than SWB_MAX_CG column groups; SWB_LARGE_FRAMES=1
  // forces it): the cover kernel's state phase, then swb_lf_raster_kernel / swb_lf_vertical_kernel over a scratch buffer
  bool large_frames = false;
  // many-sprite path (more than SWB_TUNED_SPRITES sprites; SWB_MANY_SPRITES=1 forces it): swb_ms_state_kernel, then the
  // large-frame render kernels (large_frames is set too)
  bool many_sprites = false;
  size_t lf_scratch_budget = (size_t)256 << 20;   // bytes of horizontal-pass scratch: the batch is rendered in chunks that fit
  dev_buf<int32_t> d_lf_hb, d_lf_hpo, d_lf_hp, d_lf_vb, d_lf_vk;
  int lf_vks = 0;
  dev_buf<uint8_t> d_lf_tmp;                      // ... that scratch (grown on demand)
  double timed_ms = 0.0, timed_cover_ms = 0.0;
  int64_t timed_launches = 0;
  // swb_rollout: the scratch state of the virtual environments (one allocation, grown on demand)
  dev_buf<unsigned char> d_rollout;
  dev_buf<swb_params> d_rollout_steps;     // ... and the K per-step copies of swb_params swb_rollout_fork_kernel writes
  // swb_rollout_frames: candidates of the last swb_rollout, whose end states the scratch holds (0: none has run); whether a
  // pool call since then has made them describe entries that may have been redrawn; the staging block of picked candidates
  int rollout_M = 0;
  bool rollout_stale = false;
  dev_buf<unsigned char> d_rollout_pick;
  // swb_rollout_trajectory: the states after each of the K steps of the last rollout (one allocation, grown on demand), and that
  // K (0: the last rollout was a plain swb_rollout, which kept no steps)
  dev_buf<unsigned char> d_rollout_traj;
  int rollout_kept_K = 0;
};

namespace {

typedef void (*kernel_fn)(const swb_params);

// cover kernel by canvas width (NW 32-pixel words per canvas row); resample kernel by the output rows a canvas
// row can feed at once (VS)
// (fn_sets / fn_paint_sets: the builds of handles with task sets, swb_cover_sets_kernel)
struct variant { int nw; kernel_fn fn, fn_ov, fn_paint, fn_paint_ov; size_t lds_fixed, outrow_bytes; kernel_fn fn_sets, fn_paint_sets; };

template <int NW>
variant make_variant() {
  const size_t outrow = 528;          // wave_lds::outrow is build_all_edges' scratch (132 dwords)
  kernel_fn paint = nullptr, paint_ov = nullptr;       // the builds that paint the frame themselves: canvases of up to 64 px only
  kernel_fn paint_sets = nullptr;
  if constexpr (NW == 2) { paint = swb_cover_kernel<NW, false, true>; paint_ov = swb_cover_kernel<NW, true, true>; }
  if constexpr (NW == 2) paint_sets = swb_cover_sets_kernel<NW, true>;
  return {NW, swb_cover_kernel<NW>, swb_cover_kernel<NW, true>, paint, paint_ov, (sizeof(wave_lds<NW>) + outrow + 15) & ~(size_t)15, outrow,
          swb_cover_sets_kernel<NW, false>, paint_sets};
}

// The cover build a handle launches: with task sets the SETS build (overrides included), after a sprite setter the OV build.
kernel_fn cover_fn(const swb_engine* h, const variant* v);
kernel_fn cover_paint_fn(const swb_engine* h, const variant* v);

const variant kVariants[] = {make_variant<2>(), make_variant<4>(), make_variant<5>(), make_variant<10>(), make_variant<20>()};

kernel_fn cover_fn(const swb_engine* h, const variant* v) { return h->n_sets ? v->fn_sets : (h->d_ov_flag ? v->fn_ov : v->fn); }
kernel_fn cover_paint_fn(const swb_engine* h, const variant* v) {
  return h->n_sets ? v->fn_paint_sets : (h->d_ov_flag ? v->fn_paint_ov : v->fn_paint);
}

const variant* pick_variant(int Wc) {
  for (const variant& v : kVariants)
    if (32 * v.nw >= Wc) return &v;
  return nullptr;
}

kernel_fn pick_resample(int AA, int vslots, int* vs_out) {
  if (AA == 1) { if (vs_out) *vs_out = 0; return swb_fill_kernel; }
  if (vslots <= 6) { if (vs_out) *vs_out = 6; return swb_resample_kernel<6>; }
  if (vs_out) *vs_out = 8;
  return swb_resample_kernel<8>;
}

// LDS bytes of one wave (= one environment) of the cover kernel: wave_lds + edge records + span lists.  The
// centred paths (16 B per vertex) borrow the idle mask arrays, or the edge records' storage.
size_t lds_per_wave(const swb_engine* h, const variant* v, int* cpath_in_masks) {
  const swb_params& p = h->p;
  const size_t cpath_bytes = (size_t)p.max_edges * 16;
  const int in_masks = (2 * (size_t)SWB_NWA(v->nw) * SWB_WAVE * 4 >= cpath_bytes) ? 1 : 0;
  if (cpath_in_masks) *cpath_in_masks = in_masks;
  return (v->lds_fixed + (((size_t)p.max_edges * sizeof(edge_rec) + 15) & ~(size_t)15) +
          (size_t)p.max_spans * SWB_WAVE * 4 + 15) & ~(size_t)15;
}

// The lists in memory stop being what a build under the handle's state would write (swb_params::list_epoch): no launch keeps
// a list stamped before this.
void bump_list_epoch(swb_engine* h) {
  if (++h->list_epoch == 0u) h->list_epoch = 1u;
}

// What a task evaluation depends on -- positions, labels, sprite counts, the pool rows in use, overrides -- may have changed
// outside a step: no record stamped before this is reused (swb_params::task_epoch), and no list is kept either.  Every call
// site of the two says which it is: BOTH (this one), or LISTS ONLY (bump_list_epoch: the call moves or rebuilds lists and
// leaves the state the task reads alone).  swb_reset_all and swb_reset_envs need neither for the task: a reset step evaluates.
void bump_state_epochs(swb_engine* h) {
  bump_list_epoch(h);
  if (++h->task_epoch == 0u) h->task_epoch = 1u;
}

// Overflow slots for the span lists of the cover kernel: one per wave that can be resident at once (occupancy of
// the kernel that will be launched with its LDS footprint x CUs, capped by the batch), never one per environment.
// (fn_alt: the other build of the same family -- the one that paints the frame itself / the one that does not --, which a
// launch with / without an observation buffer switches to: the slots are sized once for the more demanding of the two)
int ensure_overflow_slots(swb_engine* h, kernel_fn fn, kernel_fn fn_alt, size_t lds_bytes) {
  if (h->d_ovf) return 0;
  int per_cu = 0;
  for (kernel_fn f : {fn, fn_alt}) {
    int n = 0;
    if (!f) continue;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, reinterpret_cast<const void*>(f), SWB_WAVE, lds_bytes) != hipSuccess || n < 1)
      n = 32;
    per_cu = std::max(per_cu, n);
  }
  long long slots = (long long)per_cu * h->cus;
  slots = std::min<long long>(2 * slots, (long long)h->p.N);              // the bitmap stays at most half full: few retries
  slots = (slots + 31) / 32 * 32;
  h->ovf_slots = (int)slots;
  if (h->d_ovf.fill(nullptr, (size_t)slots * 64 * h->p.ovf_cap) || h->d_ovf_bitmap.fill(nullptr, (size_t)slots / 32)) return SWB_ERR_HIP;
  h->p.ovf = h->d_ovf; h->p.ovf_bitmap = h->d_ovf_bitmap; h->p.ovf_slots = h->ovf_slots;
  return 0;
}

// Bands of output rows, the rows at which a run must end, and the canvas columns each group of 64 output columns
// can see -- from the resampling tables (anti_aliasing > 1) or the identity (anti_aliasing = 1).
// need_lists = false: a handle whose cover kernel paints the frame itself (anti_aliasing = 1, an image of up to 64 columns)
// never hands anything to a second kernel and reserves no lists.
int ensure_handoff_tables(swb_engine* h, bool need_lists = true) {
  if (!h->tables_dirty && (h->d_runs || !need_lists)) return 0;
  bump_list_epoch(h);                // LISTS ONLY (new tables, new lists: nothing written before this is kept)
  swb_params& p = h->p;
  int nb = h->nbands;
  // Bands: about Ho / nb rows each; for the resample kernel the first row of a band is moved so that the number of
  // output rows in flight at its first canvas row is a multiple of VS (the band's oldest row then sits in slot 0).
  int vs = 0;
  (void)pick_resample(p.AA, h->vslots, &vs);
  auto first_in_flight = [&](int o_lo) {
    int f = o_lo;
    while (f > 0 && h->v_end_host[f - 1] >= h->v_ymin_host[o_lo]) --f;
    return f;
  };
  std::vector<int32_t> blo(1, 0);
  for (int b = 1; b < nb; ++b) {
    int want = (int)((long long)b * p.Ho / nb), best = -1;
    if (p.AA == 1) best = want;
    else
      for (int d = 0; d < p.Ho && best < 0; ++d)
        for (int c : {want + d, want - d})
          if (c > blo.back() && c < p.Ho && first_in_flight(c) % vs == 0) { best = c; break; }
    if (best > blo.back() && best < p.Ho) blo.push_back(best);
  }
  nb = (int)blo.size();
  blo.push_back(p.Ho);
  p.nbands = nb;
  std::vector<int32_t> y0(nb, 0), first(nb, 0), lo(p.ncg, 0), hi(p.ncg, 0);
  // two bit tables, one behind the other: the rows that start a new run, and those among them where a band starts (the run
  // that starts there heads a band's part of the list: never a continuation run, see emit_runs)
  const size_t brk_words = (size_t)(p.Hc + 31) / 32 + 3;            // (+3: a batch reads three words from its first row's word)
  std::vector<uint32_t> brk(2 * brk_words, 0u);
  auto set_break = [&](int y) { if (y >= 0 && y < p.Hc) brk[y >> 5] |= 1u << (y & 31); };
  for (int b = 0; b < nb; ++b) {
    const int o_lo = blo[b];
    if (p.AA == 1) { y0[b] = o_lo; first[b] = o_lo; }
    else { y0[b] = h->v_ymin_host[o_lo]; first[b] = first_in_flight(o_lo); }
    set_break(y0[b]);
    if (y0[b] >= 0 && y0[b] < p.Hc) brk[brk_words + (y0[b] >> 5)] |= 1u << (y0[b] & 31);
  }
  if (p.AA != 1)
    for (int o = 0; o < p.Ho; ++o) set_break(h->v_end_host[o] + 1);
  for (int g = 0; g < p.ncg; ++g) {
    if (p.AA == 1) { lo[g] = 64 * g; hi[g] = std::min(64 * g + 64, p.Wo); continue; }
    lo[g] = 1 << 30; hi[g] = 0;
    for (int o = 64 * g; o < std::min(64 * g + 64, p.Wo); ++o) {
      lo[g] = std::min(lo[g], h->h_xmin_host[o]);
      hi[g] = std::max(hi[g], h->h_xmin_host[o] + h->h_cnt_host[o]);
    }
  }
  if (h->d_band_y0.fill(y0.data(), y0.size()) || h->d_band_first.fill(first.data(), first.size()) ||
      h->d_band_lo.fill(blo.data(), blo.size()) || h->d_v_break.fill(brk.data(), brk.size()) ||
      h->d_cg_lo.fill(lo.data(), lo.size()) || h->d_cg_hi.fill(hi.data(), hi.size()))
    return SWB_ERR_HIP;
  p.band_lo = h->d_band_lo;
  p.band_y0 = h->d_band_y0; p.band_first = h->d_band_first; p.v_break = h->d_v_break; p.cg_lo = h->d_cg_lo; p.cg_hi = h->d_cg_hi;
  // run lists: run_cap units of 8 bytes per (environment, column group), then the shared arena their overflow segments
  // come from, then 4 units of slack (the resample kernel reads a run's first 16 bytes in one go)
  if (!h->d_runs && need_lists) {
    const size_t fixed = (size_t)p.N * p.ncg * p.run_cap;
    // arena (a list that outgrows its own part moves there, into a segment twice as large): half of the own parts together once
    // they have been trimmed (before that they hold any scene of convex sprites by themselves), and at least eight worst-case
    // lists -- sixteen times their size, a moved list's segment being a power of two times its own part
    size_t arena = std::max(h->lists_trimmed ? fixed / 2 : (size_t)0, (size_t)16 * h->run_cap_worst);
    if (h->arena_override >= 0) arena = (size_t)h->arena_override;
    const size_t units = fixed + arena + 4;
    if (units * 8 >= ((size_t)1 << 32))                                  // (list positions are 32-bit byte offsets)
      return fail(SWB_ERR_INVALID, "run lists of %zu MB (%d environments x %d column groups x %d units + an arena of %zu units) exceed "
                  "the 4 GB a list position can address: step fewer environments per engine", units * 8 >> 20, p.N, p.ncg, p.run_cap, arena);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && units * 8 + (size_t)p.N * SWB_RHDR_DWORDS * 4 > free_b)
      return fail(SWB_ERR_HIP, "run lists need %zu MB of device memory (%d environments x %d column groups x %d units of 8 bytes + an "
                  "arena of %zu units), %zu MB are free", units * 8 >> 20, p.N, p.ncg, p.run_cap, arena, free_b >> 20);
    if (h->d_runs.fill(nullptr, units * 2) || h->d_rhdr.fill(nullptr, (size_t)p.N * SWB_RHDR_DWORDS) || h->d_arena_head.fill(nullptr, 2))
      return SWB_ERR_HIP;
    p.runs = h->d_runs; p.rhdr = h->d_rhdr;
    p.arena_head = h->d_arena_head;
    p.arena_base = (int64_t)fixed;
    p.arena_units = (int32_t)std::min(arena, (size_t)0x7fffffff);
  }
  h->tables_dirty = false;
  return 0;
}

// Frees the hand-off lists; the next launch allocates them again with the capacity h->p.run_cap holds by then.
int drop_run_lists(swb_engine* h) {
  if (!h->d_runs) return 0;
  HIP_TRY(hipDeviceSynchronize());
  h->d_runs.release(); h->d_rhdr.release(); h->d_arena_head.release();
  h->p.runs = nullptr; h->p.rhdr = nullptr; h->p.arena_head = nullptr;
  bump_list_epoch(h);                // LISTS ONLY (a trim, or a pool call that bumps both itself)
  h->lists_valid = false;
  h->tables_dirty = true;
  return 0;
}

// A new pool may hold denser scenes than the one the lists were trimmed to: back to the full reservation.
int restore_run_list_reservation(swb_engine* h) {
  if (!h->lists_trimmed) return 0;
  if (int rc = drop_run_lists(h)) return rc;
  h->lists_trimmed = false;
  if (!getenv("SWB_RUN_CAP")) h->p.run_cap = h->run_cap_worst;
  return 0;
}

int flush_timing(swb_engine* h) {
  for (auto& ev : h->events) {
    HIP_TRY(hipEventSynchronize(ev.e2));
    float ms = 0.f, ms_cover = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e2));
    HIP_TRY(hipEventElapsedTime(&ms_cover, ev.e0, ev.e1));
    h->timed_ms += ms;
    h->timed_cover_ms += ms_cover;
    h->timed_launches += 1;
    h->event_pool.push_back(ev);
  }
  h->events.clear();
  return 0;
}

// ---------------------------------------------------------------------------------------------------
// What the two step paths share: launch() (tuned kernels) and launch_large() (large frames, many sprites) are each
// check_ready, bind_step, their own kernels between the three marks of a step_timer, and, where the state phase is a cover build,
// cover_launch_config.
// ---------------------------------------------------------------------------------------------------

int check_ready(const swb_engine* h, const void* actions, int render_only) {
  if (!h->have_shapes) return fail(SWB_ERR_STATE, "swb_upload_shapes has not been called");
  if (!h->have_pool) return fail(SWB_ERR_STATE, "swb_set_pool has not been called");
  if (h->p.AA != 1 && !(h->have_h && h->have_v))
    return fail(SWB_ERR_STATE, "swb_upload_resample (both axes) is required when anti_aliasing > 1");
  if (!render_only && actions == nullptr) return fail(SWB_ERR_INVALID, "actions is NULL");
  return 0;
}

// The kernel argument of one launch: the handle's parameters with the caller's buffers bound.
// `active`: the mask of swb_step_masked (swb_params::active), NULL for every other launch.
swb_params bind_step(const swb_engine* h, const void* actions, const swb_outputs* out, int render_only, const uint8_t* active) {
  swb_params p = h->p;
  p.actions = actions;
  p.active = active;
  p.obs = out ? out->obs : nullptr;
  p.reward = out ? out->reward : nullptr;
  p.discount = out ? out->discount : nullptr;
  p.step_type = out ? out->step_type : nullptr;
  p.success = out ? out->success : nullptr;
  p.error = out ? out->error : nullptr;
  p.render_only = render_only;
  // the task cache (swb_params::task_cache) and its counters: steps only -- h->p itself never carries them, so renders,
  // evaluations and the rollouts' forked blocks neither read nor write a record (bind_view: nor a launch on another state)
  if (render_only == 0) {
    p.task_cache = h->d_task_cache.ptr;
    p.task_stats = h->d_task_stats.ptr;
    p.task_epoch = h->task_epoch;
  }
  return p;
}

// swb_rollout_frames: the launch draws the environments of `view` (a chunk of N virtual environments of a rollout's scratch, or
// the staging block of picked candidates) in place of the live ones.  Such a launch is never a counted step of swb_timing_enable.
void bind_view(swb_params* p, const swb_state_view* view) {
  if (!view) return;
  p->x = view->x; p->y = view->y; p->nspr = view->nspr; p->entry = view->entry; p->step_count = view->step_count;
  p->episode = view->episode; p->pool_base = view->pool_base; p->pool_len = view->pool_len; p->reset_next = view->reset_next;
  p->task_cache = nullptr; p->task_stats = nullptr;
}

// Launch configuration of cover build `fn` of variant `v`: the dynamic LDS of a wave, and how the kernel finds its way in it.
int cover_launch_config(const swb_engine* h, const variant* v, kernel_fn fn, swb_params* p, size_t* lds_out) {
  int cpath_in_masks = 0;
  const size_t lds = lds_per_wave(h, v, &cpath_in_masks);
  p->cpath_in_masks = cpath_in_masks;
  p->lds_per_wave = (int32_t)lds;
  p->outrow_bytes = (int32_t)v->outrow_bytes;
  if (lds > 160 * 1024) return fail(SWB_ERR_INVALID, "LDS request %zu B exceeds 160 KiB", lds);
  if (lds > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  *lds_out = lds;
  return 0;
}

// The three events of a timed step (swb_timing_enable; nothing at all otherwise): begin() before the first kernel, mid() behind the
// state / cover kernel, end() behind the last one.  A counted step's events wait for flush_timing; those of a launch that is not
// one (swb_evaluate), or that failed half-way, go back to the pool unread.
struct step_timer {
  swb_engine* h;
  hipStream_t stream;
  swb_engine::step_events ev = {nullptr, nullptr, nullptr};
  bool held = false;
  step_timer(swb_engine* h_, hipStream_t stream_) : h(h_), stream(stream_) {}
  ~step_timer() { if (held) h->event_pool.push_back(ev); }
  int begin() {
    if (!h->timing) return 0;
    if (!h->event_pool.empty()) { ev = h->event_pool.back(); h->event_pool.pop_back(); }
    else
      for (hipEvent_t* e : {&ev.e0, &ev.e1, &ev.e2}) HIP_TRY(hipEventCreate(e));
    held = true;
    HIP_TRY(hipEventRecord(ev.e0, stream));
    return 0;
  }
  int mid() {
    if (held) HIP_TRY(hipEventRecord(ev.e1, stream));
    return 0;
  }
  int end(bool counted) {
    if (!held) return 0;
    HIP_TRY(hipEventRecord(ev.e2, stream));
    if (!counted) return 0;
    held = false;
    h->events.push_back(ev);
    return h->events.size() >= 4096 ? flush_timing(h) : 0;
  }
};

// This handle's cover kernel paints the frame itself -- anti_aliasing = 1 and one column group, that is a canvas of up to 64 px:
// the one variant with painting builds -- and no second kernel runs, no run lists exist.  SWB_NO_PAINT_IN_COVER (tests, A/B) keeps
// such a handle on two kernels; honour_switch = false asks about the geometry alone.
bool paints_in_cover(const swb_engine* h, const variant* v, bool honour_switch = true) {
  return h->p.AA == 1 && h->p.ncg == 1 && v && v->fn_paint && !(honour_switch && h->no_paint_in_cover);
}

int launch_large(swb_engine* h, const void* actions, const swb_outputs* out, int render_only, hipStream_t stream,
                 const swb_state_view* view, const uint8_t* active);

int launch(swb_engine* h, const void* actions, const swb_outputs* out, int render_only, hipStream_t stream,
           const swb_state_view* view = nullptr, const uint8_t* active = nullptr) {
  if (h->large_frames) return launch_large(h, actions, out, render_only, stream, view, active);
  if (int rc = check_ready(h, actions, render_only)) return rc;
  const variant* v = pick_variant(h->p.Wc);
  if (!v) return fail(SWB_ERR_INVALID, "canvas %dx%d not supported", h->p.Wc, h->p.Hc);
  if (int rc = ensure_handoff_tables(h, !paints_in_cover(h, v))) return rc;
  int vs = 0;
  const kernel_fn fn2 = pick_resample(h->p.AA, h->vslots, &vs);
  swb_params p = bind_step(h, actions, out, render_only, active);
  bind_view(&p, view);
  if (p.v_tab && vs == 8) {                                           // slot tables of this VS
    p.v_tab += (size_t)p.Hc * SWB_VSLOTS;
    p.v_pfx += (size_t)(p.Hc + 1) * SWB_VSLOTS;
  }
  // engines on which a sprite setter has been called run the build that reads the per-environment overrides
  const bool paint = p.obs && paints_in_cover(h, v);
  const kernel_fn fn = paint ? cover_paint_fn(h, v) : cover_fn(h, v);
  size_t lds = 0;
  if (int rc = cover_launch_config(h, v, fn, &p, &lds)) return rc;
  // first launch, a new pool that shrank the LDS footprint (more waves resident), or the switch to the override build -- not
  // the switch between the painting and the plain build of a family, which alternating launches with and without an
  // observation buffer make at every launch (the cache is keyed on the family's plain build)
  const kernel_fn fn_family = cover_fn(h, v);
  if (!h->d_ovf || (int)lds < h->ovf_lds_bytes || fn_family != h->ovf_fn) {
    if (h->d_ovf) {
      HIP_TRY(hipDeviceSynchronize());
      h->d_ovf.release(); h->d_ovf_bitmap.release();
    }
    if (int rc = ensure_overflow_slots(h, fn_family, cover_paint_fn(h, v), lds)) return rc;
    bump_list_epoch(h);              // LISTS ONLY (new overflow slots)
    h->ovf_lds_bytes = (int)lds;
    h->ovf_fn = fn_family;
    p.ovf = h->p.ovf; p.ovf_bitmap = h->p.ovf_bitmap; p.ovf_slots = h->p.ovf_slots;
  }
  // Kept lists (swb_params::list_epoch): a launch that draws the live state through the second kernel stamps its lists with the
  // handle's epoch and keeps those that carry it.  A launch on a state view leaves another state's lists behind: epoch 0, it
  // keeps nothing and stamps them invalid.  A step without a frame moves sprites and lists nothing: the epoch moves on.
  p.list_epoch = (view || !p.obs || paint || !p.rhdr || h->no_keep_lists) ? 0u : h->list_epoch;
  // (the frame cache's mover takes 16 bytes per lane where the caller's buffer and every row segment of it start on 16)
  p.obs_aligned16 = (p.obs && (reinterpret_cast<uintptr_t>(p.obs) & 15u) == 0 && (p.Wo & 15) == 0) ? 1 : 0;
  // Speculative copies (swb_params::spec_copy): a rendering launch on the live state of a handle with a
  // frame cache that files its tasks by cost grows its cover grid by one copy workgroup per (environment, column group).  State
  // views, epoch-0 launches, the painting builds and handles without a cache launch the grid they always launched; so does a
  // handle without cost order, whose resample grid has a wave for every environment: there that wave copies, as before.
  p.spec_copy = (p.obs && p.frame_cache && p.list_epoch != 0u && !paint && p.cost_cnt) ? h->spec_copy : 0;
  p.split_carry = view ? 1 : 0;
  // LISTS ONLY: the step itself keeps every task record it leaves in step with the positions it writes
  if (!p.obs && render_only == 0 && !view) bump_list_epoch(h);
  step_timer timer(h, stream);
  if (int rc = timer.begin()) return rc;
  const size_t lds2 = p.AA == 1 ? 0 : (((size_t)p.h_pfx_len * 4 + 15) & ~(size_t)15);
  p.parity = h->launch_parity;
  p.cphase = h->launch_phase;
  // anti_aliasing = 1, one column group: the cover kernel paints the frame itself, there is no second kernel
  p.paint_in_cover = paint ? 1 : 0;
  // environments in order of what their cover wave cost in the previous launch -- if that launch filed them all
  // (and the launch is more than one round of cover waves but not many: one round needs no order, and from about a dozen
  // rounds on the plain order was measured 1.6 % faster)
  {
    const long long slots = (long long)std::max(h->cus, 1) * 4 * SWB_COVER_WAVES(v->nw);
    p.cover_order = (h->cover_lists_filed && p.ccost_list && ((p.N > slots && p.N <= 4 * slots) || h->force_cover_order)) ? 1 : 0;
    if (p.N > 2 * slots) p.prio_levels &= ~2;          // (cover waves' priorities: measured +1.3 % at three rounds of waves)
  }
  // (cost-ordered: block b serves rank b / 8 of shard b % 8; a shard holds up to cost_cap environments)
  // (N < 2^24 where tasks are filed by cost, ncg <= 4: the grid with the copy workgroups stays below 2^27)
  auto launch_cover = [&](int e0, int e1) {
    const unsigned copy_groups = p.spec_copy ? (unsigned)(e1 - e0) * (unsigned)p.ncg : 0u;
    hipLaunchKernelGGL(fn, dim3((unsigned)(e1 - e0) + copy_groups), dim3(SWB_WAVE), lds, stream, p);
  };
  auto launch_resample = [&](int e0, int e1, hipStream_t st) {
    const int blocks_x = p.cost_cnt ? SWB_COST_SHARDS * ((p.cost_cap + SWB_RS_WAVES_PER_BLOCK - 1) / SWB_RS_WAVES_PER_BLOCK)
                                    : (e1 - e0 + SWB_RS_WAVES_PER_BLOCK - 1) / SWB_RS_WAVES_PER_BLOCK;
    // (cost-ordered: a list entry names its column group -- and, for small batches, its band: swb_params::band_tasks)
    const dim3 grid(blocks_x, (p.cost_cnt && p.band_tasks) ? 1 : p.nbands, p.cost_cnt ? 1 : p.ncg);
    hipLaunchKernelGGL(fn2, grid, dim3(SWB_WAVE * SWB_RS_WAVES_PER_BLOCK), lds2, st, p);
  };
  launch_cover(0, p.N);
  HIP_TRY(hipGetLastError());
  // From here on the cover kernel may have run: its waves have told the resample waves of this launch to fill the frame cache,
  // or that it is filled (SWB_RHDR_FRAME).  If those never run, the words are wrong -- every error return below moves the epoch,
  // the next launch builds every list and resets every word.
  struct epoch_guard {
    swb_engine* h; bool armed = true;
    ~epoch_guard() { if (armed) bump_list_epoch(h); }     // LISTS ONLY (a cover wave that ran left positions and record in step)
  } guard{h};
  if (int rc = timer.mid()) return rc;            // (a painting cover kernel is the whole step: nothing follows before end())
  if (p.obs && !p.paint_in_cover) launch_resample(0, p.N, stream);
  HIP_TRY(hipGetLastError());
  if (!p.obs && p.cost_cnt && render_only != 2)   // no second kernel to clear the next launch's bucket counters (kind 0; the cover kernel keeps kind 1)
    HIP_TRY(hipMemsetAsync(h->d_cost_cnt + (size_t)(p.parity ^ 1) * SWB_COST_SET, 0, SWB_COST_SET * sizeof(uint32_t), stream));
  if (!p.obs && p.cost_cnt && p.split_bands && render_only != 2) {   // ... nor to hand the split-bands word and its cleared counters to the next launch
    HIP_TRY(hipMemsetAsync(h->d_cost_cnt + SWB_COST_WORD_SPLIT_CNT(p.parity ^ 1, 0, 0), 0, SWB_COST_SET * sizeof(uint32_t), stream));
    HIP_TRY(hipMemcpyAsync(h->d_cost_cnt + SWB_COST_WORD_SPLIT(p.parity ^ 1), h->d_cost_cnt + SWB_COST_WORD_SPLIT(p.parity), sizeof(uint32_t),
                           hipMemcpyDeviceToDevice, stream));
  }
  guard.armed = false;
  // swb_evaluate files nothing and lists nothing: the dispatch state (parity, phase, what the previous launch filed) stays as
  // the last step left it -- an evaluation between two steps does not cost the next one its cost order (round-5 advice) --, and
  // it is not a timed launch
  if (render_only == 2) return timer.end(false);
  h->cover_lists_filed = p.obs && p.ccost_list;
  h->lists_valid = p.obs && !p.paint_in_cover;
  h->launch_phase = (h->launch_phase + 1) % 3;
  h->launch_parity ^= 1;
  return timer.end(view == nullptr);
}

// ---------------------------------------------------------------------------------------------------
// Large-frame path (swb_engine::large_frames): the cover kernel of the narrowest build with obs = NULL -- its state phase
// only, whose LDS does not depend on the canvas --, then the render kernels of swb_kernels.hip.inc on the state it left,
// in chunks of environments whose horizontal-pass scratch fits lf_scratch_budget.
// ---------------------------------------------------------------------------------------------------
#define SWB_LF_MAX_CANVAS 4096        // canvas pixels in either direction
#define SWB_LF_MAX_COLUMNS 1024       // image columns (image_size[0])

// LDS of a workgroup of the raster kernel: the head (per-sprite tables), vertices and edges of `max_verts_env` polygon
// vertices, and per wave a canvas row, its span mask and the crossings of a row
size_t lf_lds_bytes(const swb_params& p, int max_verts_env) {
  const size_t row_bytes = (size_t)((p.Wc + 15) & ~15), mask_words = (size_t)(p.Wc / 32 + 1);
  return swb_lf_head_bytes(max_verts_env) + (size_t)SWB_LF_WAVES * (row_bytes + 4 * mask_words + 2 * 4 * SWB_LF_MAX_CROSS);
}
#define SWB_LF_MAX_LDS (160 * 1024)

// Refuses a scene of `verts` polygon vertices whose tables would not fit the raster kernel's LDS (large-frame handles only):
// a pool must fail where it is installed, not at its first launch.
int lf_check_vertices(const swb_engine* h, int verts, const char* what) {
  if (!h->large_frames || lf_lds_bytes(h->p, std::max(verts, 4)) <= SWB_LF_MAX_LDS) return 0;
  int budget = 4;                      // (the tables are sized in steps of 4 vertices: the budget named is one a scene can reach)
  while (lf_lds_bytes(h->p, budget + 4) <= SWB_LF_MAX_LDS) budget += 4;
  return fail(SWB_ERR_INVALID, "%s: a scene of %d polygon vertices exceeds the vertex budget of the large-frame raster kernel, %d vertices "
              "per scene at a %d px canvas (160 KiB of LDS)", what, verts, budget, h->p.Wc);
}

int lf_render(swb_engine* h, const swb_params& p, hipStream_t stream) {
  const size_t per_env = p.AA == 1 ? 0 : (size_t)p.Hc * p.Wo * 3;
  long long chunk = per_env ? (long long)(h->lf_scratch_budget / per_env) : (long long)p.N;
  chunk = std::max(1ll, std::min(chunk, std::min((long long)p.N, 65535ll)));       // (environments are a grid dimension)
  if (per_env && h->d_lf_tmp.count < (size_t)chunk * per_env) {
    if (h->d_lf_tmp) HIP_TRY(hipDeviceSynchronize());
    if (h->d_lf_tmp.fill(nullptr, (size_t)chunk * per_env)) return SWB_ERR_HIP;
  }
  swb_lf_args a;
  memset(&a, 0, sizeof(a));
  a.hb = h->d_lf_hb; a.hpo = h->d_lf_hpo; a.hp = h->d_lf_hp; a.vb = h->d_lf_vb; a.vk = h->d_lf_vk; a.vks = h->lf_vks;
  a.max_verts_env = std::max(p.max_edges, 4);
  a.row_bytes = (p.Wc + 15) & ~15;
  a.mask_words = p.Wc / 32 + 1;
  a.rows_per_block = p.N >= 64 ? 64 : 16;        // (small batches: more workgroups per environment)
  a.tmp = h->d_lf_tmp;
  const size_t lds = lf_lds_bytes(p, a.max_verts_env);
  if (lds > SWB_LF_MAX_LDS) return fail(SWB_ERR_INVALID, "large-frame raster kernel: LDS request %zu B exceeds 160 KiB", lds);
  if (lds > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(swb_lf_raster_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const int nd = (p.Wo * 3) >> 2;
  for (long long e0 = 0; e0 < p.N; e0 += chunk) {
    a.e0 = (int32_t)e0;
    a.ne = (int32_t)std::min(chunk, (long long)p.N - e0);
    hipLaunchKernelGGL(swb_lf_raster_kernel, dim3((p.Hc + a.rows_per_block - 1) / a.rows_per_block, a.ne), dim3(SWB_WAVE * SWB_LF_WAVES),
                       lds, stream, p, a);
    HIP_TRY(hipGetLastError());
    if (p.AA != 1) {
      hipLaunchKernelGGL(swb_lf_vertical_kernel, dim3((nd + SWB_WAVE - 1) / SWB_WAVE, (p.Ho + SWB_LF_WAVES - 1) / SWB_LF_WAVES, a.ne),
                         dim3(SWB_WAVE * SWB_LF_WAVES), 0, stream, p, a);
      HIP_TRY(hipGetLastError());
    }
  }
  return 0;
}

int launch_large(swb_engine* h, const void* actions, const swb_outputs* out, int render_only, hipStream_t stream,
                 const swb_state_view* view, const uint8_t* active) {
  if (int rc = check_ready(h, actions, render_only)) return rc;
  swb_params p = bind_step(h, actions, out, render_only, active);
  bind_view(&p, view);
  // the state phase: the cover kernel of the narrowest build with obs = NULL, or (many sprites) swb_ms_state_kernel, whose LDS
  // does not depend on the scene
  kernel_fn fn;
  size_t lds;
  if (h->many_sprites) {
    fn = h->n_sets ? swb_ms_state_sets_kernel : (h->d_ov_flag ? swb_ms_state_kernel<true> : swb_ms_state_kernel<false>);
    lds = sizeof(swb_ms_lds);
  } else {
    const variant* v = &kVariants[0];
    fn = cover_fn(h, v);
    if (int rc = cover_launch_config(h, v, fn, &p, &lds)) return rc;
  }
  step_timer timer(h, stream);
  if (int rc = timer.begin()) return rc;
  if (render_only != 1) {                      // the state phase (swb_render has no state to advance: the frame only)
    swb_params pc = p;
    pc.obs = nullptr;
    hipLaunchKernelGGL(fn, dim3(p.N), dim3(SWB_WAVE), lds, stream, pc);
    HIP_TRY(hipGetLastError());
  }
  if (int rc = timer.mid()) return rc;
  if (p.obs && render_only != 2)
    if (int rc = lf_render(h, p, stream)) return rc;
  return timer.end(render_only != 2 && !view); // (swb_evaluate: not a timed launch, as on the tuned path)
}

// swb_upload_resample of a large-frame handle: the raw Pillow tables, and per output column the prefix sums of its
// coefficients (the horizontal pass weighs a span of constant colour with one difference of two of them)
int upload_resample_large(swb_engine* h, int axis, int out_size, int ksize, const int32_t* bounds, const int32_t* coeffs) {
  const swb_params& p = h->p;
  if (ksize < 1) return fail(SWB_ERR_INVALID, "ksize must be >= 1");
  if (axis == 0) {
    if (out_size != p.Wo) return fail(SWB_ERR_INVALID, "horizontal table has %d outputs, image width is %d", out_size, p.Wo);
    std::vector<int32_t> hb(2 * (size_t)out_size), hpo(out_size), hp;
    for (int o = 0; o < out_size; ++o) {
      const int xmin = bounds[2 * o], cnt = bounds[2 * o + 1];
      if (cnt < 0 || cnt > ksize || xmin < 0 || xmin + cnt > p.Wc) return fail(SWB_ERR_INVALID, "bad horizontal bounds at %d", o);
      hb[2 * o] = xmin; hb[2 * o + 1] = cnt;
      hpo[o] = (int32_t)hp.size();
      int32_t acc = 0;
      hp.push_back(0);
      for (int j = 0; j < cnt; ++j) { acc += coeffs[(size_t)o * ksize + j]; hp.push_back(acc); }
    }
    if (h->d_lf_hb.fill(hb.data(), hb.size()) || h->d_lf_hpo.fill(hpo.data(), hpo.size()) || h->d_lf_hp.fill(hp.data(), hp.size()))
      return SWB_ERR_HIP;
    h->have_h = true;
  } else if (axis == 1) {
    if (out_size != p.Ho) return fail(SWB_ERR_INVALID, "vertical table has %d outputs, image height is %d", out_size, p.Ho);
    for (int r = 0; r < out_size; ++r) {
      const int ymin = bounds[2 * r], cnt = bounds[2 * r + 1];
      if (cnt < 0 || cnt > ksize || ymin < 0 || ymin + cnt > p.Hc) return fail(SWB_ERR_INVALID, "bad vertical bounds at %d", r);
    }
    if (h->d_lf_vb.fill(bounds, 2 * (size_t)out_size) || h->d_lf_vk.fill(coeffs, (size_t)out_size * ksize)) return SWB_ERR_HIP;
    h->lf_vks = ksize;
    h->have_v = true;
  } else {
    return fail(SWB_ERR_INVALID, "axis must be 0 or 1");
  }
  return SWB_OK;
}

// The override flags of a handle, allocated ONCE and only here: N flag bytes, then -- on a 64-byte line of its own -- the
// pointer to the task-set block (SWB_OV_SLOT; NULL until publish_entry_sets).  The layout is an agreement between this file and
// task_view_of<true> in the kernels: nothing else allocates, resizes or clears d_ov_flag as a whole (the flags are written
// one byte at a time, by ov_store and by the kernels' reset), and publish_entry_sets alone writes the pointer.
static_assert(SWB_OV_SLOT(1) == 64 && SWB_OV_SLOT(64) == 64 && SWB_OV_SLOT(65) == 128 && SWB_OV_FLAG_BYTES(64) == 128 &&
              sizeof(const uint8_t*) <= 64, "the block's pointer has a line of its own behind the flags");
int alloc_ov_flags(swb_engine* h) {
  if (h->d_ov_flag) return 0;
  return h->d_ov_flag.fill(nullptr, SWB_OV_FLAG_BYTES(h->p.N));
}

// Task sets: the kernels find the handle's block through the pointer behind the override flags (swb_params::ov_flag,
// SWB_OV_SLOT).  Synchronous: the block it replaces has been freed behind a device synchronise already.
int publish_entry_sets(swb_engine* h) {
  if (!h->n_sets) return 0;
  const uint8_t* block = h->d_p_set.ptr;
  HIP_TRY(hipMemcpy(h->d_ov_flag.ptr + SWB_OV_SLOT(h->p.N), &block, sizeof(block), hipMemcpyHostToDevice));
  return 0;
}

// ... a fresh block for a pool of P entries: the handle's table, then every entry in set 0.
int fill_entry_sets(swb_engine* h, int P) {
  if (!h->n_sets) return 0;
  std::vector<uint8_t> block(SWB_SET_TABLE_BYTES + (size_t)P, 0);
  memcpy(block.data(), h->sets, sizeof(h->sets));
  if (h->d_p_set.fill(block.data(), block.size())) return SWB_ERR_HIP;
  return publish_entry_sets(h);
}

// The pool's device arrays as the kernels see them (swb_set_pool, swb_sample_pool).  The angle and colour columns are optional in
// a pool set from the host, the per-cell labels exist on handles with a task that keys on position.
void bind_pool(swb_engine* h, bool have_angle, bool have_color) {
  swb_params& p = h->p;
  p.p_n = h->d_p_n; p.p_x = h->d_p_x; p.p_y = h->d_p_y; p.p_xv = h->d_p_xv; p.p_yv = h->d_p_yv;
  p.p_scale = h->d_p_scale; p.p_ca = h->d_p_ca; p.p_sa = h->d_p_sa; p.p_shape = h->d_p_shape; p.p_rgb = h->d_p_rgb;
  p.p_label = h->d_p_label; p.pool_base = h->d_pool_base; p.pool_len = h->d_pool_len;
  p.p_angle = have_angle ? h->d_p_angle.ptr : nullptr;
  p.p_color = have_color ? h->d_p_color.ptr : nullptr;
  p.p_cell_label = h->keyed ? h->d_p_cell_label.ptr : nullptr;
}

// Argument of swb_sample_pool_kernel.  skip_live (swb_resample_pool): entries an environment is playing are left as they are.
swb_sampler_args sampler_args(const swb_engine* h, uint64_t seed, uint64_t first_entry, bool skip_live) {
  return {h->d_sampler, h->pool_entries, h->p.S, h->p.n_tasks, seed, first_entry, skip_live ? h->d_entry.ptr : nullptr,
          skip_live ? h->d_pool_base.ptr : nullptr, skip_live ? h->d_pool_len.ptr : nullptr, h->p.N, h->d_p_n, h->d_p_x, h->d_p_y,
          h->d_p_xv, h->d_p_yv, h->d_p_scale, h->d_p_ca, h->d_p_sa, h->d_p_angle, h->d_p_color, h->d_p_shape, h->d_p_rgb,
          h->d_p_label, h->d_p_attr};
}


// The device arrays of a pool of P entries that a sampler kernel is about to fill (swb_sample_pool, swb_sample_pool_tree), and
// the environments' ranges in it; bound to the kernels' parameters.
int alloc_sampled_pool(swb_engine* h, int P, const int32_t* pool_base_host, const int32_t* pool_len_host) {
  const int S = h->p.S, T = h->p.n_tasks, N = h->p.N;
  const size_t PS = (size_t)P * S;
  int rc = 0;
  h->rollout_stale = true;                        // (swb_rollout_frames: as in swb_set_pool)
  h->pool_id = next_pool_id();
  if (h->pool_entries != P || !h->d_p_angle || !h->d_p_color || (h->keyed && !h->d_p_cell_label)) {
    rc |= h->d_p_n.fill(nullptr, P);
    rc |= h->d_p_x.fill(nullptr, PS); rc |= h->d_p_y.fill(nullptr, PS);
    rc |= h->d_p_xv.fill(nullptr, PS); rc |= h->d_p_yv.fill(nullptr, PS);
    rc |= h->d_p_scale.fill(nullptr, PS); rc |= h->d_p_ca.fill(nullptr, PS);
    rc |= h->d_p_sa.fill(nullptr, PS);
    rc |= h->d_p_shape.fill(nullptr, PS); rc |= h->d_p_rgb.fill(nullptr, PS);
    rc |= h->d_p_label.fill(nullptr, (size_t)P * T * S);
    if (h->keyed) rc |= h->d_p_cell_label.fill(nullptr, (size_t)P * T * S * SWB_MAX_CELLS);
    rc |= h->d_p_attr.fill(nullptr, PS);
    rc |= h->d_p_angle.fill(nullptr, PS); rc |= h->d_p_color.fill(nullptr, PS * 3);
  }
  rc |= h->d_pool_base.fill(pool_base_host, N);
  rc |= h->d_pool_len.fill(pool_len_host, N);
  rc |= fill_entry_sets(h, P);                                         // (task sets: every entry in set 0)
  if (rc) return SWB_ERR_HIP;
  h->pool_entries = P;
  bind_pool(h, true, true);
  return 0;
}

// ... and once the kernel is launched: every environment resets on its next step (environment.py:70), the run lists get
// their full reservation back, and the layout is remembered for swb_resample_pool.
int finish_sampled_pool(swb_engine* h, const int32_t* pool_base_host, const int32_t* pool_len_host, hipStream_t st) {
  const int N = h->p.N;
  HIP_TRY(hipMemsetAsync(h->d_reset_next, 1, N, st));
  HIP_TRY(hipMemsetAsync(h->d_episode, 0, sizeof(int32_t) * N, st));
  HIP_TRY(hipMemsetAsync(h->d_step_count, 0, sizeof(int32_t) * N, st));
  h->have_pool = true;
  if (int rc2 = restore_run_list_reservation(h)) return rc2;
  h->pool_sampled = true;
  h->pool_uniform = true;
  for (int i = 0; i < N; ++i)
    if (pool_len_host[i] != pool_len_host[0] || pool_base_host[i] != i * pool_len_host[0]) h->pool_uniform = false;
  return SWB_OK;
}

// swb_sample_tree_kernel over the whole pool (swb_sample_pool_tree), or over all but the live entries (swb_resample_pool).
int launch_tree_sampler(swb_engine* h, uint64_t seed, uint64_t first_entry, bool skip_live, hipStream_t st) {
  HIP_TRY(hipMemsetAsync(h->d_exhausted, 0, sizeof(unsigned long long), st));
  const swb_tree_args a = {sampler_args(h, seed, first_entry, skip_live), h->d_tree, h->keyed ? h->d_p_cell_label.ptr : nullptr,
                           h->d_exhausted};
  hipLaunchKernelGGL(swb_sample_tree_kernel, dim3((h->pool_entries + 255) / 256), dim3(256), 0, st, a);
  HIP_TRY(hipGetLastError());
  return SWB_OK;
}

bool cdf_ok(const double* cdf, int n) {
  for (int i = 0; i < n; ++i)
    if (!(cdf[i] >= (i ? cdf[i - 1] : 0.0)) || !(cdf[i] <= 1.0)) return false;
  return true;
}

// Everything swb_sample_tree_kernel relies on (include/swb.h, swb_sample_pool_tree): indices, jumps, stack depths, factor kinds.
int check_tree_sampler(const swb_engine* h, const swb_tree_sampler* sp) {
  if (sp->n_groups < 1 || sp->n_groups > SWB_MAX_GROUPS) return fail(SWB_ERR_INVALID, "n_groups must be in [1, %d]", SWB_MAX_GROUPS);
  if (sp->shuffle < 0) return fail(SWB_ERR_INVALID, "shuffle must be >= 0");
  if (sp->max_tries < 1) return fail(SWB_ERR_INVALID, "max_tries must be >= 1");
  if (sp->n_tasks != h->p.n_tasks) return fail(SWB_ERR_INVALID, "the sampler labels %d tasks, the handle has %d", sp->n_tasks, h->p.n_tasks);
  if (sp->n_leaves < 0 || sp->n_leaves > SWB_TREE_MAX_LEAVES) return fail(SWB_ERR_INVALID, "at most %d leaves", SWB_TREE_MAX_LEAVES);
  if (sp->n_pred_nodes < 0 || sp->n_pred_nodes > SWB_TREE_MAX_PRED_NODES)
    return fail(SWB_ERR_INVALID, "at most %d predicate nodes", SWB_TREE_MAX_PRED_NODES);
  if (sp->n_preds < 0 || sp->n_preds > SWB_TREE_MAX_PREDS) return fail(SWB_ERR_INVALID, "at most %d predicates", SWB_TREE_MAX_PREDS);
  if (sp->n_ops < 0 || sp->n_ops > SWB_TREE_MAX_OPS) return fail(SWB_ERR_INVALID, "at most %d ops", SWB_TREE_MAX_OPS);
  if (sp->n_choices < 0 || sp->n_choices > SWB_TREE_MAX_CHOICES) return fail(SWB_ERR_INVALID, "at most %d choices", SWB_TREE_MAX_CHOICES);
  if (sp->n_alternatives < 0 || sp->n_alternatives > SWB_MAX_ALTERNATIVES)
    return fail(SWB_ERR_INVALID, "n_alternatives must be in [0, %d]", SWB_MAX_ALTERNATIVES);
  for (int i = 0; i < sp->n_alternatives; ++i) {
    const swb_alternative& alt = sp->alternatives[i];
    if (alt.n < 1 || alt.n > SWB_MAX_GROUPS) return fail(SWB_ERR_INVALID, "alternative %d: 1..%d groups", i, SWB_MAX_GROUPS);
    for (int g = 0; g < alt.n; ++g)
      if (alt.group[g] < 0 || alt.group[g] >= sp->n_groups) return fail(SWB_ERR_INVALID, "alternative %d: bad group index", i);
  }
  if (sp->alternatives_weighted && (sp->n_alternatives < 1 || !cdf_ok(sp->alternative_cdf, sp->n_alternatives)))
    return fail(SWB_ERR_INVALID, "alternative_cdf must be non-decreasing within [0, 1]");
  for (int i = 0; i < sp->n_leaves; ++i) {
    const swb_tree_leaf& lf = sp->leaves[i];
    if (lf.factor < 0 || lf.factor >= SWB_TREE_N_FACTORS) return fail(SWB_ERR_INVALID, "leaf %d: bad factor index", i);
    if (lf.kind < SWB_FACTOR_UNIFORM_F32 || lf.kind > SWB_FACTOR_DISCRETE) return fail(SWB_ERR_INVALID, "leaf %d: bad kind", i);
    if (lf.kind == SWB_FACTOR_DISCRETE && (lf.n < 1 || lf.n > SWB_MAX_CANDIDATES))
      return fail(SWB_ERR_INVALID, "leaf %d: Discrete leaves take 1..%d candidates", i, SWB_MAX_CANDIDATES);
    if (lf.kind == SWB_FACTOR_DISCRETE && lf.weighted && !cdf_ok(lf.cdf, lf.n))
      return fail(SWB_ERR_INVALID, "leaf %d: cdf must be non-decreasing within [0, 1]", i);
    if (lf.factor == SWB_F_SHAPE) {
      if (lf.kind != SWB_FACTOR_DISCRETE) return fail(SWB_ERR_INVALID, "leaf %d: shape must be a Discrete leaf", i);
      for (int k = 0; k < lf.n; ++k)
        if (!(lf.cand[k] >= 0.0 && lf.cand[k] < (double)SWB_MAX_SHAPES && lf.cand[k] == (double)(int)lf.cand[k]))
          return fail(SWB_ERR_INVALID, "leaf %d: bad shape index", i);
    }
  }
  for (int i = 0; i < sp->n_preds; ++i) {
    const swb_tree_pred& pr = sp->preds[i];
    if (pr.first < 0 || pr.n < 1 || pr.first + pr.n > sp->n_pred_nodes) return fail(SWB_ERR_INVALID, "predicate %d: nodes out of range", i);
    int depth = 0;
    for (int k = pr.first; k < pr.first + pr.n; ++k) {
      const swb_pred_node& nd = sp->pred_nodes[k];
      if (nd.op == SWB_PRED_LEAF) {
        if (nd.leaf < 0 || nd.leaf >= sp->n_leaves) return fail(SWB_ERR_INVALID, "predicate %d: bad leaf index", i);
        ++depth;
      } else if (nd.op == SWB_PRED_TRUE) {
        ++depth;
      } else if (nd.op == SWB_PRED_AND || nd.op == SWB_PRED_OR || nd.op == SWB_PRED_ANDNOT) {
        if (depth < 2) return fail(SWB_ERR_INVALID, "predicate %d: stack underflow at node %d", i, k - pr.first);
        --depth;
      } else {
        return fail(SWB_ERR_INVALID, "predicate %d: bad op", i);
      }
      if (depth > SWB_TREE_MAX_STACK) return fail(SWB_ERR_INVALID, "predicate %d: stack deeper than %d", i, SWB_TREE_MAX_STACK);
    }
    if (depth != 1) return fail(SWB_ERR_INVALID, "predicate %d leaves %d values on the stack", i, depth);
  }
  for (int t = 0; t < sp->n_tasks; ++t) {
    const swb_tree_task& tk = sp->tasks[t];
    if (tk.kind != h->cfg.tasks[t].kind) return fail(SWB_ERR_INVALID, "task %d: kind differs from the handle's", t);
    if (tk.n_preds < 0 || tk.n_preds > SWB_TREE_MAX_CLUSTERS || (tk.kind == SWB_TASK_FIND_GOAL && tk.n_preds > 1))
      return fail(SWB_ERR_INVALID, "task %d: bad predicate count", t);
    for (int k = 0; k < tk.n_preds; ++k)
      if (tk.pred[k] < 0 || tk.pred[k] >= sp->n_preds) return fail(SWB_ERR_INVALID, "task %d: bad predicate index", t);
  }
  for (int i = 0; i < sp->n_choices; ++i) {
    const swb_tree_choice& ch = sp->choices[i];
    if (ch.n < 1 || ch.n > SWB_MAX_CANDIDATES || !cdf_ok(ch.cdf, ch.n))
      return fail(SWB_ERR_INVALID, "choice %d: 1..%d targets, cdf non-decreasing within [0, 1]", i, SWB_MAX_CANDIDATES);
  }
  for (int g = 0; g < sp->n_groups; ++g) {
    const swb_tree_group& grp = sp->groups[g];
    if (grp.count_min < 0 || grp.count_max < grp.count_min) return fail(SWB_ERR_INVALID, "group %d: bad sprite count range", g);
    if (grp.first_op < 0 || grp.n_ops < 0 || grp.first_op + grp.n_ops > sp->n_ops) return fail(SWB_ERR_INVALID, "group %d: program out of range", g);
    const double dsh = grp.defaults[SWB_F_SHAPE];
    if (!(dsh >= 0.0 && dsh < (double)SWB_MAX_SHAPES && dsh == (double)(int)dsh)) return fail(SWB_ERR_INVALID, "group %d: bad default shape", g);
    const int end = grp.first_op + grp.n_ops;
    bool draws_x = false, draws_y = false;
    for (int pc = grp.first_op; pc < end; ++pc) {
      const swb_tree_op& op = sp->ops[pc];
      if (op.kind == SWB_OP_DRAW) {
        if (op.a < 0 || op.a >= sp->n_leaves) return fail(SWB_ERR_INVALID, "group %d, op %d: bad leaf index", g, pc);
        const swb_tree_leaf& lf = sp->leaves[op.a];
        if (lf.factor == SWB_F_X || lf.factor == SWB_F_Y) {
          if (lf.kind != SWB_FACTOR_UNIFORM_F32) return fail(SWB_ERR_INVALID, "group %d: x and y must be float32 Continuous factors", g);
          (lf.factor == SWB_F_X ? draws_x : draws_y) = true;
        }
        if (lf.factor == SWB_F_ANGLE && (lf.kind == SWB_FACTOR_UNIFORM_F32 ||
                                        (lf.kind == SWB_FACTOR_UNIFORM_INT && !(lf.lo >= 0.0 && lf.hi <= 360.0 && lf.lo <= lf.hi))))
          return fail(SWB_ERR_INVALID, "group %d: angle must be Discrete or integer degrees within [0, 360]", g);
        if (sp->color_map == 1 && lf.kind == SWB_FACTOR_UNIFORM_INT && lf.factor >= SWB_F_C0 && lf.factor <= SWB_F_C2)
          return fail(SWB_ERR_INVALID, "group %d: hsv colours must be float factors", g);
      } else if (op.kind == SWB_OP_CHOOSE) {
        if (op.a < 0 || op.a >= sp->n_choices) return fail(SWB_ERR_INVALID, "group %d, op %d: bad choice index", g, pc);
        const swb_tree_choice& ch = sp->choices[op.a];
        for (int k = 0; k < ch.n; ++k)
          if (ch.target[k] <= pc || ch.target[k] > end) return fail(SWB_ERR_INVALID, "group %d, op %d: choice target %d outside (%d, %d]", g, pc, ch.target[k], pc, end);
      } else if (op.kind == SWB_OP_JUMP) {
        if (op.a > end) return fail(SWB_ERR_INVALID, "group %d, op %d: jump to %d, outside the program [%d, %d]", g, pc, op.a, grp.first_op, end);
        if (op.a <= pc) return fail(SWB_ERR_INVALID, "group %d, op %d: backward JUMP to %d (only TEST goes back)", g, pc, op.a);
      } else if (op.kind == SWB_OP_TEST) {
        if (op.a < 0 || op.a >= sp->n_preds) return fail(SWB_ERR_INVALID, "group %d, op %d: bad predicate index", g, pc);
        if (op.c < grp.first_op || op.c > pc) return fail(SWB_ERR_INVALID, "group %d, op %d: TEST retries at %d, outside [%d, %d]", g, pc, op.c, grp.first_op, pc);
      } else {
        return fail(SWB_ERR_INVALID, "group %d, op %d: bad op kind", g, pc);
      }
    }
    if (!draws_x || !draws_y) return fail(SWB_ERR_INVALID, "group %d: x and y must be float32 Continuous factors", g);
  }
  return 0;
}

}  // namespace

extern "C" {

const char* swb_last_error(void) { return g_err.c_str(); }
int swb_version(void) { return 1; }

int swb_create(const swb_config* cfg, int device, swb_handle* out) {
  if (!cfg || !out) return fail(SWB_ERR_INVALID, "null argument");
  if (cfg->n_envs < 1) return fail(SWB_ERR_INVALID, "n_envs must be >= 1");
  if (cfg->max_sprites < 1 || cfg->max_sprites > SWB_MAX_SPRITES)
    return fail(SWB_ERR_INVALID, "max_sprites must be in [1, %d] (at most %d sprites per environment)", SWB_MAX_SPRITES, SWB_MAX_SPRITES);
  if (cfg->n_tasks < 1 || cfg->n_tasks > SWB_MAX_TASKS) return fail(SWB_ERR_INVALID, "n_tasks must be in [1, %d]", SWB_MAX_TASKS);
  if (cfg->anti_aliasing < 1) return fail(SWB_ERR_INVALID, "anti_aliasing must be >= 1");
  if (cfg->image_h < 1 || cfg->image_w < 1 || (cfg->image_h % 4) != 0)
    return fail(SWB_ERR_INVALID, "image_size[0] must be a positive multiple of 4");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(SWB_ERR_NO_DEVICE, "no HIP device visible");
  if (device < 0 || device >= ndev) return fail(SWB_ERR_NO_DEVICE, "device %d out of range (%d devices)", device, ndev);
  HIP_TRY(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(SWB_ERR_NO_DEVICE, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
  // (a refusal below frees whatever the handle holds by then: it is the caller's only once *out is set)
  std::unique_ptr<swb_engine> owner(new swb_engine());
  swb_engine* const h = owner.get();
  h->cfg = *cfg;
  h->device = device;
  HIP_TRY(hipDeviceGetAttribute(&h->cus, hipDeviceAttributeMultiprocessorCount, device));
  h->no_paint_in_cover = getenv("SWB_NO_PAINT_IN_COVER") != nullptr;
  h->force_cover_order = getenv("SWB_COVER_ORDER") != nullptr;
  h->no_keep_lists = getenv("SWB_NO_KEEP_LISTS") != nullptr;
  swb_params& p = h->p;
  memset(&p, 0, sizeof(p));
  p.N = cfg->n_envs; p.S = cfg->max_sprites; p.AA = cfg->anti_aliasing;
  // The reference makes the PIL canvas of *size* (AA*image_size[0], AA*image_size[1]) = (width, height)
  // (pil_renderer.py:50-51,64); np.array(image) is then [image_size[1], image_size[0], 3].
  p.Wo = cfg->image_h; p.Ho = cfg->image_w;
  p.Wc = p.AA * p.Wo; p.Hc = p.AA * p.Ho;
  p.bg = (uint32_t)cfg->bg_rgb[0] | ((uint32_t)cfg->bg_rgb[1] << 8) | ((uint32_t)cfg->bg_rgb[2] << 16);
  p.action_space = cfg->action_space; p.keep_in_frame = cfg->keep_in_frame;
  p.max_episode_length = cfg->max_episode_length; p.pos_is_f32 = cfg->pos_is_f32;
  p.action_is_f32 = cfg->action_is_f32;
  p.action_scale = cfg->action_scale; p.motion_cost = cfg->motion_cost;
  p.n_tasks = cfg->n_tasks; p.is_meta = cfg->is_meta; p.meta_aggregator = cfg->meta_aggregator;
  p.meta_termination = cfg->meta_termination; p.meta_terminate_bonus = cfg->meta_terminate_bonus;
  memcpy(p.tasks, cfg->tasks, sizeof(p.tasks));
  for (int t = 0; t < cfg->n_tasks; ++t) {
    const swb_task& tk = cfg->tasks[t];
    if (tk.n_xcuts < 0 || tk.n_xcuts > SWB_MAX_CUTS || tk.n_ycuts < 0 || tk.n_ycuts > SWB_MAX_CUTS)
      return fail(SWB_ERR_INVALID, "task %d: between 0 and %d position thresholds per axis supported", t, SWB_MAX_CUTS);
    for (int k = 1; k < tk.n_xcuts; ++k) if (!(tk.xcuts[k - 1] < tk.xcuts[k])) return fail(SWB_ERR_INVALID, "task %d: xcuts must ascend", t);
    for (int k = 1; k < tk.n_ycuts; ++k) if (!(tk.ycuts[k - 1] < tk.ycuts[k])) return fail(SWB_ERR_INVALID, "task %d: ycuts must ascend", t);
    if (tk.n_xcuts + tk.n_ycuts > 0) h->keyed = true;
  }
  // frames the tuned kernels cannot take (a canvas wider than the widest cover build, more than SWB_MAX_CG column groups) go
  // the large-frame path; SWB_LARGE_FRAMES=1 (tests) sends every geometry there
  {
    const char* lf = getenv("SWB_LARGE_FRAMES");
    const char* ms = getenv("SWB_MANY_SPRITES");
    // (more sprites than the tuned kernels are built for: the many-sprite state kernel, then the large-frame render kernels;
    // SWB_MANY_SPRITES=1, tests, sends every handle there)
    h->many_sprites = p.S > SWB_TUNED_SPRITES || (ms && atoi(ms) != 0);
    h->large_frames = !pick_variant(p.Wc) || p.Wo > 64 * SWB_MAX_CG || (lf && atoi(lf) != 0) || h->many_sprites;
    if (const char* x = getenv("SWB_LF_SCRATCH_BYTES")) h->lf_scratch_budget = (size_t)std::max(1ll, atoll(x));   // tests: force chunks
  }
  if (h->large_frames) {
    if (p.Wc > SWB_LF_MAX_CANVAS || p.Hc > SWB_LF_MAX_CANVAS)
      return fail(SWB_ERR_INVALID, "canvas %dx%d too large: at most %d px in either direction (anti_aliasing * image_size)", p.Wc, p.Hc,
                  SWB_LF_MAX_CANVAS);
    if (p.Wo > SWB_LF_MAX_COLUMNS) return fail(SWB_ERR_INVALID, "image width %d too large: at most %d columns", p.Wo, SWB_LF_MAX_COLUMNS);
  } else if (p.Hc > 65535) {
    return fail(SWB_ERR_INVALID, "canvas %dx%d too large", p.Wc, p.Hc);
  }
  // groups of 64 output columns (the kernels of the large-frame path know none: swb_params::ncg stays 0 there)
  const int ncg = (p.Wo + 63) / 64;
  if (!h->large_frames) p.ncg = ncg;
  const int cus = std::max(h->cus, 1);
  // Bands of output rows per (environment, column group) in the second kernel: a band repeats the 25 canvas rows it
  // shares with the band above, so there are only as many as it takes to give every SIMD its eight waves (small
  // batches), in bands of at least 16 rows -- of 8 rows where those fill the SIMDs no more than once (measured, 64-px images:
  // 512 environments 0.0311 ms in 8 bands against 0.0354 in 4; 1024 environments, every band a task of its own (band_tasks
  // below), 0.0342 against 0.0366; 2048 environments 0.0498 against 0.0422: profiles/r06_experiments/bands_small_batches.txt).
  {
    const long long resident = (long long)cus * 4 * SWB_RS_WAVES_PER_SIMD;
    const long long tasks = (long long)p.N * ncg;
    int nb = 1;
    while (nb < SWB_MAX_BANDS && tasks * nb < resident && (p.Ho / (2 * nb) >= 16 || (p.Ho / (2 * nb) >= 8 && tasks * nb * 2 <= resident))) nb *= 2;
    if (const char* x = getenv("SWB_BANDS")) nb = std::max(1, std::min(atoi(x), (int)SWB_MAX_BANDS));
    h->nbands = std::min(nb, p.Ho);
    // Split bands (swb_params::split_bands): a batch whose rule gives ONE band but whose launch is at most two
    // rounds of resident waves builds its lists and tables for SWB_SPLIT_BANDS_DEFAULT bands all the same, and every launch decides on
    // the device which environments use them -- those that resample or fill, when few enough do that the launch ends with its
    // last resampling wave.  Only handles that will own a frame cache (the copies stay whole) and dispatch by cost; not under
    // SWB_BANDS, not in the Embodied action space.  SWB_SPLIT_BANDS=n (tests, A/B runs): 0 never, n >= 2 the mode with n bands at any batch size.
    const bool cache_wanted = p.AA != 1 && !h->large_frames && !h->no_keep_lists && !getenv("SWB_NO_FRAME_CACHE");
    const bool cost_ordered = !getenv("SWB_NO_COST_ORDER") && p.N < (1 << 24) && !h->large_frames;
    // (not in the Embodied action space, where the agent's body moves at nearly every step: `embodied_s12` keeps 6 % of its lists,
    // copies nothing and never splits, and the band starts in 7 700 lists a launch made its cover kernel 2 % longer.  A proxy for
    // "almost nothing is kept", not a measure: a batch of another action space whose sprites all move at every step still takes the
    // mode and pays that; an Embodied batch with long still periods gets it only through SWB_SPLIT_BANDS.)
    int split = (nb == 1 && tasks <= 2 * resident && p.action_space != SWB_ACTION_EMBODIED) ? SWB_SPLIT_BANDS_DEFAULT : 0;
    if (const char* x = getenv("SWB_SPLIT_BANDS")) split = atoi(x) >= 2 ? std::min(atoi(x), (int)SWB_MAX_BANDS) : 0;
    if (getenv("SWB_BANDS") || !cache_wanted || !cost_ordered || std::min(split, p.Ho) < 2) split = 0;
    if (split) {
      h->split_bands = true;
      h->nbands = std::min(split, p.Ho);
      p.split_bands = 1;
      // the threshold, in frames that resampled or filled in the previous launch: two per SIMD (swept: profiles/r20_split_bands.md)
      p.split_when = 2 * cus * 4;
      if (const char* x = getenv("SWB_SPLIT_WHEN")) p.split_when = (int32_t)std::max(0ll, std::min(atoll(x), 0x7fffffffll));
    }
  }
  // waves of the second kernel: one per (environment, column group, band) -- split bands: counted at the nominal one band, what
  // decides priorities and dealing below is the launch the batch rule saw
  const long long rs_waves = (long long)p.N * ncg * (h->split_bands ? 1 : h->nbands);
  // cost buckets of the second kernel's tasks: 32 of them over the cost of a run list (3 per run + 2 per 8-byte unit: a canvas row
  // costs 1 unit (one span), 2 (two or three) or more, and rows that repeat the row above nothing); the range they span is
  // fitted by every launch (cost_housekeeping), to begin with it is [0, 8 * canvas height)
  p.cost_range0 = std::max(8 * p.Hc, SWB_KEY_BUCKETS_FITTED);      // (a run and its units cost 5 .. 9; a launch later the range is a measured one)
  if (!getenv("SWB_NO_COST_ORDER") && p.N < (1 << 24) && !h->large_frames) {
    // Small batches in several bands: a task of the second kernel is one BAND of a list, filed under the band's own cost, once
    // the launch has four waves or more per SIMD to deal (measured, resample / fill kernel: 2048 environments in 4 bands -9.5 %,
    // 1024 -2 %, a 128x128 image at anti_aliasing = 1 -22 %; two waves per SIMD, 256 environments in 8 bands, +3 %:
    // profiles/r06_experiments/band_tasks_ab.txt).
    p.band_tasks = (h->nbands > 1 && rs_waves >= 4ll * cus * 4 && !getenv("SWB_NO_BAND_TASKS")) ? 1 : 0;
    if (const char* x = getenv("SWB_BAND_TASKS")) p.band_tasks = (h->nbands > 1 && atoi(x) != 0) ? 1 : 0;      // tests
    // (split bands: the tasks are band tasks or whole ones; lists and grid hold the worst case, every environment in bands --
    // any launch can meet a step in which all of them build)
    if (h->split_bands) p.band_tasks = 1;
    p.cost_cap = ncg * ((p.N + SWB_COST_SHARDS - 1) / SWB_COST_SHARDS) * (p.band_tasks ? h->nbands : 1);
    std::vector<uint32_t> cnt0(5 * SWB_COST_SET + SWB_COST_WORDS, 0u);
    // (split bands: the first launch decides as if every frame had resampled in the one before it)
    for (int par = 0; par < 2; ++par) cnt0[SWB_COST_WORD_SPLIT(par)] = (h->split_bands && p.split_when > 0 && (long long)p.N * ncg <= p.split_when) ? 1u : 0u;
    for (int ph = 0; ph < 3; ++ph) cnt0[SWB_COST_WORD_COVER_SHIFT(ph)] = 12;   // bucket width of the cover kernel's cycle counts: 2^12 to begin with
    for (int par = 0; par < 2; ++par) {                                       // buckets of the second kernel's tasks: [0, cost_range0) to begin with
      cnt0[SWB_COST_WORD_KEY_LO(par)] = 0u;
      cnt0[SWB_COST_WORD_KEY_RANGE(par)] = (uint32_t)p.cost_range0;
      cnt0[SWB_COST_WORD_KEY_SCALE(par)] = (uint32_t)(((unsigned long long)SWB_KEY_BUCKETS_FITTED << 16) / (uint32_t)p.cost_range0);
    }
    p.prio_div = 4;              // (measured: levels of a quarter of a mean wave 2 % better than of half a wave, at 8192 environments)
    if (const char* x = getenv("SWB_PRIO_DIV")) p.prio_div = std::max(1, atoi(x));
    // (priorities when the launch is at most two rounds of resample waves: in steady state they cost 0.8 %)
    p.prio_levels = (!getenv("SWB_NO_PRIO") && rs_waves <= 2ll * cus * 4 * SWB_RS_WAVES_PER_SIMD) ? 1 : 0;
    if (!getenv("SWB_NO_COVER_PRIO")) p.prio_levels |= 2;          // (cover waves: only ever used with cover_order)
    const size_t ccap = (size_t)(p.N + SWB_COST_SHARDS - 1) / SWB_COST_SHARDS;
    if (h->d_cost_cnt.fill(cnt0.data(), cnt0.size()) ||
        h->d_ccost_list.fill(nullptr, (size_t)3 * SWB_COST_SHARDS * SWB_COST_BUCKETS * ccap) ||
        h->d_cost_list.fill(nullptr, (size_t)2 * SWB_COST_SHARDS * SWB_COST_BUCKETS * p.cost_cap))
      return SWB_ERR_HIP;
    p.cost_cnt = h->d_cost_cnt; p.cost_list = h->d_cost_list;
    if (!getenv("SWB_NO_COVER_ORDER")) p.ccost_list = h->d_ccost_list;
    // rounds of the dealing = the compute units of an XCD (8 XCDs; a power of two on this part: 32)
    const int per_xcd = h->cus / SWB_COST_SHARDS;
    // (only when every wave of the launch is resident at once: with several rounds of waves the heaviest tasks must simply
    // come first -- measured on two rounds: +1...2 % with alternating rounds)
    if (per_xcd >= 2 && (per_xcd & (per_xcd - 1)) == 0 && rs_waves <= (long long)h->cus * 4 * SWB_RS_WAVES_PER_SIMD && !getenv("SWB_NO_SNAKE"))
      while ((1 << p.deal_shift) < per_xcd) ++p.deal_shift;
    if (const char* x = getenv("SWB_DEAL_SHIFT")) p.deal_shift = std::max(0, atoi(x));      // tests: short rounds on small batches
  }
  // Run lists, in 8-byte units.  A canvas row of s >= 2 visible spans costs 1 + s / 2 units and S convex sprites leave at most
  // 2 S - 1 spans in a row: (S + 1) units per row hold any scene of convex sprites even if no two rows fold into a run.  That is
  // what every list reserves to BEGIN with (round 5: ten sprites on a 60-row canvas needed 4.5 units per row) -- 133 KB per
  // environment on 12 sprites at 128x128, a tenth of it used.  swb_trim_run_lists() then cuts the lists' own (fixed) parts down to
  // 1.25 x the longest list the launches so far wrote and adds a shared ARENA from which a list that outgrows its part continues
  // by atomic bump (swb_params::run_cap); only a scene that finds the arena exhausted too is flagged (SWB_ENV_ERR_SPAN_OVERFLOW,
  // its frame short of a batch of rows) -- never silently.  A new pool (swb_set_pool / swb_sample_pool) restores the reservation.
  h->run_cap_worst = std::max(4, p.S + 1) * p.Hc + 1;
  p.run_cap = h->run_cap_worst;
  if (const char* x = getenv("SWB_RUN_CAP")) p.run_cap = std::max(8, atoi(x));      // tests
  if (const char* x = getenv("SWB_ARENA_UNITS")) h->arena_override = std::max(0, atoi(x));   // tests (0: no arena)
  const size_t NS = (size_t)p.N * p.S;
  if (h->d_x.fill(nullptr, NS) || h->d_y.fill(nullptr, NS) || h->d_nspr.fill(nullptr, p.N) || h->d_entry.fill(nullptr, p.N) ||
      h->d_step_count.fill(nullptr, p.N) || h->d_episode.fill(nullptr, p.N) || h->d_reset_next.fill(nullptr, p.N))
    return SWB_ERR_HIP;
  if (getenv("SWB_LIST_STATS")) {
    if (h->d_list_stats.fill(nullptr, 2) || h->d_frame_stats.fill(nullptr, 7) || h->d_task_stats.fill(nullptr, 2)) return SWB_ERR_HIP;
    p.list_stats = h->d_list_stats;
    p.frame_stats = h->d_frame_stats;
    if (h->split_bands) {
      if (h->d_split_stats.fill(nullptr, 3)) return SWB_ERR_HIP;
      p.split_stats = h->d_split_stats;
    }
  }
  // The frame cache: N frames, for the handles whose frames the resample kernel computes from lists that can be kept -- not the
  // fill kernel and the painting builds (anti_aliasing = 1), not the large-frame and many-sprite paths, not SWB_NO_KEEP_LISTS.
  // A handle that cannot have the memory runs without it (every wave resamples, as before): no error, and none left behind.
  // SWB_SPEC_COPY (tests): `first` puts the cover launch's copy workgroups in front of the state workgroups -- the order in which
  // every one of them reads the word the previous launch left; `behind` is the default
  if (const char* x = getenv("SWB_SPEC_COPY")) {
    if (!strcmp(x, "first")) h->spec_copy = 2;
    else if (strcmp(x, "behind")) return fail(SWB_ERR_INVALID, "SWB_SPEC_COPY must be `behind` or `first`, not `%s`", x);
  }
  if (p.AA != 1 && !h->large_frames && !h->no_keep_lists && !getenv("SWB_NO_FRAME_CACHE")) {
    const size_t bytes = (size_t)p.N * p.Wo * p.Ho * 3;
    if (hipMalloc(reinterpret_cast<void**>(&h->d_frame_cache.ptr), bytes) == hipSuccess) {
      h->d_frame_cache.count = bytes;
      p.frame_cache = h->d_frame_cache;
    } else {
      h->d_frame_cache.ptr = nullptr;
      (void)hipGetLastError();
    }
  }
  // The task cache: 16 zeroed bytes per environment, on every path (swb_params::task_cache is bound by bind_step, for steps
  // only).  As above: a handle that cannot have the memory runs without it, no error left behind.
  if (!getenv("SWB_NO_TASK_CACHE")) {
    const size_t bytes = (size_t)p.N * sizeof(swb_task_record);
    if (hipMalloc(reinterpret_cast<void**>(&h->d_task_cache.ptr), bytes) == hipSuccess && hipMemset(h->d_task_cache.ptr, 0, bytes) == hipSuccess) {
      h->d_task_cache.count = (size_t)p.N;
    } else {
      if (h->d_task_cache.ptr) (void)hipFree(h->d_task_cache.ptr);
      h->d_task_cache.ptr = nullptr;
      (void)hipGetLastError();
    }
  }
  p.max_spans = SWB_MIN_SPANS;
  if (const char* ms = getenv("SWB_MAX_SPANS")) p.max_spans = atoi(ms) < SWB_MIN_SPANS ? SWB_MIN_SPANS : atoi(ms);
  p.span_cap = p.max_spans;
  if (const char* sc = getenv("SWB_LDS_SPAN_CAP")) p.span_cap = std::max(0, std::min(atoi(sc), p.max_spans));   // tests
  // visible-span lists: 3 per canvas row in registers, M in LDS, up to ovf_cap more in an HBM slot that a wave
  // takes only when a row of its batch needs it (allocated at the first launch, see ensure_overflow_slots)
  p.ovf_cap = std::min(p.Wc / 2 + 1, 32);
  p.ovf = nullptr;
  p.x = h->d_x; p.y = h->d_y; p.nspr = h->d_nspr; p.entry = h->d_entry; p.step_count = h->d_step_count;
  p.episode = h->d_episode; p.reset_next = h->d_reset_next;
  *out = owner.release();
  return SWB_OK;
}

int swb_destroy(swb_handle h) {
  if (!h) return SWB_OK;
  (void)hipSetDevice(h->device);
  for (auto* list : {&h->events, &h->event_pool})
    for (auto& ev : *list) { (void)hipEventDestroy(ev.e0); (void)hipEventDestroy(ev.e1); (void)hipEventDestroy(ev.e2); }
  delete h;
  return SWB_OK;
}

int swb_upload_shapes(swb_handle h, const double* verts, const int32_t* offsets, int32_t n_shapes) {
  if (!h || !verts || !offsets) return fail(SWB_ERR_INVALID, "null argument");
  bump_state_epochs(h);              // BOTH (the task reads no shape; in doubt)
  if (n_shapes < 1 || n_shapes > SWB_MAX_SHAPES) return fail(SWB_ERR_INVALID, "n_shapes must be in [1, %d]", SWB_MAX_SHAPES);
  HIP_TRY(hipSetDevice(h->device));
  int maxv = 0;
  for (int i = 0; i < n_shapes; ++i) {
    const int n = offsets[i + 1] - offsets[i];
    if (n < 3 || n > SWB_MAX_SHAPE_VERTS) return fail(SWB_ERR_INVALID, "shape %d has %d vertices (3..%d supported)", i, n, SWB_MAX_SHAPE_VERTS);
    if (n > maxv) maxv = n;
  }
  // smallest distance between two vertices of each shape: the kernel's test for "no two vertices
  // of this sprite can land on one canvas pixel" (swb_kernels.hip.inc, build_all_edges)
  std::vector<double> dmin(n_shapes, 0.0);
  for (int i = 0; i < n_shapes; ++i) {
    double best = 1e300;
    for (int a = offsets[i]; a < offsets[i + 1]; ++a)
      for (int b = a + 1; b < offsets[i + 1]; ++b)
        best = std::min(best, std::hypot(verts[2 * a] - verts[2 * b], verts[2 * a + 1] - verts[2 * b + 1]));
    dmin[i] = best;
  }
  // (both small tables are padded to SWB_MAX_SHAPES entries: a cover wave loads them whole, lane i = entry i, beside its first
  // round of loads and looks a sprite's shape up with a cross-lane read -- not with a third dependent round trip to memory)
  dmin.resize(SWB_MAX_SHAPES, 0.0);
  std::vector<int32_t> off_padded(offsets, offsets + n_shapes + 1);
  off_padded.resize(SWB_MAX_SHAPES + 1, offsets[n_shapes]);
  if (h->d_shape_dmin.fill(dmin.data(), dmin.size())) return SWB_ERR_HIP;
  h->p.shape_dmin = h->d_shape_dmin;
  if (h->d_shape_verts.fill(verts, (size_t)offsets[n_shapes] * 2)) return SWB_ERR_HIP;
  if (h->d_shape_off.fill(off_padded.data(), off_padded.size())) return SWB_ERR_HIP;
  h->p.shape_verts = h->d_shape_verts;
  h->p.shape_off = h->d_shape_off;
  h->p.max_verts = maxv;
  h->p.max_edges = maxv * h->p.S;                 // until a pool is installed (then: the pool's largest episode)
  h->shape_nverts.resize(n_shapes);
  for (int i = 0; i < n_shapes; ++i) h->shape_nverts[i] = offsets[i + 1] - offsets[i];
  h->have_shapes = true;
  return SWB_OK;
}

int swb_upload_resample(swb_handle h, int32_t axis, int32_t out_size, int32_t ksize, const int32_t* bounds,
                        const int32_t* coeffs) {
  if (!h || !bounds || !coeffs) return fail(SWB_ERR_INVALID, "null argument");
  bump_list_epoch(h);                // LISTS ONLY (resampling tables: frames, not the state)
  HIP_TRY(hipSetDevice(h->device));
  if (h->large_frames) return upload_resample_large(h, axis, out_size, ksize, bounds, coeffs);
  const swb_params& p = h->p;
  if (axis == 0) {
    if (out_size != p.Wo) return fail(SWB_ERR_INVALID, "horizontal table has %d outputs, image width is %d", out_size, p.Wo);
    // prefix sums, de-duplicated: the interior columns share one vector
    std::vector<int32_t> xmin(out_size), cnt(out_size), tbl(out_size), pfx;
    std::vector<std::vector<int32_t>> uniq;
    std::vector<int32_t> uniq_off;
    for (int o = 0; o < out_size; ++o) {
      xmin[o] = bounds[2 * o]; cnt[o] = bounds[2 * o + 1];
      if (cnt[o] < 0 || cnt[o] > ksize || xmin[o] < 0 || xmin[o] + cnt[o] > p.Wc)
        return fail(SWB_ERR_INVALID, "bad horizontal bounds at %d", o);
      std::vector<int32_t> v(cnt[o] + 1, 0);
      for (int j = 0; j < cnt[o]; ++j) v[j + 1] = v[j] + coeffs[(size_t)o * ksize + j];
      int found = -1;
      for (size_t u = 0; u < uniq.size(); ++u) if (uniq[u] == v) { found = (int)u; break; }
      if (found < 0) { found = (int)uniq.size(); uniq.push_back(v); uniq_off.push_back((int32_t)pfx.size()); pfx.insert(pfx.end(), v.begin(), v.end()); }
      tbl[o] = uniq_off[found];
    }
    if (pfx.size() * 4 > 32 * 1024) return fail(SWB_ERR_INVALID, "horizontal prefix table too large (%zu entries)", pfx.size());
    if (h->d_h_xmin.fill(xmin.data(), xmin.size()) || h->d_h_cnt.fill(cnt.data(), cnt.size()) ||
        h->d_h_tbl.fill(tbl.data(), tbl.size()) || h->d_h_pfx.fill(pfx.data(), pfx.size()))
      return SWB_ERR_HIP;
    h->p.h_xmin = h->d_h_xmin; h->p.h_cnt = h->d_h_cnt; h->p.h_tbl = h->d_h_tbl; h->p.h_pfx = h->d_h_pfx;
    h->p.h_pfx_len = (int32_t)pfx.size();
    h->h_xmin_host = xmin; h->h_cnt_host = cnt;
    h->tables_dirty = true;
    h->have_h = true;
  } else if (axis == 1) {
    if (out_size != p.Ho) return fail(SWB_ERR_INVALID, "vertical table has %d outputs, image height is %d", out_size, p.Ho);
    // v_tab holds two tables of [Hc][SWB_VSLOTS]: output row r accumulates in slot r % 6 (first table,
    // kernels with VS = 6) or r % 8 (second table, VS = 8), so the in-flight rows never move between
    // accumulators; the rows in flight at a canvas row are consecutive, hence in distinct slots.
    const size_t tab_len = (size_t)p.Hc * SWB_VSLOTS;
    std::vector<int32_t> vend(out_size), vtab(2 * tab_len, 0);
    for (int r = 0; r < out_size; ++r) {
      const int ymin = bounds[2 * r], c = bounds[2 * r + 1];
      if (c < 1 || c > ksize || ymin < 0 || ymin + c > p.Hc) return fail(SWB_ERR_INVALID, "bad vertical bounds at %d", r);
      vend[r] = ymin + c - 1;
      if (r > 0 && (vend[r] < vend[r - 1] || ymin < bounds[2 * (r - 1)])) return fail(SWB_ERR_INVALID, "vertical windows are not monotone");
    }
    int used = 1;
    for (int y = 0; y < p.Hc; ++y) {
      int rf = 0;
      while (rf < out_size && vend[rf] < y) ++rf;     // rows completed before canvas row y
      for (int r = 0; r < out_size; ++r) {
        const int ymin = bounds[2 * r];
        if (y < ymin || y > vend[r]) continue;
        const int k = r - rf;
        if (k < 0 || k >= SWB_VSLOTS) return fail(SWB_ERR_INVALID, "more than %d output rows in flight at canvas row %d", SWB_VSLOTS, y);
        const int32_t cf = coeffs[(size_t)r * ksize + (y - ymin)];
        vtab[(size_t)y * SWB_VSLOTS + (r % 6)] = cf;           // only used when used <= 6
        vtab[tab_len + (size_t)y * SWB_VSLOTS + (r % 8)] = cf;
        if (k + 1 > used) used = k + 1;
      }
    }
    // prefix sums over canvas rows of both slot tables: the coefficient sums of a run of rows
    // [y1, y2] that lies between two row completions are pfx[y2 + 1] - pfx[y1]
    const size_t pfx_len = (size_t)(p.Hc + 1) * SWB_VSLOTS;
    std::vector<int32_t> vpfx(2 * pfx_len, 0);
    for (int t = 0; t < 2; ++t)
      for (int y = 0; y < p.Hc; ++y)
        for (int k = 0; k < SWB_VSLOTS; ++k)
          vpfx[t * pfx_len + (size_t)(y + 1) * SWB_VSLOTS + k] =
              vpfx[t * pfx_len + (size_t)y * SWB_VSLOTS + k] + vtab[t * tab_len + (size_t)y * SWB_VSLOTS + k];
    std::vector<int32_t> vend_padded(vend);
    vend_padded.push_back(0x7fffffff); vend_padded.push_back(0x7fffffff);       // the resample kernel loads one row ahead
    if (h->d_v_tab.fill(vtab.data(), vtab.size()) || h->d_v_end.fill(vend_padded.data(), vend_padded.size()) ||
        h->d_v_pfx.fill(vpfx.data(), vpfx.size()))
      return SWB_ERR_HIP;
    h->p.v_tab = h->d_v_tab; h->p.v_end = h->d_v_end; h->p.v_pfx = h->d_v_pfx;
    h->vslots = used;
    h->v_end_host = vend;
    h->v_ymin_host.resize(out_size);
    for (int r = 0; r < out_size; ++r) h->v_ymin_host[r] = bounds[2 * r];
    h->tables_dirty = true;
    h->have_v = true;
  } else {
    return fail(SWB_ERR_INVALID, "axis must be 0 or 1");
  }
  return SWB_OK;
}

int swb_set_pool(swb_handle h, const swb_pool* pool) {
  if (!h || !pool) return fail(SWB_ERR_INVALID, "null argument");
  bump_state_epochs(h);              // BOTH (a new pool: labels and rows in use)
  HIP_TRY(hipSetDevice(h->device));
  const int P = pool->n_entries, S = h->p.S, T = h->p.n_tasks, N = h->p.N;
  if (P < 1) return fail(SWB_ERR_INVALID, "pool is empty");
  for (int i = 0; i < P; ++i)
    if (pool->n_sprites[i] < 0 || pool->n_sprites[i] > S) return fail(SWB_ERR_INVALID, "pool entry %d has %d sprites (max %d)", i, pool->n_sprites[i], S);
  for (int i = 0; i < N; ++i)
    if (pool->pool_len[i] < 1 || pool->pool_base[i] < 0 || pool->pool_base[i] + pool->pool_len[i] > P)
      return fail(SWB_ERR_INVALID, "env %d: pool range [%d, +%d) outside the pool of %d", i, pool->pool_base[i], pool->pool_len[i], P);
  const size_t PS = (size_t)P * S;
  // polygon vertices of the largest episode: sizes the per-wave edge records and centred paths in LDS (checked before anything
  // is installed: a pool the large-frame raster kernel cannot hold is refused here)
  int most_verts = -1;
  if (h->have_shapes) {
    int most = 1;
    for (int e = 0; e < P; ++e) {
      int tot = 0;
      for (int s2 = 0; s2 < pool->n_sprites[e]; ++s2) {
        const int sh = pool->shape[(size_t)e * S + s2];
        if (sh < 0 || sh >= (int)h->shape_nverts.size()) return fail(SWB_ERR_INVALID, "pool entry %d uses shape %d, %zu shapes uploaded", e, sh, h->shape_nverts.size());
        tot += h->shape_nverts[sh];
      }
      most = std::max(most, tot);
    }
    most_verts = (most + 3) & ~3;
    if (int rc = lf_check_vertices(h, most_verts, "swb_set_pool")) return rc;
  }
  std::vector<uint32_t> rgb(PS);
  for (size_t i = 0; i < PS; ++i)
    rgb[i] = (uint32_t)pool->rgb[4 * i] | ((uint32_t)pool->rgb[4 * i + 1] << 8) | ((uint32_t)pool->rgb[4 * i + 2] << 16);
  for (size_t i = 0; i < PS; ++i)
    if (pool->shape[i] < 0 || (h->have_shapes && pool->shape[i] >= SWB_MAX_SHAPES)) return fail(SWB_ERR_INVALID, "bad shape index in pool");
  int rc = 0;
  h->rollout_stale = true;                        // (swb_rollout_frames: a candidate may sit in an entry that is replaced here)
  h->pool_id = next_pool_id();
  rc |= h->d_p_n.fill(pool->n_sprites, P);
  rc |= h->d_p_x.fill(pool->x, PS); rc |= h->d_p_y.fill(pool->y, PS);
  rc |= h->d_p_xv.fill(pool->x_vel, PS); rc |= h->d_p_yv.fill(pool->y_vel, PS);
  rc |= h->d_p_scale.fill(pool->scale, PS); rc |= h->d_p_ca.fill(pool->cos_a, PS); rc |= h->d_p_sa.fill(pool->sin_a, PS);
  rc |= h->d_p_shape.fill(pool->shape, PS);
  rc |= h->d_p_rgb.fill(rgb.data(), PS);
  rc |= h->d_p_label.fill(pool->label, (size_t)P * T * S);
  if (h->keyed) {
    if (!pool->cell_label) return fail(SWB_ERR_INVALID, "a task of this handle keys on position (swb_task::n_xcuts / n_ycuts): swb_pool::cell_label is required");
    rc |= h->d_p_cell_label.fill(pool->cell_label, (size_t)P * T * S * SWB_MAX_CELLS);
  }
  rc |= h->d_p_attr.fill(pool->attr_f32, PS);                          // (NULL: zeros = Python numbers)
  rc |= h->d_pool_base.fill(pool->pool_base, N);
  rc |= h->d_pool_len.fill(pool->pool_len, N);
  if (pool->angle) rc |= h->d_p_angle.fill(pool->angle, PS);
  if (pool->color) rc |= h->d_p_color.fill(pool->color, PS * 3);
  rc |= fill_entry_sets(h, P);                                         // (task sets: every entry in set 0)
  if (rc) return SWB_ERR_HIP;
  bind_pool(h, pool->angle != nullptr, pool->color != nullptr);
  h->pool_entries = P;
  h->pool_sampled = false;
  if (most_verts > 0) h->p.max_edges = most_verts;
  HIP_TRY(hipMemset(h->d_reset_next, 1, N));      // environment.py:70
  HIP_TRY(hipMemset(h->d_episode, 0, sizeof(int32_t) * N));
  HIP_TRY(hipMemset(h->d_step_count, 0, sizeof(int32_t) * N));
  h->have_pool = true;
  if (int rc2 = restore_run_list_reservation(h)) return rc2;
  return SWB_OK;
}

int swb_sample_pool(swb_handle h, const swb_sampler* spec, int32_t n_entries, const int32_t* pool_base_host,
                    const int32_t* pool_len_host, uint64_t seed, uint64_t first_entry, void* stream) {
  if (!h || !spec || !pool_base_host || !pool_len_host) return fail(SWB_ERR_INVALID, "null argument");
  bump_state_epochs(h);              // BOTH (a new pool)
  HIP_TRY(hipSetDevice(h->device));
  const int P = n_entries, S = h->p.S, N = h->p.N;
  if (P < 1) return fail(SWB_ERR_INVALID, "pool is empty");
  if (h->keyed) return fail(SWB_ERR_INVALID, "a task of this handle keys on position: its labels depend on where a sprite is drawn -- sample such "
                            "generators on the host (swb_set_pool with swb_pool::cell_label)");
  if (spec->n_groups < 1 || spec->n_groups > SWB_MAX_GROUPS) return fail(SWB_ERR_INVALID, "n_groups must be in [1, %d]", SWB_MAX_GROUPS);
  if (spec->shuffle < 0) return fail(SWB_ERR_INVALID, "shuffle must be >= 0");
  if (spec->n_alternatives < 0 || spec->n_alternatives > SWB_MAX_ALTERNATIVES)
    return fail(SWB_ERR_INVALID, "n_alternatives must be in [0, %d]", SWB_MAX_ALTERNATIVES);
  for (int i = 0; i < spec->n_alternatives; ++i) {
    const swb_alternative& alt = spec->alternatives[i];
    if (alt.n < 1 || alt.n > SWB_MAX_GROUPS) return fail(SWB_ERR_INVALID, "alternative %d: 1..%d groups", i, SWB_MAX_GROUPS);
    for (int g = 0; g < alt.n; ++g)
      if (alt.group[g] < 0 || alt.group[g] >= spec->n_groups) return fail(SWB_ERR_INVALID, "alternative %d: bad group index", i);
  }
  int max_total = 0;
  for (int g = 0; g < spec->n_groups; ++g) {
    const swb_sprite_group& grp = spec->groups[g];
    if (grp.count_min < 0 || grp.count_max < grp.count_min) return fail(SWB_ERR_INVALID, "group %d: bad sprite count range", g);
    if (grp.n_shapes < 1 || grp.n_shapes > SWB_MAX_CANDIDATES)
      return fail(SWB_ERR_INVALID, "group %d: 1..%d shape candidates", g, SWB_MAX_CANDIDATES);
    for (const swb_factor* f = grp.factors; f != grp.factors + SWB_N_FACTORS; ++f) {
      if (f->kind < SWB_FACTOR_UNIFORM_F32 || f->kind > SWB_FACTOR_DISCRETE) return fail(SWB_ERR_INVALID, "group %d: bad factor kind", g);
      if (f->kind == SWB_FACTOR_DISCRETE && (f->n < 1 || f->n > SWB_MAX_CANDIDATES))
        return fail(SWB_ERR_INVALID, "group %d: Discrete factors take 1..%d candidates", g, SWB_MAX_CANDIDATES);
    }
    if (grp.factors[SWB_F_X].kind != SWB_FACTOR_UNIFORM_F32 || grp.factors[SWB_F_Y].kind != SWB_FACTOR_UNIFORM_F32)
      return fail(SWB_ERR_INVALID, "group %d: x and y must be float32 Continuous factors", g);
    const swb_factor& ang = grp.factors[SWB_F_ANGLE];
    if (ang.kind == SWB_FACTOR_UNIFORM_F32 ||
        (ang.kind == SWB_FACTOR_UNIFORM_INT && !(ang.lo >= 0.0 && ang.hi <= 360.0 && ang.lo <= ang.hi)))
      return fail(SWB_ERR_INVALID, "group %d: angle must be Discrete or integer degrees within [0, 360]", g);
    if (grp.n_holdouts < 0 || grp.n_holdouts > SWB_MAX_HOLDOUTS) return fail(SWB_ERR_INVALID, "group %d: at most %d hold-outs", g, SWB_MAX_HOLDOUTS);
    for (int i = 0; i < grp.n_holdouts; ++i)
      if (grp.holdouts[i].box_mask == 0 || (grp.holdouts[i].box_mask & ~grp.holdouts[i].redraw_mask) ||
          (grp.holdouts[i].redraw_mask >> SWB_N_FACTORS))
        return fail(SWB_ERR_INVALID, "group %d: hold-out keys must be a non-empty subset of the redrawn keys", g);
    if (spec->color_map == 1 && (grp.factors[SWB_F_C0].kind == SWB_FACTOR_UNIFORM_INT || grp.factors[SWB_F_C1].kind == SWB_FACTOR_UNIFORM_INT ||
                                 grp.factors[SWB_F_C2].kind == SWB_FACTOR_UNIFORM_INT))
      return fail(SWB_ERR_INVALID, "group %d: hsv colours must be float factors", g);
    for (int i = 0; i < grp.n_shapes; ++i)
      if (grp.shapes[i] < 0 || grp.shapes[i] >= SWB_MAX_SHAPES) return fail(SWB_ERR_INVALID, "group %d: bad shape index", g);
    max_total += grp.count_max;
  }
  if (spec->n_alternatives > 0) {
    max_total = 0;
    for (int i = 0; i < spec->n_alternatives; ++i) {
      int tot = 0;
      for (int g = 0; g < spec->alternatives[i].n; ++g) tot += spec->groups[spec->alternatives[i].group[g]].count_max;
      if (tot > max_total) max_total = tot;
    }
  }
  if (max_total > S) return fail(SWB_ERR_INVALID, "sampler can emit %d sprites (max_sprites %d)", max_total, S);
  if (h->have_shapes) {       // the most polygon vertices an episode of this sampler can have (LDS sizing)
    auto group_verts = [&](const swb_sprite_group& grp) {
      int mv = 0;
      for (int i = 0; i < grp.n_shapes; ++i)
        if (grp.shapes[i] < (int)h->shape_nverts.size()) mv = std::max(mv, h->shape_nverts[grp.shapes[i]]);
      return mv * grp.count_max;
    };
    int most = 0;
    if (spec->n_alternatives > 0) {
      for (int i = 0; i < spec->n_alternatives; ++i) {
        int tot = 0;
        for (int g = 0; g < spec->alternatives[i].n; ++g) tot += group_verts(spec->groups[spec->alternatives[i].group[g]]);
        most = std::max(most, tot);
      }
    } else {
      for (int g = 0; g < spec->n_groups; ++g) most += group_verts(spec->groups[g]);
    }
    if (int rc = lf_check_vertices(h, (std::max(most, 1) + 3) & ~3, "swb_sample_pool")) return rc;
    h->p.max_edges = (std::max(most, 1) + 3) & ~3;
  }
  for (int i = 0; i < N; ++i)
    if (pool_len_host[i] < 1 || pool_base_host[i] < 0 || pool_base_host[i] + pool_len_host[i] > P)
      return fail(SWB_ERR_INVALID, "env %d: pool range [%d, +%d) outside the pool of %d", i, pool_base_host[i], pool_len_host[i], P);
  if (alloc_sampled_pool(h, P, pool_base_host, pool_len_host) || h->d_sampler.fill(spec, 1)) return SWB_ERR_HIP;
  const swb_sampler_args a = sampler_args(h, seed, first_entry, false);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(swb_sample_pool_kernel, dim3((P + 255) / 256), dim3(256), 0, st, a);
  HIP_TRY(hipGetLastError());
  h->pool_tree = false;
  return finish_sampled_pool(h, pool_base_host, pool_len_host, st);
}

int swb_resample_pool(swb_handle h, uint64_t seed, uint64_t first_entry, void* stream) {
  if (!h) return fail(SWB_ERR_INVALID, "null handle");
  bump_state_epochs(h);              // BOTH (pool rows redrawn)
  if (!h->have_pool || !h->pool_sampled) return fail(SWB_ERR_STATE, "swb_sample_pool has not been called");
  if (!h->pool_uniform)
    return fail(SWB_ERR_STATE, "swb_resample_pool needs the env-major layout pool_base[n] = n * pool_len, equal pool_len");
  HIP_TRY(hipSetDevice(h->device));
  h->rollout_stale = true;      // (swb_rollout_frames: only entries the LIVE environments play are kept, a candidate's may be redrawn)
  h->pool_id = next_pool_id();  // (... and so may the entries a snapshot plays)
  if (h->pool_tree) return launch_tree_sampler(h, seed, first_entry, true, (hipStream_t)stream);
  const swb_sampler_args a = sampler_args(h, seed, first_entry, true);
  hipLaunchKernelGGL(swb_sample_pool_kernel, dim3((h->pool_entries + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return SWB_OK;
}

int swb_sample_pool_tree(swb_handle h, const swb_tree_sampler* spec, int32_t n_entries, const int32_t* pool_base_host,
                         const int32_t* pool_len_host, uint64_t seed, uint64_t first_entry, void* stream) {
  if (!h || !spec || !pool_base_host || !pool_len_host) return fail(SWB_ERR_INVALID, "null argument");
  bump_state_epochs(h);              // BOTH (a new pool)
  HIP_TRY(hipSetDevice(h->device));
  const int P = n_entries, S = h->p.S, N = h->p.N;
  if (P < 1) return fail(SWB_ERR_INVALID, "pool is empty");
  if (!h->cfg.pos_is_f32) return fail(SWB_ERR_INVALID, "the device sampler draws float32 positions (swb_config::pos_is_f32)");
  if (int rc = check_tree_sampler(h, spec)) return rc;
  auto over_lists = [&](auto per_group) {          // the most of a per-group figure an episode can add up to
    int most = 0;
    if (spec->n_alternatives > 0) {
      for (int i = 0; i < spec->n_alternatives; ++i) {
        int tot = 0;
        for (int g = 0; g < spec->alternatives[i].n; ++g) tot += per_group(spec->groups[spec->alternatives[i].group[g]]);
        most = std::max(most, tot);
      }
    } else {
      for (int g = 0; g < spec->n_groups; ++g) most += per_group(spec->groups[g]);
    }
    return most;
  };
  const int max_total = over_lists([](const swb_tree_group& grp) { return grp.count_max; });
  if (max_total > S) return fail(SWB_ERR_INVALID, "sampler can emit %d sprites (max_sprites %d)", max_total, S);
  if (h->have_shapes) {       // the most polygon vertices an episode of this sampler can have (LDS sizing)
    auto verts_of = [&](double shape) { return (int)shape < (int)h->shape_nverts.size() ? h->shape_nverts[(int)shape] : 0; };
    const int most = over_lists([&](const swb_tree_group& grp) {
      int mv = 0;
      bool drawn = false;
      for (int pc = grp.first_op; pc < grp.first_op + grp.n_ops; ++pc) {
        if (spec->ops[pc].kind != SWB_OP_DRAW || spec->leaves[spec->ops[pc].a].factor != SWB_F_SHAPE) continue;
        const swb_tree_leaf& lf = spec->leaves[spec->ops[pc].a];
        for (int i = 0; i < lf.n; ++i) mv = std::max(mv, verts_of(lf.cand[i]));
        drawn = true;
      }
      if (!drawn) mv = verts_of(grp.defaults[SWB_F_SHAPE]);
      return mv * grp.count_max;
    });
    if (int rc = lf_check_vertices(h, (std::max(most, 1) + 3) & ~3, "swb_sample_pool_tree")) return rc;
    h->p.max_edges = (std::max(most, 1) + 3) & ~3;
  }
  for (int i = 0; i < N; ++i)
    if (pool_len_host[i] < 1 || pool_base_host[i] < 0 || pool_base_host[i] + pool_len_host[i] > P)
      return fail(SWB_ERR_INVALID, "env %d: pool range [%d, +%d) outside the pool of %d", i, pool_base_host[i], pool_len_host[i], P);
  auto dev = std::make_unique<swb_tree_dev>();
  memset(dev.get(), 0, sizeof(swb_tree_dev));
  dev->spec = *spec;
  for (int t = 0; t < h->p.n_tasks; ++t) {
    const swb_task& tk = h->cfg.tasks[t];
    dev->n_xcuts[t] = tk.n_xcuts; dev->n_ycuts[t] = tk.n_ycuts;
    for (int k = 0; k < SWB_MAX_CUTS; ++k) { dev->xcuts[t][k] = tk.xcuts[k]; dev->ycuts[t][k] = tk.ycuts[k]; }
  }
  if (alloc_sampled_pool(h, P, pool_base_host, pool_len_host) || h->d_tree.fill(dev.get(), 1) ||
      (!h->d_exhausted && h->d_exhausted.fill(nullptr, 1)))
    return SWB_ERR_HIP;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = launch_tree_sampler(h, seed, first_entry, false, st)) return rc;
  h->pool_tree = true;
  return finish_sampled_pool(h, pool_base_host, pool_len_host, st);
}

int swb_sampler_exhausted(swb_handle h, int64_t* sprites, void* stream) {
  if (!h || !sprites) return fail(SWB_ERR_INVALID, "null argument");
  *sprites = 0;
  if (!h->d_exhausted) return SWB_OK;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  unsigned long long n = 0;
  HIP_TRY(hipMemcpy(&n, h->d_exhausted, sizeof(n), hipMemcpyDeviceToHost));
  *sprites = (int64_t)n;
  return SWB_OK;
}

int swb_get_pool(swb_handle h, const swb_pool* pool) {
  if (!h || !pool) return fail(SWB_ERR_INVALID, "null argument");
  if (!h->have_pool) return fail(SWB_ERR_STATE, "no pool on the device");
  if (pool->n_entries != h->pool_entries) return fail(SWB_ERR_INVALID, "pool has %d entries, not %d", h->pool_entries, pool->n_entries);
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  const int P = h->pool_entries, S = h->p.S, T = h->p.n_tasks, N = h->p.N;
  const size_t PS = (size_t)P * S;
#define SWB_D2H(dst, src, count) \
  if (dst) HIP_TRY(hipMemcpy((void*)(dst), (src), (count) * sizeof(*(src)), hipMemcpyDeviceToHost))
  SWB_D2H(pool->n_sprites, h->d_p_n, (size_t)P);
  SWB_D2H(pool->x, h->d_p_x, PS); SWB_D2H(pool->y, h->d_p_y, PS);
  SWB_D2H(pool->x_vel, h->d_p_xv, PS); SWB_D2H(pool->y_vel, h->d_p_yv, PS);
  SWB_D2H(pool->scale, h->d_p_scale, PS); SWB_D2H(pool->cos_a, h->d_p_ca, PS); SWB_D2H(pool->sin_a, h->d_p_sa, PS);
  SWB_D2H(pool->shape, h->d_p_shape, PS);
  SWB_D2H(pool->label, h->d_p_label, (size_t)P * T * S);
  if (h->keyed) SWB_D2H(pool->cell_label, h->d_p_cell_label, (size_t)P * T * S * SWB_MAX_CELLS);
  SWB_D2H(pool->attr_f32, h->d_p_attr, PS);
  SWB_D2H(pool->pool_base, h->d_pool_base, (size_t)N); SWB_D2H(pool->pool_len, h->d_pool_len, (size_t)N);
  if (h->p.p_angle) SWB_D2H(pool->angle, h->d_p_angle, PS);
  if (h->p.p_color) SWB_D2H(pool->color, h->d_p_color, PS * 3);
  if (pool->rgb) {
    std::vector<uint32_t> rgb(PS);
    HIP_TRY(hipMemcpy(rgb.data(), h->d_p_rgb, PS * 4, hipMemcpyDeviceToHost));
    uint8_t* dst = const_cast<uint8_t*>(pool->rgb);
    for (size_t i = 0; i < PS; ++i) {
      dst[4 * i] = rgb[i] & 255; dst[4 * i + 1] = (rgb[i] >> 8) & 255; dst[4 * i + 2] = (rgb[i] >> 16) & 255; dst[4 * i + 3] = 0;
    }
  }
#undef SWB_D2H
  return SWB_OK;
}

int swb_reset_all(swb_handle h, void* stream) {
  if (!h) return fail(SWB_ERR_INVALID, "null handle");
  bump_list_epoch(h);                // LISTS ONLY (the reset step evaluates the task and leaves a record for the new episode)
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipMemsetAsync(h->d_reset_next, 1, h->p.N, (hipStream_t)stream));
  return SWB_OK;
}

int swb_step(swb_handle h, const void* actions_dev, const swb_outputs* out, void* stream) {
  return swb_step_masked(h, actions_dev, nullptr, out, stream);
}

int swb_step_masked(swb_handle h, const void* actions_dev, const uint8_t* active_dev, const swb_outputs* out, void* stream) {
  if (!h) return fail(SWB_ERR_INVALID, "null handle");
  HIP_TRY(hipSetDevice(h->device));
  return launch(h, actions_dev, out, 0, (hipStream_t)stream, nullptr, active_dev);
}

// (the list epoch stays: the environments marked build their lists at their FIRST step whatever the stamp says, the others go on
// keeping theirs)
int swb_reset_envs(swb_handle h, const uint8_t* mask_dev, void* stream) {
  if (!h) return fail(SWB_ERR_INVALID, "swb_reset_envs: null handle");
  if (!mask_dev) return fail(SWB_ERR_INVALID, "swb_reset_envs: mask is NULL (u8[N] in device memory; swb_reset_all resets every environment)");
  HIP_TRY(hipSetDevice(h->device));
  hipLaunchKernelGGL(swb_reset_envs_kernel, dim3((unsigned)((h->p.N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, h->d_reset_next.ptr,
                     mask_dev, (int)h->p.N);
  HIP_TRY(hipGetLastError());
  return SWB_OK;
}

int swb_render(swb_handle h, uint8_t* obs_dev, void* stream) {
  if (!h || !obs_dev) return fail(SWB_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(h->device));
  swb_outputs out;
  memset(&out, 0, sizeof(out));
  out.obs = obs_dev;
  return launch(h, nullptr, &out, 1, (hipStream_t)stream);
}

int swb_evaluate(swb_handle h, uint8_t* success_dev, void* stream) {
  if (!h || !success_dev) return fail(SWB_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(h->device));
  swb_outputs out;
  memset(&out, 0, sizeof(out));
  out.success = success_dev;
  return launch(h, nullptr, &out, 2, (hipStream_t)stream);
}

// Rollouts (include/swb.h): swb_rollout_fork_kernel copies the live state into the scratch of N * M virtual environments,
// swb_rollout_kernel steps them K times.  Neither touches the live state, the run lists or the dispatch bookkeeping of launch().
#define SWB_ROLLOUT_MAX_VENVS (1 << 24)      // N * M: one workgroup each, and N * M * S fits an int
#define SWB_ROLLOUT_MAX_STEPS (1 << 16)      // K: one copy of swb_params each
// The state arrays of `nv` environments of S sprites in a block of nv * (16 * S + 32) bytes: the rollout's scratch, and the
// staging block of swb_rollout_frames' picked candidates.
static swb_state_view rollout_state_view(unsigned char* base, size_t nv, size_t S) {
  swb_state_view v;
  v.x = reinterpret_cast<double*>(base);
  v.y = v.x + nv * S;
  v.nspr = reinterpret_cast<int32_t*>(v.y + nv * S);
  v.entry = v.nspr + nv; v.step_count = v.entry + nv; v.episode = v.step_count + nv;
  v.pool_base = v.episode + nv; v.pool_len = v.pool_base + nv;
  v.reset_next = reinterpret_cast<uint8_t*>(v.pool_len + nv);      // (nv bytes of the last 8 nv)
  return v;
}
// The trajectory block of swb_rollout_trajectory (swb_rollout_keep::traj): the scratch's arrays with [K][nv] in front, K * nv *
// (16 * S + 24) bytes; pool_base / pool_len are the scratch's own (they do not change during a rollout).
static swb_state_view rollout_trajectory_view(unsigned char* base, size_t K, size_t nv, size_t S, const swb_state_view& scratch) {
  swb_state_view v;
  const size_t e = K * nv;
  v.x = reinterpret_cast<double*>(base);
  v.y = v.x + e * S;
  v.nspr = reinterpret_cast<int32_t*>(v.y + e * S);
  v.entry = v.nspr + e; v.step_count = v.entry + e; v.episode = v.step_count + e;
  v.reset_next = reinterpret_cast<uint8_t*>(v.episode + e);        // (e bytes of the last 8 e)
  v.pool_base = scratch.pool_base; v.pool_len = scratch.pool_len;
  return v;
}
// `v` moved on by `e` environments in the arrays a step writes and by `e_pool` in pool_base / pool_len.
static swb_state_view advanced(swb_state_view v, size_t e, size_t e_pool, size_t S) {
  v.x += e * S; v.y += e * S;
  v.nspr += e; v.entry += e; v.step_count += e; v.episode += e; v.reset_next += e;
  v.pool_base += e_pool; v.pool_len += e_pool;
  return v;
}

// swb_rollout (steps == nullptr, keep == false), swb_rollout_trajectory, swb_rollout_sampled and swb_rollout_guided (`name` is the
// caller's, for the messages).  `sampled` (swb_rollout_sampled; its `actions` is actions_dev): the rollout kernel's builds that
// draw the actions; `guided` (swb_rollout_guided, likewise): the kernels that draw them from a plan.
static int rollout_launch(swb_handle h, const char* name, const void* actions_dev, int32_t M, int32_t K, const swb_rollout_outputs* out,
                          bool keep, const swb_rollout_step_outputs* steps, void* stream, const swb_rollout_sample_args* sampled = nullptr,
                          const swb_rollout_guided_args* guided = nullptr) {
  if (!h) return fail(SWB_ERR_INVALID, "null handle");
  if (M <= 0 || K <= 0) return fail(SWB_ERR_INVALID, "%s: M and K must be positive (M = %d, K = %d)", name, M, K);
  if (!actions_dev) return fail(SWB_ERR_INVALID, "%s: actions is NULL", name);
  const swb_params& p = h->p;
  if ((long long)p.N * M > SWB_ROLLOUT_MAX_VENVS)
    return fail(SWB_ERR_INVALID, "%s: %d environments x %d candidates exceed the grid limit of %d virtual environments", name, p.N, M,
                SWB_ROLLOUT_MAX_VENVS);
  if (K > SWB_ROLLOUT_MAX_STEPS) return fail(SWB_ERR_INVALID, "%s: K = %d exceeds the limit of %d steps", name, K, SWB_ROLLOUT_MAX_STEPS);
  if (keep && (long long)K * p.N * M * p.S > 0x7fffffffll)
    return fail(SWB_ERR_INVALID, "%s: K x N x M x max_sprites = %d x %d x %d x %d does not fit an int (the kept steps are indexed with one)",
                name, K, p.N, M, p.S);
  if (!h->have_shapes) return fail(SWB_ERR_STATE, "swb_upload_shapes has not been called");
  if (!h->have_pool) return fail(SWB_ERR_STATE, "swb_set_pool has not been called");
  if (h->setters)
    return fail(SWB_ERR_STATE, "%s: sprite setters have been called on this handle; rollouts under live overrides are not supported", name);
  if (h->n_sets)
    return fail(SWB_ERR_STATE, "%s: the handle has task sets (swb_set_task_sets); rollouts under task sets are not supported", name);
  HIP_TRY(hipSetDevice(h->device));
  const hipStream_t st = (hipStream_t)stream;
  const size_t NV = (size_t)p.N * M, S = (size_t)p.S;
  const size_t bytes = NV * (16 * S + 32), traj_bytes = keep ? (size_t)K * NV * (16 * S + 24) : 0;
  h->rollout_M = 0;                          // (until both kernels are in the stream, the scratch holds no rollout's end states)
  h->rollout_kept_K = 0;
  if (bytes > h->d_rollout.count || (size_t)K > h->d_rollout_steps.count || traj_bytes > h->d_rollout_traj.count) {
    HIP_TRY(hipStreamSynchronize(st));       // (the one blocking case: an earlier rollout may still use the old buffers)
    if (bytes > h->d_rollout.count && h->d_rollout.fill(nullptr, bytes)) return SWB_ERR_HIP;
    if ((size_t)K > h->d_rollout_steps.count && h->d_rollout_steps.fill(nullptr, K)) return SWB_ERR_HIP;
    if (traj_bytes > h->d_rollout_traj.count && h->d_rollout_traj.fill(nullptr, traj_bytes)) {
      (void)hipGetLastError();               // (not left for the next launch to find: the handle stays usable)
      const std::string why = g_err;
      return fail(SWB_ERR_HIP, "%s: could not allocate %zu bytes for the states of %d steps of %zu virtual environments (%s)", name,
                  traj_bytes, K, NV, why.c_str());
    }
  }
  swb_rollout_args a;
  memset(&a, 0, sizeof(a));
  a.M = M; a.K = K;
  const swb_state_view sv = rollout_state_view(h->d_rollout.ptr, NV, S);
  a.x = sv.x; a.y = sv.y; a.nspr = sv.nspr; a.entry = sv.entry; a.step_count = sv.step_count; a.episode = sv.episode;
  a.pool_base = sv.pool_base; a.pool_len = sv.pool_len; a.reset_next = sv.reset_next;
  a.steps = h->d_rollout_steps;
  a.actions = actions_dev;
  if (out) {
    a.reward = out->reward; a.discount = out->discount; a.step_type = out->step_type; a.success = out->success;
    a.error = out->error; a.out_x = out->x; a.out_y = out->y; a.out_n = out->n_sprites;
  }
  swb_rollout_keep kp;
  memset(&kp, 0, sizeof(kp));
  if (keep) {
    kp.traj = rollout_trajectory_view(h->d_rollout_traj.ptr, (size_t)K, NV, S, sv);
    if (steps) { kp.out_x = steps->x; kp.out_y = steps->y; kp.out_n = steps->n_sprites; }
  }
  const size_t threads = std::max(NV * S, (size_t)K);
  hipLaunchKernelGGL(swb_rollout_fork_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, p, a);
  HIP_TRY(hipGetLastError());
  swb_rollout_sample_args sa;
  memset(&sa, 0, sizeof(sa));
  if (sampled) sa = *sampled;
  const dim3 grid((unsigned)NV), block(SWB_WAVE);
  if (guided) {
    swb_rollout_guided_args ga = *guided;
    ga.N = p.N;
    if (keep) hipLaunchKernelGGL((swb_rollout_guided_kernel<true>), grid, block, sizeof(swb_ms_lds), st, a, p.S, kp, ga);
    else hipLaunchKernelGGL((swb_rollout_guided_kernel<false>), grid, block, sizeof(swb_ms_lds), st, a, p.S, kp, ga);
  } else if (sampled && keep) hipLaunchKernelGGL((swb_rollout_kernel<true, true>), grid, block, sizeof(swb_ms_lds), st, a, p.S, kp, sa);
  else if (sampled) hipLaunchKernelGGL((swb_rollout_kernel<false, true>), grid, block, sizeof(swb_ms_lds), st, a, p.S, kp, sa);
  else if (keep) hipLaunchKernelGGL((swb_rollout_kernel<true, false>), grid, block, sizeof(swb_ms_lds), st, a, p.S, kp, sa);
  else hipLaunchKernelGGL((swb_rollout_kernel<false, false>), grid, block, sizeof(swb_ms_lds), st, a, p.S, kp, sa);
  HIP_TRY(hipGetLastError());
  h->rollout_M = M;
  h->rollout_kept_K = keep ? K : 0;
  h->rollout_stale = false;
  return SWB_OK;
}

int swb_rollout(swb_handle h, const void* actions_dev, int32_t M, int32_t K, const swb_rollout_outputs* out, void* stream) {
  return rollout_launch(h, "swb_rollout", actions_dev, M, K, out, false, nullptr, stream);
}

int swb_rollout_trajectory(swb_handle h, const void* actions_dev, int32_t M, int32_t K, const swb_rollout_outputs* out,
                           const swb_rollout_step_outputs* steps, void* stream) {
  return rollout_launch(h, "swb_rollout_trajectory", actions_dev, M, K, out, true, steps, stream);
}

// A rollout that draws its candidates' actions in the kernel (include/swb.h): rollout_launch with the sampling arguments.
int swb_rollout_sampled(swb_handle h, int32_t mode, uint64_t seed, uint64_t first_env, int32_t M, int32_t K, int32_t keep_steps,
                        const swb_rollout_outputs* out, const swb_rollout_step_outputs* steps, const swb_rollout_sampled_outputs* sampled,
                        void* stream) {
  if (!h) return fail(SWB_ERR_INVALID, "null handle");
  if (mode != SWB_SAMPLE_UNIFORM && mode != SWB_SAMPLE_ON_SPRITE) return fail(SWB_ERR_INVALID, "swb_rollout_sampled: unknown mode %d", mode);
  if (!sampled || !sampled->actions)
    return fail(SWB_ERR_INVALID, "swb_rollout_sampled: sampled->actions is NULL (the drawn actions are a required output)");
  if (mode == SWB_SAMPLE_UNIFORM && (sampled->sprite || sampled->tries))
    return fail(SWB_ERR_INVALID, "swb_rollout_sampled: sprite and tries are outputs of SWB_SAMPLE_ON_SPRITE only");
  if (!keep_steps && steps)
    return fail(SWB_ERR_INVALID, "swb_rollout_sampled: per-step outputs (steps) need keep_steps != 0");
  swb_rollout_sample_args sa;
  memset(&sa, 0, sizeof(sa));
  sa.mode = mode; sa.seed = seed; sa.first_env = first_env;
  sa.actions = sampled->actions; sa.sprite = sampled->sprite; sa.tries = sampled->tries;
  return rollout_launch(h, "swb_rollout_sampled", sampled->actions, M, K, out, keep_steps != 0, steps, stream, &sa);
}

// A rollout that draws its candidates' actions from a plan distribution (include/swb.h): rollout_launch with the plan.  The
// weights are not looked at here (that would synchronise): the kernel's rules make every value of them safe.
int swb_rollout_guided(swb_handle h, const swb_rollout_plan* plan, uint64_t seed, uint64_t first_env, int32_t M, int32_t K,
                       int32_t keep_steps, const swb_rollout_outputs* out, const swb_rollout_step_outputs* steps,
                       const swb_rollout_sampled_outputs* sampled, void* stream) {
  if (!h) return fail(SWB_ERR_INVALID, "null handle");
  if (!plan) return fail(SWB_ERR_INVALID, "swb_rollout_guided: plan is NULL");
  if (!sampled || !sampled->actions)
    return fail(SWB_ERR_INVALID, "swb_rollout_guided: sampled->actions is NULL (the drawn actions are a required output)");
  const bool embodied = h->p.action_space == SWB_ACTION_EMBODIED;
  if (embodied) {
    if (plan->width != 8)
      return fail(SWB_ERR_INVALID, "swb_rollout_guided: width = %d, an Embodied plan has exactly 8 action weights (carry * 4 + direction)",
                  plan->width);
    if (plan->motion_mean || plan->motion_std)
      return fail(SWB_ERR_INVALID, "swb_rollout_guided: motion_mean and motion_std must be NULL for an Embodied action space");
    if (sampled->tries) return fail(SWB_ERR_INVALID, "swb_rollout_guided: tries must be NULL for an Embodied action space (no click is drawn)");
  } else {
    if (plan->width < 1 || plan->width > h->p.S)
      return fail(SWB_ERR_INVALID, "swb_rollout_guided: width = %d is outside [1, %d] (max_sprites)", plan->width, h->p.S);
    if (!plan->motion_mean || !plan->motion_std)
      return fail(SWB_ERR_INVALID, "swb_rollout_guided: motion_mean and motion_std are required (f64[K,N,2] in device memory)");
  }
  if (!keep_steps && steps)
    return fail(SWB_ERR_INVALID, "swb_rollout_guided: per-step outputs (steps) need keep_steps != 0");
  swb_rollout_guided_args ga;
  memset(&ga, 0, sizeof(ga));
  ga.seed = seed; ga.first_env = first_env;
  ga.actions = sampled->actions; ga.sprite = sampled->sprite; ga.tries = sampled->tries;
  ga.cdf = plan->choice_cdf; ga.mean = plan->motion_mean; ga.std = plan->motion_std; ga.W = plan->width;
  return rollout_launch(h, "swb_rollout_guided", sampled->actions, M, K, out, keep_steps != 0, steps, stream, nullptr, &ga);
}

// Frames of a rollout's end states (include/swb.h): render launches of the path the handle renders with, their state pointers
// moved to the scratch -- M chunks of N consecutive virtual environments, what the run lists, dispatch tables and overflow
// slots are sized for --, or one launch on a staging block swb_rollout_pick_kernel gathers the picked candidates into.
int swb_rollout_frames(swb_handle h, int32_t M, const int32_t* cand_dev, uint8_t* obs_dev, uint8_t* error_dev, void* stream) {
  if (!h) return fail(SWB_ERR_INVALID, "null handle");
  if (h->n_sets)
    return fail(SWB_ERR_STATE, "swb_rollout_frames: the handle has task sets (swb_set_task_sets); rollouts under task sets are not supported");
  if (!h->rollout_M) return fail(SWB_ERR_STATE, "swb_rollout_frames: no rollout has run on this handle (swb_rollout first)");
  if (!obs_dev) return fail(SWB_ERR_INVALID, "swb_rollout_frames: obs is NULL");
  if (M != h->rollout_M)
    return fail(SWB_ERR_INVALID, "swb_rollout_frames: M = %d, but the last rollout of this handle had %d candidates", M, h->rollout_M);
  if (h->rollout_stale)
    return fail(SWB_ERR_STATE, "swb_rollout_frames: the pool has changed since the last rollout (swb_set_pool, swb_sample_pool or "
                "swb_resample_pool): its candidates may sit in entries that have been redrawn; roll out again");
  if (h->setters)
    return fail(SWB_ERR_STATE, "swb_rollout_frames: sprite setters have been called on this handle; rollouts under live overrides are not supported");
  if (int rc = check_ready(h, nullptr, 1)) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const hipStream_t st = (hipStream_t)stream;
  const size_t N = (size_t)h->p.N, S = (size_t)h->p.S, frame = (size_t)h->p.Wo * h->p.Ho * 3;
  const swb_state_view all = rollout_state_view(h->d_rollout.ptr, N * M, S);
  swb_outputs out;
  memset(&out, 0, sizeof(out));
  if (cand_dev) {
    const size_t bytes = N * (16 * S + 32);
    if (bytes > h->d_rollout_pick.count) {     // (blocking, once: an earlier call may still use the old block)
      HIP_TRY(hipStreamSynchronize(st));
      if (h->d_rollout_pick.fill(nullptr, bytes)) return SWB_ERR_HIP;
    }
    const swb_state_view picked = rollout_state_view(h->d_rollout_pick.ptr, N, S);
    hipLaunchKernelGGL(swb_rollout_pick_kernel, dim3((unsigned)((N * S + 255) / 256)), dim3(256), 0, st, all, picked, cand_dev, (int)N,
                       (int)S, (int)M);
    HIP_TRY(hipGetLastError());
    out.obs = obs_dev; out.error = error_dev;
    return launch(h, nullptr, &out, 1, st, &picked);
  }
  for (size_t c = 0; c < (size_t)M; ++c) {     // virtual environments [c N, (c + 1) N)
    swb_state_view chunk = all;
    chunk.x += c * N * S; chunk.y += c * N * S;
    chunk.nspr += c * N; chunk.entry += c * N; chunk.step_count += c * N; chunk.episode += c * N;
    chunk.pool_base += c * N; chunk.pool_len += c * N; chunk.reset_next += c * N;
    out.obs = obs_dev + c * N * frame;
    out.error = error_dev ? error_dev + c * N : nullptr;
    if (int rc = launch(h, nullptr, &out, 1, st, &chunk)) return rc;
  }
  return SWB_OK;
}

// Frames of the steps inside a rollout (include/swb.h): swb_rollout_frames' render launches with their state pointers on a slot of
// the trajectory block swb_rollout_trajectory kept -- M chunks of N virtual environments of one step, or a staging block that
// swb_rollout_pick_steps_kernel gathers the picked candidates of one step (N environments) or of every step (K * N) into, drawn N at a time.
int swb_rollout_step_frames(swb_handle h, int32_t M, int32_t step, const int32_t* cand_dev, uint8_t* obs_dev, uint8_t* error_dev,
                            void* stream) {
  if (!h) return fail(SWB_ERR_INVALID, "null handle");
  if (h->n_sets)
    return fail(SWB_ERR_STATE, "swb_rollout_step_frames: the handle has task sets (swb_set_task_sets); rollouts under task sets are not supported");
  if (!h->rollout_M) return fail(SWB_ERR_STATE, "swb_rollout_step_frames: no rollout has run on this handle (swb_rollout_trajectory first)");
  if (!h->rollout_kept_K)
    return fail(SWB_ERR_STATE, "swb_rollout_step_frames: the last rollout of this handle was a plain swb_rollout, which kept no steps "
                "(swb_rollout_trajectory keeps them)");
  if (!obs_dev) return fail(SWB_ERR_INVALID, "swb_rollout_step_frames: obs is NULL");
  if (M != h->rollout_M)
    return fail(SWB_ERR_INVALID, "swb_rollout_step_frames: M = %d, but the last rollout of this handle had %d candidates", M, h->rollout_M);
  const int K = h->rollout_kept_K;
  if (step < SWB_ALL_STEPS || step >= K)
    return fail(SWB_ERR_INVALID, "swb_rollout_step_frames: step = %d is outside [0, %d), the steps of the last rollout (SWB_ALL_STEPS = -1: "
                "every step)", step, K);
  if (step == SWB_ALL_STEPS && !cand_dev)
    return fail(SWB_ERR_INVALID, "swb_rollout_step_frames: SWB_ALL_STEPS needs picked candidates (cand is NULL): loop over the steps for "
                "the frames of all candidates");
  if (h->rollout_stale)
    return fail(SWB_ERR_STATE, "swb_rollout_step_frames: the pool has changed since the last rollout (swb_set_pool, swb_sample_pool or "
                "swb_resample_pool): its candidates may sit in entries that have been redrawn; roll out again");
  if (h->setters)
    return fail(SWB_ERR_STATE, "swb_rollout_step_frames: sprite setters have been called on this handle; rollouts under live overrides are not supported");
  if (int rc = check_ready(h, nullptr, 1)) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const hipStream_t st = (hipStream_t)stream;
  const size_t N = (size_t)h->p.N, S = (size_t)h->p.S, NV = N * M, frame = (size_t)h->p.Wo * h->p.Ho * 3;
  const swb_state_view scratch = rollout_state_view(h->d_rollout.ptr, NV, S);
  const swb_state_view traj = rollout_trajectory_view(h->d_rollout_traj.ptr, (size_t)K, NV, S, scratch);
  swb_outputs out;
  memset(&out, 0, sizeof(out));
  if (cand_dev) {
    const int k0 = step == SWB_ALL_STEPS ? 0 : step, nk = step == SWB_ALL_STEPS ? K : 1;
    const size_t bytes = (size_t)nk * N * (16 * S + 32);
    if (bytes > h->d_rollout_pick.count) {     // (blocking, once: an earlier call may still use the old block)
      HIP_TRY(hipStreamSynchronize(st));
      if (h->d_rollout_pick.fill(nullptr, bytes)) return SWB_ERR_HIP;
    }
    const swb_state_view picked = rollout_state_view(h->d_rollout_pick.ptr, (size_t)nk * N, S);
    hipLaunchKernelGGL(swb_rollout_pick_steps_kernel, dim3((unsigned)(((size_t)nk * N * S + 255) / 256)), dim3(256), 0, st, traj, scratch,
                       picked, cand_dev, (int)N, (int)S, (int)M, k0, nk);
    HIP_TRY(hipGetLastError());
    for (size_t kk = 0; kk < (size_t)nk; ++kk) {   // environments [kk N, (kk + 1) N) of the staging block: step k0 + kk
      const swb_state_view chunk = advanced(picked, kk * N, kk * N, S);
      out.obs = obs_dev + kk * N * frame;
      out.error = error_dev ? error_dev + kk * N : nullptr;
      if (int rc = launch(h, nullptr, &out, 1, st, &chunk)) return rc;
    }
    return SWB_OK;
  }
  for (size_t c = 0; c < (size_t)M; ++c) {     // virtual environments [c N, (c + 1) N) of slot `step`
    const swb_state_view chunk = advanced(traj, (size_t)step * NV + c * N, c * N, S);
    out.obs = obs_dev + c * N * frame;
    out.error = error_dev ? error_dev + c * N : nullptr;
    if (int rc = launch(h, nullptr, &out, 1, st, &chunk)) return rc;
  }
  return SWB_OK;
}

// Random-agent actions (include/swb.h): one kernel that only reads the handle -- not a launch(): no parity, phase or cost list moves.
int swb_sample_actions(swb_handle h, int32_t mode, uint64_t seed, uint64_t first_env, const swb_sampled_actions* out, void* stream) {
  if (!h) return fail(SWB_ERR_INVALID, "null handle");
  if (mode != SWB_SAMPLE_UNIFORM && mode != SWB_SAMPLE_ON_SPRITE) return fail(SWB_ERR_INVALID, "swb_sample_actions: unknown mode %d", mode);
  if (!out || (!out->actions && !out->position && !out->sprite && !out->tries))
    return fail(SWB_ERR_INVALID, "swb_sample_actions: every output is NULL");
  if (mode == SWB_SAMPLE_UNIFORM && (out->position || out->sprite || out->tries))
    return fail(SWB_ERR_INVALID, "swb_sample_actions: position, sprite and tries are outputs of SWB_SAMPLE_ON_SPRITE only");
  if (mode == SWB_SAMPLE_ON_SPRITE) {
    if (!h->have_shapes) return fail(SWB_ERR_STATE, "swb_upload_shapes has not been called");
    if (!h->have_pool) return fail(SWB_ERR_STATE, "swb_set_pool has not been called");
  }
  HIP_TRY(hipSetDevice(h->device));
  swb_sample_actions_args a;
  memset(&a, 0, sizeof(a));
  a.mode = mode; a.seed = seed; a.first_env = first_env;
  a.actions = out->actions; a.position = out->position; a.sprite = out->sprite; a.tries = out->tries;
  hipLaunchKernelGGL(swb_sample_actions_kernel, dim3((unsigned)h->p.N), dim3(SWB_WAVE), SWB_MAX_SHAPE_VERTS * sizeof(double2),
                     (hipStream_t)stream, h->p, a);
  HIP_TRY(hipGetLastError());
  return SWB_OK;
}

int swb_trim_run_lists(swb_handle h, int32_t* run_cap_out, void* stream) {
  if (!h) return fail(SWB_ERR_INVALID, "null handle");
  HIP_TRY(hipSetDevice(h->device));
  if (h->large_frames) {                 // (no run lists on the large-frame path: nothing to trim)
    if (run_cap_out) *run_cap_out = 0;
    return SWB_OK;
  }
  if (run_cap_out) *run_cap_out = h->p.run_cap;
  if (h->lists_trimmed || getenv("SWB_RUN_CAP") || getenv("SWB_NO_TRIM")) return SWB_OK;   // (done already / a test pinned the capacity)
  // (the cover kernel paints the frame: no lists at all -- nor, before its first launch, on a handle SWB_NO_PAINT_IN_COVER keeps from it)
  if (!h->d_runs && paints_in_cover(h, pick_variant(h->p.Wc), false)) return SWB_OK;
  if (!h->d_runs || !h->lists_valid) return fail(SWB_ERR_STATE, "swb_trim_run_lists: the last launch listed no runs (step or render first)");
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  // the longest list of the last launch: its end is in the header (no list has left its fixed part: it holds any scene)
  const swb_params& p = h->p;
  std::vector<uint32_t> hdr((size_t)p.N * SWB_RHDR_DWORDS);
  HIP_TRY(hipMemcpy(hdr.data(), h->d_rhdr, hdr.size() * 4, hipMemcpyDeviceToHost));
  uint32_t longest = 0;
  for (int n = 0; n < p.N; ++n)
    for (int g = 0; g < p.ncg; ++g) longest = std::max(longest, hdr[(size_t)n * SWB_RHDR_DWORDS + SWB_RHDR_GROUPS + g * SWB_RHDR_GSTRIDE]);
  if (longest >= (uint32_t)p.run_cap) return SWB_OK;                 // (cannot be: keep what there is)
  const int want = std::max(p.Hc / 2, (int)(longest + longest / 4 + 16)) + 1;
  if (want >= p.run_cap) return SWB_OK;                              // nothing to gain
  if (int rc = drop_run_lists(h)) return rc;          // (the lists move: no list stamped before this is kept, bump_list_epoch there)
  h->p.run_cap = want;
  h->lists_trimmed = true;
  if (int rc = ensure_handoff_tables(h)) return rc;
  if (run_cap_out) *run_cap_out = h->p.run_cap;
  return SWB_OK;
}

int swb_list_stats(swb_handle h, int64_t* kept, int64_t* built, void* stream) {
  if (!h || !kept || !built) return fail(SWB_ERR_INVALID, "null argument");
  if (!h->d_list_stats) return fail(SWB_ERR_STATE, "swb_list_stats: SWB_LIST_STATS was not set when the handle was created");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  unsigned long long w[2] = {0ull, 0ull};
  HIP_TRY(hipMemcpy(w, h->d_list_stats, sizeof(w), hipMemcpyDeviceToHost));
  *kept = (int64_t)w[0]; *built = (int64_t)w[1];
  return SWB_OK;
}

int swb_task_stats(swb_handle h, int64_t* reused, int64_t* evaluated, void* stream) {
  if (!h || !reused || !evaluated) return fail(SWB_ERR_INVALID, "null argument");
  if (!h->d_task_stats) return fail(SWB_ERR_STATE, "swb_task_stats: SWB_LIST_STATS was not set when the handle was created");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  unsigned long long w[2] = {0ull, 0ull};
  HIP_TRY(hipMemcpy(w, h->d_task_stats, sizeof(w), hipMemcpyDeviceToHost));
  *reused = (int64_t)w[0]; *evaluated = (int64_t)w[1];
  return SWB_OK;
}

int swb_frame_stats(swb_handle h, int64_t* copied, int64_t* filled, int64_t* resampled, void* stream) {
  if (!h || !copied || !filled || !resampled) return fail(SWB_ERR_INVALID, "null argument");
  if (!h->d_frame_stats) return fail(SWB_ERR_STATE, "swb_frame_stats: SWB_LIST_STATS was not set when the handle was created");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  unsigned long long w[3] = {0ull, 0ull, 0ull};
  HIP_TRY(hipMemcpy(w, h->d_frame_stats, sizeof(w), hipMemcpyDeviceToHost));
  *copied = (int64_t)w[0]; *filled = (int64_t)w[1]; *resampled = (int64_t)w[2];
  return SWB_OK;
}

int swb_split_stats(swb_handle h, int64_t* whole, int64_t* bands, int64_t* whole_copies, void* stream) {
  if (!h || !whole || !bands || !whole_copies) return fail(SWB_ERR_INVALID, "null argument");
  if (!h->d_split_stats)
    return fail(SWB_ERR_STATE, "swb_split_stats: the handle is not in split-bands mode, or SWB_LIST_STATS was not set when it was created");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  unsigned long long w[3] = {0ull, 0ull, 0ull};
  HIP_TRY(hipMemcpy(w, h->d_split_stats, sizeof(w), hipMemcpyDeviceToHost));
  *whole = (int64_t)w[0]; *bands = (int64_t)w[1]; *whole_copies = (int64_t)w[2];
  return SWB_OK;
}

int swb_frame_cycles(swb_handle h, int64_t* out3, void* stream) {
  if (!h || !out3) return fail(SWB_ERR_INVALID, "null argument");
  if (!h->d_frame_stats) return fail(SWB_ERR_STATE, "swb_frame_cycles: SWB_LIST_STATS was not set when the handle was created");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  unsigned long long w[3] = {0ull, 0ull, 0ull};
  HIP_TRY(hipMemcpy(w, h->d_frame_stats + 3, sizeof(w), hipMemcpyDeviceToHost));
  for (int i = 0; i < 3; ++i) out3[i] = (int64_t)w[i];
  return SWB_OK;
}

int swb_spec_copy_stats(swb_handle h, int64_t* copy_groups, void* stream) {
  if (!h || !copy_groups) return fail(SWB_ERR_INVALID, "null argument");
  if (!h->d_frame_stats) return fail(SWB_ERR_STATE, "swb_spec_copy_stats: SWB_LIST_STATS was not set when the handle was created");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  unsigned long long w = 0ull;
  HIP_TRY(hipMemcpy(&w, h->d_frame_stats + 6, sizeof(w), hipMemcpyDeviceToHost));
  *copy_groups = (int64_t)w;
  return SWB_OK;
}

int swb_factors(swb_handle h, double* factors_dev, void* stream) {
  if (!h || !factors_dev) return fail(SWB_ERR_INVALID, "null argument");
  if (!h->have_pool) return fail(SWB_ERR_STATE, "swb_set_pool has not been called");
  HIP_TRY(hipSetDevice(h->device));
  const int total = h->p.N * h->p.S;
  hipLaunchKernelGGL(swb_factors_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->p, factors_dev);
  HIP_TRY(hipGetLastError());
  return SWB_OK;
}

int swb_get_state(swb_handle h, const swb_state* st, void* stream) {
  if (!h || !st) return fail(SWB_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  const size_t N = h->p.N, NS = N * h->p.S;
  if (st->x) HIP_TRY(hipMemcpy(st->x, h->d_x, NS * 8, hipMemcpyDeviceToHost));
  if (st->y) HIP_TRY(hipMemcpy(st->y, h->d_y, NS * 8, hipMemcpyDeviceToHost));
  if (st->n_sprites) HIP_TRY(hipMemcpy(st->n_sprites, h->d_nspr, N * 4, hipMemcpyDeviceToHost));
  if (st->pool_entry) HIP_TRY(hipMemcpy(st->pool_entry, h->d_entry, N * 4, hipMemcpyDeviceToHost));
  if (st->step_count) HIP_TRY(hipMemcpy(st->step_count, h->d_step_count, N * 4, hipMemcpyDeviceToHost));
  if (st->reset_next) HIP_TRY(hipMemcpy(st->reset_next, h->d_reset_next, N, hipMemcpyDeviceToHost));
  if (st->episode) HIP_TRY(hipMemcpy(st->episode, h->d_episode, N * 4, hipMemcpyDeviceToHost));
  return SWB_OK;
}

int swb_get_env_state(swb_handle h, int32_t env, int32_t* out5, void* stream) {
  if (!h || !out5) return fail(SWB_ERR_INVALID, "null argument");
  if (env < 0 || env >= h->p.N) return fail(SWB_ERR_INVALID, "environment %d out of range", env);
  HIP_TRY(hipSetDevice(h->device));
  // (the N = 1 drop-in asks for this several times per step: one gather kernel and ONE 20-byte copy, stream-ordered behind
  // the steps, instead of a stream synchronisation and five 4-byte copies)
  if (!h->d_env_state && h->d_env_state.fill(nullptr, 8)) return SWB_ERR_HIP;
  hipLaunchKernelGGL(swb_env_state_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, h->p, env, h->d_env_state);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out5, h->d_env_state, 5 * sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return SWB_OK;
}

int swb_get_sprite_types(swb_handle h, int32_t env, int32_t sprite, int32_t* flags, void* stream) {
  if (!h || !flags) return fail(SWB_ERR_INVALID, "null argument");
  if (!h->have_pool) return fail(SWB_ERR_STATE, "no pool on the device");
  if (env < 0 || env >= h->p.N) return fail(SWB_ERR_INVALID, "environment %d out of range", env);
  if (sprite < 0 || sprite >= h->p.S) return fail(SWB_ERR_INVALID, "sprite %d out of range", sprite);
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  int32_t en = 0;
  uint8_t f = 0;
  HIP_TRY(hipMemcpy(&en, h->d_entry + env, 4, hipMemcpyDeviceToHost));
  if (en < 0 || en >= h->pool_entries) return fail(SWB_ERR_STATE, "environment %d has not been reset yet", env);
  HIP_TRY(hipMemcpy(&f, h->d_p_attr + (size_t)en * h->p.S + sprite, 1, hipMemcpyDeviceToHost));
  *flags = f;
  return SWB_OK;
}

int swb_set_positions(swb_handle h, const double* x_host, const double* y_host, void* stream) {
  if (!h || !x_host || !y_host) return fail(SWB_ERR_INVALID, "null argument");
  bump_state_epochs(h);              // BOTH (positions)
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  const size_t NS = (size_t)h->p.N * h->p.S;
  HIP_TRY(hipMemcpy(h->d_x, x_host, NS * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_y, y_host, NS * 8, hipMemcpyHostToDevice));
  return SWB_OK;
}

// ---------------------------------------------------------------------------------------------------
// Snapshots (include/swb.h): swb_state_save_kernel / swb_state_load_kernel between the handle's state arrays -- or the scratch of
// its last rollout -- and a caller's block of C slots.  Neither is a launch(): no parity, phase or cost list moves.
// ---------------------------------------------------------------------------------------------------
static swb_state_view live_state_view(swb_engine* h) {
  swb_state_view v;
  v.x = h->d_x; v.y = h->d_y; v.nspr = h->d_nspr; v.entry = h->d_entry; v.step_count = h->d_step_count; v.episode = h->d_episode;
  v.pool_base = h->d_pool_base; v.pool_len = h->d_pool_len; v.reset_next = h->d_reset_next;
  return v;
}

// What swb_save_state and swb_load_state refuse alike (`name`: the caller's, for the messages); the snapshot as a state view.
static int check_snapshot_call(swb_handle h, const char* name, const swb_snapshot* snap, int32_t C, swb_state_view* v) {
  if (!h) return fail(SWB_ERR_INVALID, "%s: null handle", name);
  if (!snap) return fail(SWB_ERR_INVALID, "%s: snapshot is NULL", name);
  if (!snap->x || !snap->y || !snap->n_sprites || !snap->pool_entry || !snap->step_count || !snap->episode || !snap->pool_base ||
      !snap->pool_len || !snap->reset_next)
    return fail(SWB_ERR_INVALID, "%s: a pointer of the snapshot is NULL (every array is required)", name);
  if (C < 1) return fail(SWB_ERR_INVALID, "%s: C must be positive (C = %d)", name, C);
  if ((long long)C * h->p.S > 0x7fffffffll)
    return fail(SWB_ERR_INVALID, "%s: C x max_sprites = %d x %d does not fit an int (the slots are indexed with one)", name, C, h->p.S);
  v->x = snap->x; v->y = snap->y; v->nspr = snap->n_sprites; v->entry = snap->pool_entry; v->step_count = snap->step_count;
  v->episode = snap->episode; v->pool_base = snap->pool_base; v->pool_len = snap->pool_len; v->reset_next = snap->reset_next;
  return 0;
}

int swb_pool_id(swb_handle h, uint64_t* id) {
  if (!h || !id) return fail(SWB_ERR_INVALID, "swb_pool_id: null argument");
  *id = h->have_pool ? h->pool_id : 0;
  return SWB_OK;
}

int swb_save_state(swb_handle h, int32_t source, const int32_t* index_dev, int32_t C, const swb_snapshot* snap, void* stream) {
  swb_state_view dst;
  if (int rc = check_snapshot_call(h, "swb_save_state", snap, C, &dst)) return rc;
  if (source != SWB_STATE_LIVE && source != SWB_STATE_ROLLOUT_END) return fail(SWB_ERR_INVALID, "swb_save_state: unknown source %d", source);
  if (!h->have_pool) return fail(SWB_ERR_STATE, "swb_save_state: swb_set_pool has not been called");
  if (h->setters)
    return fail(SWB_ERR_STATE, "swb_save_state: sprite setters have been called on this handle; snapshots under live overrides are not supported");
  long long n_src = h->p.N;
  swb_state_view src = live_state_view(h);
  if (source == SWB_STATE_ROLLOUT_END) {
    if (!h->rollout_M) return fail(SWB_ERR_STATE, "swb_save_state: no rollout has run on this handle (swb_rollout first)");
    if (h->rollout_stale)
      return fail(SWB_ERR_STATE, "swb_save_state: the pool has changed since the last rollout (swb_set_pool, swb_sample_pool or "
                  "swb_resample_pool): its candidates may sit in entries that have been redrawn; roll out again");
    n_src = (long long)h->p.N * h->rollout_M;          // (the scratch is in candidate order already: v = n * M + m)
    src = rollout_state_view(h->d_rollout.ptr, (size_t)n_src, (size_t)h->p.S);
  }
  if (!index_dev && C != n_src)
    return fail(SWB_ERR_INVALID, "swb_save_state: index is NULL (slot c takes element c) but C = %d and the source has %lld", C, n_src);
  HIP_TRY(hipSetDevice(h->device));
  const size_t threads = (size_t)C * h->p.S;
  hipLaunchKernelGGL(swb_state_save_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, dst,
                     index_dev, (int)C, (int)h->p.S, (int)n_src);
  HIP_TRY(hipGetLastError());
  return SWB_OK;
}

int swb_load_state(swb_handle h, const swb_snapshot* snap, int32_t C, const int32_t* slot_dev, uint64_t pool_id,
                   int32_t* rejected_dev, void* stream) {
  swb_state_view src;
  if (int rc = check_snapshot_call(h, "swb_load_state", snap, C, &src)) return rc;
  if (!slot_dev && C != h->p.N)
    return fail(SWB_ERR_INVALID, "swb_load_state: slot is NULL (environment n takes slot n) but C = %d and the handle has %d environments",
                C, h->p.N);
  if (!h->have_pool) return fail(SWB_ERR_STATE, "swb_load_state: swb_set_pool has not been called");
  if (h->setters)
    return fail(SWB_ERR_STATE, "swb_load_state: sprite setters have been called on this handle; snapshots under live overrides are not supported");
  if (pool_id != 0 && pool_id != h->pool_id)
    return fail(SWB_ERR_STATE, "swb_load_state: the snapshot was saved under pool %llu, the handle holds pool %llu (a pool call since "
                "may have redrawn the entries it plays; pool_id = 0 skips the check)", (unsigned long long)pool_id,
                (unsigned long long)h->pool_id);
  HIP_TRY(hipSetDevice(h->device));
  // Invalidation, per environment: the kernel clears SWB_RHDR_STAMP of the environments it loads, so their next cover wave
  // builds (and resets SWB_RHDR_FRAME); the epoch stays, the others keep lists and cached frames.  A handle without headers
  // has nothing to clear: painting builds, large frames and many sprites have no lists and pass epoch 0 at every launch, and
  // headers that are not allocated yet (no launch so far, or dropped by a trim or a pool call) come back zeroed -- no stamp.
  // The task records have no per-environment invalidation: positions, labels and counts of the loaded environments change, so
  // the task epoch moves for all (one evaluation each at the next step) -- the list epoch still stays.
  if (++h->task_epoch == 0u) h->task_epoch = 1u;
  uint32_t* const rhdr = h->d_rhdr ? h->d_rhdr.ptr : nullptr;
  // (the ranges may have moved between environments: swb_resample_pool's skip of live entries needs the env-major layout)
  h->pool_uniform = false;
  const size_t threads = (size_t)h->p.N * h->p.S;
  hipLaunchKernelGGL(swb_state_load_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src,
                     live_state_view(h), slot_dev, (int)C, (int)h->p.N, (int)h->p.S, rhdr, rejected_dev);
  HIP_TRY(hipGetLastError());
  return SWB_OK;
}

int swb_copy_pool(swb_handle dst, swb_handle src, const int32_t* pool_base_host, const int32_t* pool_len_host, void* stream) {
  if (!dst || !src || !pool_base_host || !pool_len_host) return fail(SWB_ERR_INVALID, "swb_copy_pool: null argument");
  if (dst == src) return fail(SWB_ERR_INVALID, "swb_copy_pool: dst and src are the same handle");
  if (dst->device != src->device || dst->p.S != src->p.S || dst->p.n_tasks != src->p.n_tasks || dst->p.pos_is_f32 != src->p.pos_is_f32 ||
      dst->keyed != src->keyed)
    return fail(SWB_ERR_INVALID, "swb_copy_pool: the handles differ (device %d / %d, max_sprites %d / %d, n_tasks %d / %d, pos_is_f32 %d / %d, "
                "a task keys on position %d / %d)", dst->device, src->device, dst->p.S, src->p.S, dst->p.n_tasks, src->p.n_tasks,
                dst->p.pos_is_f32, src->p.pos_is_f32, (int)dst->keyed, (int)src->keyed);
  if (dst->n_sets != src->n_sets || memcmp(dst->sets, src->sets, sizeof(swb_task_set) * (size_t)src->n_sets) != 0)
    return fail(SWB_ERR_INVALID, "swb_copy_pool: the handles' task sets differ (%d / %d sets, or their fields): the entries' sets would "
                "mean another task in dst", dst->n_sets, src->n_sets);
  if (!src->have_pool) return fail(SWB_ERR_STATE, "swb_copy_pool: src has no pool (swb_set_pool has not been called on it)");
  if (dst->setters || src->setters)
    return fail(SWB_ERR_STATE, "swb_copy_pool: sprite setters have been called on one of the handles; snapshots under live overrides are not supported");
  const int P = src->pool_entries, N = dst->p.N;
  for (int i = 0; i < N; ++i)
    if (pool_len_host[i] < 1 || pool_base_host[i] < 0 || pool_base_host[i] + pool_len_host[i] > P)
      return fail(SWB_ERR_INVALID, "swb_copy_pool: env %d: pool range [%d, +%d) outside the pool of %d", i, pool_base_host[i], pool_len_host[i], P);
  const int verts = src->have_shapes ? src->p.max_edges : 0;       // (the pool's largest scene: sizes dst's LDS as it does src's)
  if (verts > 0)
    if (int rc = lf_check_vertices(dst, verts, "swb_copy_pool")) return rc;
  HIP_TRY(hipSetDevice(dst->device));
  const hipStream_t st = (hipStream_t)stream;
  // Into temporaries, swapped in once every copy is made (the advice on swb_set_pool): a failure half-way leaves dst's pool whole.
  // SWB_COPY_POOL_FAIL_AT (tests): the allocation that fails.
  dev_buf<int32_t> t_n, t_shape, t_base, t_len;
  dev_buf<double> t_x, t_y, t_xv, t_yv, t_scale, t_ca, t_sa, t_angle, t_color;
  dev_buf<uint32_t> t_rgb;
  dev_buf<int8_t> t_label, t_cell_label;
  dev_buf<uint8_t> t_attr, t_set;
  const bool have_angle = src->p.p_angle != nullptr, have_color = src->p.p_color != nullptr;
  int made = 0, fail_at = -1;
  if (const char* x = getenv("SWB_COPY_POOL_FAIL_AT")) fail_at = atoi(x);
#define SWB_CLONE(tmp, from)                                                                                               \
  do {                                                                                                                     \
    if (made++ == fail_at) return fail(SWB_ERR_HIP, "swb_copy_pool: allocation %d refused (SWB_COPY_POOL_FAIL_AT)", made - 1); \
    if (tmp.clone(src->from.ptr, src->from.count, st)) return SWB_ERR_HIP;                                                 \
  } while (0)
  SWB_CLONE(t_n, d_p_n);
  SWB_CLONE(t_x, d_p_x); SWB_CLONE(t_y, d_p_y); SWB_CLONE(t_xv, d_p_xv); SWB_CLONE(t_yv, d_p_yv);
  SWB_CLONE(t_scale, d_p_scale); SWB_CLONE(t_ca, d_p_ca); SWB_CLONE(t_sa, d_p_sa);
  SWB_CLONE(t_shape, d_p_shape); SWB_CLONE(t_rgb, d_p_rgb); SWB_CLONE(t_label, d_p_label); SWB_CLONE(t_attr, d_p_attr);
  if (src->keyed) SWB_CLONE(t_cell_label, d_p_cell_label);
  if (have_angle) SWB_CLONE(t_angle, d_p_angle);
  if (have_color) SWB_CLONE(t_color, d_p_color);
  if (src->n_sets) SWB_CLONE(t_set, d_p_set);
#undef SWB_CLONE
  if (t_base.fill(pool_base_host, N) || t_len.fill(pool_len_host, N)) return SWB_ERR_HIP;
  HIP_TRY(hipDeviceSynchronize());                 // (the copies are made; work in flight may still read dst's old arrays)
  dst->d_p_n.swap(t_n); dst->d_p_x.swap(t_x); dst->d_p_y.swap(t_y); dst->d_p_xv.swap(t_xv); dst->d_p_yv.swap(t_yv);
  dst->d_p_scale.swap(t_scale); dst->d_p_ca.swap(t_ca); dst->d_p_sa.swap(t_sa); dst->d_p_shape.swap(t_shape); dst->d_p_rgb.swap(t_rgb);
  dst->d_p_label.swap(t_label); dst->d_p_attr.swap(t_attr);
  if (src->keyed) dst->d_p_cell_label.swap(t_cell_label);
  if (have_angle) dst->d_p_angle.swap(t_angle);
  if (have_color) dst->d_p_color.swap(t_color);
  if (src->n_sets) { dst->d_p_set.swap(t_set); if (int rc = publish_entry_sets(dst)) return rc; }
  dst->d_pool_base.swap(t_base); dst->d_pool_len.swap(t_len);
  bump_state_epochs(dst);            // BOTH (dst plays another pool)
  dst->rollout_stale = true;
  bind_pool(dst, have_angle, have_color);
  dst->pool_entries = P;
  dst->pool_id = src->pool_id;
  dst->pool_sampled = false;                       // (the sampler's specification is not copied: dst cannot redraw)
  dst->pool_tree = false;
  dst->pool_uniform = false;
  if (verts > 0) dst->p.max_edges = verts;
  HIP_TRY(hipMemsetAsync(dst->d_reset_next, 1, N, st));
  HIP_TRY(hipMemsetAsync(dst->d_episode, 0, sizeof(int32_t) * N, st));
  HIP_TRY(hipMemsetAsync(dst->d_step_count, 0, sizeof(int32_t) * N, st));
  dst->have_pool = true;
  return restore_run_list_reservation(dst);
}

// ---------------------------------------------------------------------------------------------------
// Task sets: the table lives in device memory in front of the set of every pool entry (d_p_set,
// the block), not in the kernel arguments, and the block's pointer behind the override flags: swb_params does not grow.  A handle with a table runs the OV builds of the step kernels -- the ones that carry the lookup --: it owns the
// override FLAGS (all zero) from here on, the override arrays only once a setter is called (swb_engine::setters).
// ---------------------------------------------------------------------------------------------------
int swb_set_task_sets(swb_handle h, int32_t n_sets, const swb_task_set* sets) {
  if (!h || !sets) return fail(SWB_ERR_INVALID, "swb_set_task_sets: null argument");
  if (h->n_sets) return fail(SWB_ERR_STATE, "swb_set_task_sets: the handle has its task sets already (set once, after swb_create)");
  if (h->have_pool) return fail(SWB_ERR_STATE, "swb_set_task_sets: a pool has been installed (call it after swb_create, before any pool)");
  if (n_sets < 1 || n_sets > SWB_MAX_TASK_SETS)
    return fail(SWB_ERR_INVALID, "swb_set_task_sets: n_sets = %d is outside [1, %d]", n_sets, SWB_MAX_TASK_SETS);
  for (int g = 0; g < n_sets; ++g) {
    const swb_task_set& s = sets[g];
    if (s.n_tasks < 1 || s.first_task < 0 || (long long)s.first_task + s.n_tasks > h->p.n_tasks)
      return fail(SWB_ERR_INVALID, "swb_set_task_sets: set %d: sub-tasks [%d, +%d) outside the %d of the handle", g, s.first_task, s.n_tasks,
                  h->p.n_tasks);
    if (!s.is_meta && s.n_tasks != 1)
      return fail(SWB_ERR_INVALID, "swb_set_task_sets: set %d: %d sub-tasks without is_meta (a plain task is one sub-task)", g, s.n_tasks);
    if (s.is_meta && (s.meta_aggregator < SWB_AGG_SUM || s.meta_aggregator > SWB_AGG_MEAN || s.meta_termination < SWB_TERM_ALL ||
                      s.meta_termination > SWB_TERM_ANY))
      return fail(SWB_ERR_INVALID, "swb_set_task_sets: set %d: unknown aggregator %d or termination rule %d", g, s.meta_aggregator,
                  s.meta_termination);
    if (s.max_episode_length < 0) return fail(SWB_ERR_INVALID, "swb_set_task_sets: set %d: max_episode_length = %d", g, s.max_episode_length);
  }
  HIP_TRY(hipSetDevice(h->device));
  if (alloc_ov_flags(h)) return SWB_ERR_HIP;
  h->p.ov_flag = h->d_ov_flag;
  memset(h->sets, 0, sizeof(h->sets));
  for (int g = 0; g < n_sets; ++g) {
    h->sets[g] = sets[g];
    h->sets[g].is_meta = sets[g].is_meta ? 1 : 0;
    if (!sets[g].is_meta) { h->sets[g].meta_aggregator = 0; h->sets[g].meta_termination = 0; h->sets[g].meta_terminate_bonus = 0.0; }
  }
  h->n_sets = n_sets;
  bump_state_epochs(h);              // BOTH (nothing is kept across the switch of kernels)
  return SWB_OK;
}

static int check_entry_sets_call(swb_handle h, const char* name, const void* arg) {
  if (!h || !arg) return fail(SWB_ERR_INVALID, "%s: null argument", name);
  if (!h->n_sets) return fail(SWB_ERR_STATE, "%s: the handle has no task sets (swb_set_task_sets)", name);
  if (!h->have_pool) return fail(SWB_ERR_STATE, "%s: swb_set_pool has not been called", name);
  return 0;
}

int swb_set_entry_task_sets(swb_handle h, const uint8_t* set_of_entry_host, void* stream) {
  if (int rc = check_entry_sets_call(h, "swb_set_entry_task_sets", set_of_entry_host)) return rc;
  for (int e = 0; e < h->pool_entries; ++e)
    if (set_of_entry_host[e] >= h->n_sets)
      return fail(SWB_ERR_INVALID, "swb_set_entry_task_sets: entry %d names set %d, the handle has %d", e, (int)set_of_entry_host[e], h->n_sets);
  HIP_TRY(hipSetDevice(h->device));
  const hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemcpyAsync(h->d_p_set.ptr + SWB_SET_TABLE_BYTES, set_of_entry_host, (size_t)h->pool_entries, hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st)); // (the host array is the caller's, and pageable: it may be gone on return)
  // the task of running episodes changes: no record stamped before this is reused.  Lists and cached frames do not depend on it.
  if (++h->task_epoch == 0u) h->task_epoch = 1u;
  return SWB_OK;
}

int swb_get_entry_task_sets(swb_handle h, uint8_t* set_of_entry_host) {
  if (int rc = check_entry_sets_call(h, "swb_get_entry_task_sets", set_of_entry_host)) return rc;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(set_of_entry_host, h->d_p_set.ptr + SWB_SET_TABLE_BYTES, (size_t)h->pool_entries, hipMemcpyDeviceToHost));
  return SWB_OK;
}

int swb_env_task_sets(swb_handle h, int32_t* set_dev, void* stream) {
  if (int rc = check_entry_sets_call(h, "swb_env_task_sets", set_dev)) return rc;
  HIP_TRY(hipSetDevice(h->device));
  hipLaunchKernelGGL(swb_env_task_sets_kernel, dim3((unsigned)((h->p.N + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const int32_t*)h->d_entry.ptr, (const uint8_t*)h->d_p_set.ptr + SWB_SET_TABLE_BYTES, set_dev, (int)h->p.N, (int)h->pool_entries);
  HIP_TRY(hipGetLastError());
  return SWB_OK;
}

// ---------------------------------------------------------------------------------------------------
// Sprite attribute setters (sprite.py:152-175).  The arithmetic is matplotlib's, restated on the host:
//   Affine2D.rotate(theta)   -> [[a, -b, 0], [b, a, 0]] with a = cos(theta), b = sin(theta)   (transforms.py)
//   Affine2D.scale(s)        -> [[s, 0, 0], [0, s, 0]]
//   transform_path           -> _path.h affine_transform_2d: t0 = sx*x; t1 = shx*y; x' = t0 + t1 + tx  (no FMA;
//                               this file is compiled with -ffp-contract=off)
// ---------------------------------------------------------------------------------------------------
static void affine2(double sx, double shx, double shy, double sy, int n, const double* in, double* out) {
  for (int i = 0; i < n; ++i) {
    const double x = in[2 * i], y = in[2 * i + 1];
    double t0 = sx * x, t1 = shx * y;
    const double ox = t0 + t1 + 0.0;
    t0 = shy * x; t1 = sy * y;
    out[2 * i] = ox;
    out[2 * i + 1] = t0 + t1 + 0.0;
  }
}
static double deg2rad(double d) { return d * (3.14159265358979323846 / 180.0); }   // math.radians

int swb_sprite_path_op(int32_t attr, double a, double b, int32_t n, const double* in_xy, double* out_xy) {
  if (!in_xy || !out_xy || n < 0) return fail(SWB_ERR_INVALID, "bad argument");
  if (attr == SWB_ATTR_SHAPE) {          // _reset_centered_path: scale(a) then rotate_deg(b): M = R * S
    const double th = deg2rad(b), ca = std::cos(th), sa = std::sin(th);
    affine2(ca * a, -sa * a, sa * a, ca * a, n, in_xy, out_xy);
  } else if (attr == SWB_ATTR_ANGLE) {   // rotate_deg(a - b)
    const double th = deg2rad(a - b), ca = std::cos(th), sa = std::sin(th);
    affine2(ca, -sa, sa, ca, n, in_xy, out_xy);
  } else if (attr == SWB_ATTR_SCALE) {   // scale(a - b): the reference's setter scales by the DIFFERENCE (sprite.py:173)
    const double f = a - b;
    affine2(f, 0.0, 0.0, f, n, in_xy, out_xy);
  } else {
    return fail(SWB_ERR_INVALID, "unknown sprite attribute %d", attr);
  }
  return SWB_OK;
}

namespace {

// Host copy of one environment's override record.
struct env_override {
  std::vector<int32_t> shape;
  std::vector<double> scale, angle, cpath;   // cpath: [S][SWB_MAX_SHAPE_VERTS][2]
  std::vector<int8_t> label;                 // [T][S]
};

int ov_allocate(swb_engine* h) {
  if (h->setters) return 0;
  const size_t N = h->p.N, NS = N * h->p.S, T = h->p.n_tasks;
  int rc = 0;
  rc |= h->d_ov_shape.fill(nullptr, NS);
  rc |= h->d_ov_scale.fill(nullptr, NS);
  rc |= h->d_ov_angle.fill(nullptr, NS);
  rc |= h->d_ov_label.fill(nullptr, NS * T);
  rc |= h->d_ov_cpath.fill(nullptr, NS * SWB_MAX_SHAPE_VERTS * 2);
  if (h->keyed) rc |= h->d_ov_cell_label.fill(nullptr, NS * T * SWB_MAX_CELLS);
  rc |= alloc_ov_flags(h);                   // last: its presence switches the engine to the OV kernels
  if (rc) return SWB_ERR_HIP;
  h->setters = true;
  swb_params& p = h->p;
  p.ov_flag = h->d_ov_flag; p.ov_shape = h->d_ov_shape; p.ov_scale = h->d_ov_scale; p.ov_angle = h->d_ov_angle;
  p.ov_label = h->d_ov_label; p.ov_cpath = h->d_ov_cpath;
  p.ov_cell_label = h->d_ov_cell_label;
  return 0;
}

// The record of environment `env`: its override arrays when the flag is set, else built from its pool entry
// (fresh centred paths, sprite.py:96-101).  `n` receives the episode's sprite count.
// `for_write`: a setter needs a running episode; reading the sprites of an episode that has just ended (the
// reference's sprites stay readable until the next reset) is fine.
int ov_fetch(swb_engine* h, int env, env_override* r, int* n, bool* was_set, bool for_write = true) {
  const int S = h->p.S, T = h->p.n_tasks;
  r->shape.assign(S, 0); r->scale.assign(S, 1.0); r->angle.assign(S, 0.0);
  r->cpath.assign((size_t)S * SWB_MAX_SHAPE_VERTS * 2, 0.0); r->label.assign((size_t)T * S, 0);
  uint8_t flag = 0, rn = 0;
  int32_t en = 0, ns = 0;
  if (h->d_ov_flag) HIP_TRY(hipMemcpy(&flag, h->d_ov_flag + env, 1, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(&rn, h->d_reset_next + env, 1, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(&en, h->d_entry + env, 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(&ns, h->d_nspr + env, 4, hipMemcpyDeviceToHost));
  int32_t ep = 0;
  HIP_TRY(hipMemcpy(&ep, h->d_episode + env, 4, hipMemcpyDeviceToHost));
  if (ep == 0) return fail(SWB_ERR_STATE, "environment %d has not been reset yet: it has no sprites", env);
  if (rn && for_write)
    return fail(SWB_ERR_STATE, "environment %d is about to reset (its episode ended): its sprites are gone at the next step", env);
  *n = ns;
  *was_set = flag != 0;
  const size_t o = (size_t)env * S, pe = (size_t)en * S;
  if (flag) {
    HIP_TRY(hipMemcpy(r->shape.data(), h->d_ov_shape + o, S * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(r->scale.data(), h->d_ov_scale + o, S * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(r->angle.data(), h->d_ov_angle + o, S * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(r->label.data(), h->d_ov_label + o * T, (size_t)T * S, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(r->cpath.data(), h->d_ov_cpath + o * SWB_MAX_SHAPE_VERTS * 2, (size_t)S * SWB_MAX_SHAPE_VERTS * 16,
                      hipMemcpyDeviceToHost));
    return 0;
  }
  if (!h->p.p_angle) return fail(SWB_ERR_STATE, "the pool carries no angle column (swb_pool.angle)");
  std::vector<double> ca(S), sa(S);
  HIP_TRY(hipMemcpy(r->shape.data(), h->d_p_shape + pe, S * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(r->scale.data(), h->d_p_scale + pe, S * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(r->angle.data(), h->d_p_angle + pe, S * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(ca.data(), h->d_p_ca + pe, S * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(sa.data(), h->d_p_sa + pe, S * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(r->label.data(), h->d_p_label + pe * T, (size_t)T * S, hipMemcpyDeviceToHost));
  std::vector<double> sv((size_t)h->p.max_verts * 2 + 2);
  std::vector<int32_t> off(h->shape_nverts.size() + 1);
  HIP_TRY(hipMemcpy(off.data(), h->d_shape_off, off.size() * 4, hipMemcpyDeviceToHost));
  for (int s2 = 0; s2 < ns; ++s2) {
    const int sh = r->shape[s2];
    if (sh < 0 || sh >= (int)h->shape_nverts.size()) return fail(SWB_ERR_STATE, "pool entry %d uses shape %d", en, sh);
    const int nv = h->shape_nverts[sh];
    HIP_TRY(hipMemcpy(sv.data(), h->d_shape_verts + 2 * (size_t)off[sh], (size_t)nv * 16, hipMemcpyDeviceToHost));
    // the kernel's centered_vertex with the pool's cos / sin (math.cos(math.radians(angle)), computed by the caller)
    affine2(ca[s2] * r->scale[s2], -sa[s2] * r->scale[s2], sa[s2] * r->scale[s2], ca[s2] * r->scale[s2], nv, sv.data(),
            r->cpath.data() + (size_t)s2 * SWB_MAX_SHAPE_VERTS * 2);
  }
  return 0;
}

int ov_store(swb_engine* h, int env, const env_override& r) {
  const int S = h->p.S, T = h->p.n_tasks;
  const size_t o = (size_t)env * S;
  HIP_TRY(hipMemcpy(h->d_ov_shape + o, r.shape.data(), S * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_ov_scale + o, r.scale.data(), S * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_ov_angle + o, r.angle.data(), S * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_ov_label + o * T, r.label.data(), (size_t)T * S, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_ov_cpath + o * SWB_MAX_SHAPE_VERTS * 2, r.cpath.data(), (size_t)S * SWB_MAX_SHAPE_VERTS * 16,
                    hipMemcpyHostToDevice));
  const uint8_t one = 1;
  HIP_TRY(hipMemcpy(h->d_ov_flag + env, &one, 1, hipMemcpyHostToDevice));
  return 0;
}

}  // namespace

int swb_set_sprite_attr(swb_handle h, int32_t env, int32_t sprite, int32_t attr, double value, const double* delta,
                        const int8_t* label, void* stream) {
  if (!h) return fail(SWB_ERR_INVALID, "null handle");
  bump_state_epochs(h);              // BOTH (a position, a label, or what a filter reads)
  if (!h->have_pool || !h->have_shapes) return fail(SWB_ERR_STATE, "no pool / shape table installed");
  if (env < 0 || env >= h->p.N) return fail(SWB_ERR_INVALID, "environment %d out of range", env);
  if (attr < SWB_ATTR_SHAPE || attr > SWB_ATTR_SCALE) return fail(SWB_ERR_INVALID, "unknown sprite attribute %d", attr);
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  env_override r;
  int n = 0;
  bool was_set = false;
  if (int rc = ov_fetch(h, env, &r, &n, &was_set)) return rc;
  if (sprite < 0 || sprite >= n) return fail(SWB_ERR_INVALID, "environment %d has %d sprites: sprite %d out of range", env, n, sprite);
  const int S = h->p.S, T = h->p.n_tasks;
  double* path = r.cpath.data() + (size_t)sprite * SWB_MAX_SHAPE_VERTS * 2;
  const int nv_old = h->shape_nverts[r.shape[sprite]];
  std::vector<double> out((size_t)SWB_MAX_SHAPE_VERTS * 2, 0.0);
  if (attr == SWB_ATTR_SHAPE) {                        // sprite.py:152-155: _shape = s; _reset_centered_path()
    const int sh = (int)value;
    if ((double)sh != value || sh < 0 || sh >= (int)h->shape_nverts.size()) return fail(SWB_ERR_INVALID, "bad shape index %g", value);
    const int nv = h->shape_nverts[sh];
    std::vector<int32_t> off(h->shape_nverts.size() + 1);
    HIP_TRY(hipMemcpy(off.data(), h->d_shape_off, off.size() * 4, hipMemcpyDeviceToHost));
    std::vector<double> sv((size_t)nv * 2);
    HIP_TRY(hipMemcpy(sv.data(), h->d_shape_verts + 2 * (size_t)off[sh], (size_t)nv * 16, hipMemcpyDeviceToHost));
    if (int rc = swb_sprite_path_op(SWB_ATTR_SHAPE, r.scale[sprite], r.angle[sprite], nv, sv.data(), out.data())) return rc;
    r.shape[sprite] = sh;
  } else if (attr == SWB_ATTR_ANGLE) {                 // :161-165: rotate_deg(a - _angle) applied to the current path
    const double a = delta ? *delta : value, b = delta ? 0.0 : r.angle[sprite];
    if (int rc = swb_sprite_path_op(SWB_ATTR_ANGLE, a, b, nv_old, path, out.data())) return rc;
    r.angle[sprite] = value;
  } else {                                             // :171-175: scale(s - _scale) applied to the current path
    const double a = delta ? *delta : value, b = delta ? 0.0 : r.scale[sprite];
    if (int rc = swb_sprite_path_op(SWB_ATTR_SCALE, a, b, nv_old, path, out.data())) return rc;
    r.scale[sprite] = value;
  }
  memcpy(path, out.data(), out.size() * sizeof(double));
  if (label) for (int t = 0; t < T; ++t) r.label[(size_t)t * S + sprite] = label[t];
  // LDS of a wave is sized by the most polygon vertices an episode can have: a new shape may raise it
  int tot = 0;
  for (int s2 = 0; s2 < n; ++s2) tot += h->shape_nverts[r.shape[s2]];
  if (int rc = lf_check_vertices(h, std::max(h->p.max_edges, (tot + 3) & ~3), "swb_set_sprite_attr")) return rc;
  h->p.max_edges = std::max(h->p.max_edges, (tot + 3) & ~3);
  if (int rc = ov_allocate(h)) return rc;
  if (!was_set && h->keyed) {                          // the episode's per-cell labels: from its pool entry, until
    int32_t en = 0;                                    // swb_set_sprite_cell_labels replaces the sprite's
    HIP_TRY(hipMemcpy(&en, h->d_entry + env, 4, hipMemcpyDeviceToHost));
    const size_t blk = (size_t)T * S * SWB_MAX_CELLS;
    HIP_TRY(hipMemcpy(h->d_ov_cell_label + (size_t)env * blk, h->d_p_cell_label + (size_t)en * blk, blk, hipMemcpyDeviceToDevice));
  }
  return ov_store(h, env, r);
}

int swb_set_sprite_cell_labels(swb_handle h, int32_t env, int32_t sprite, const int8_t* cells, void* stream) {
  if (!h || !cells) return fail(SWB_ERR_INVALID, "null argument");
  bump_state_epochs(h);              // BOTH (labels per cell)
  if (!h->keyed) return fail(SWB_ERR_INVALID, "no task of this handle keys on position");
  if (env < 0 || env >= h->p.N || sprite < 0 || sprite >= h->p.S) return fail(SWB_ERR_INVALID, "environment %d / sprite %d out of range", env, sprite);
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  uint8_t flag = 0;
  if (h->d_ov_flag) HIP_TRY(hipMemcpy(&flag, h->d_ov_flag + env, 1, hipMemcpyDeviceToHost));
  if (!flag) return fail(SWB_ERR_STATE, "swb_set_sprite_cell_labels follows swb_set_sprite_attr on the same environment");
  const int S = h->p.S, T = h->p.n_tasks;
  for (int t = 0; t < T; ++t)
    HIP_TRY(hipMemcpy(h->d_ov_cell_label + (((size_t)env * T + t) * S + sprite) * SWB_MAX_CELLS, cells + (size_t)t * SWB_MAX_CELLS,
                      SWB_MAX_CELLS, hipMemcpyHostToDevice));
  return SWB_OK;
}

int swb_get_sprite(swb_handle h, int32_t env, int32_t sprite, int32_t* shape, double* angle, double* scale, int32_t* n_verts,
                   double* path_xy, void* stream) {
  if (!h) return fail(SWB_ERR_INVALID, "null handle");
  if (!h->have_pool || !h->have_shapes) return fail(SWB_ERR_STATE, "no pool / shape table installed");
  if (env < 0 || env >= h->p.N) return fail(SWB_ERR_INVALID, "environment %d out of range", env);
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  env_override r;
  int n = 0;
  bool was_set = false;
  if (int rc = ov_fetch(h, env, &r, &n, &was_set, false)) return rc;
  if (sprite < 0 || sprite >= n) return fail(SWB_ERR_INVALID, "environment %d has %d sprites: sprite %d out of range", env, n, sprite);
  const int nv = h->shape_nverts[r.shape[sprite]];
  if (shape) *shape = r.shape[sprite];
  if (angle) *angle = r.angle[sprite];
  if (scale) *scale = r.scale[sprite];
  if (n_verts) *n_verts = nv;
  if (path_xy) memcpy(path_xy, r.cpath.data() + (size_t)sprite * SWB_MAX_SHAPE_VERTS * 2, (size_t)nv * 16);
  return SWB_OK;
}

int swb_variant(swb_handle h, swb_variant_info* out) {
  if (!h || !out) return fail(SWB_ERR_INVALID, "null argument");
  out->task_cache_bytes = (int64_t)(h->d_task_cache.count * sizeof(swb_task_record));
  if (h->large_frames) {                 // the narrowest cover build (state phase only), then the large-frame render kernels
    const variant* v0 = &kVariants[0];
    out->nw = v0->nw; out->ncol = 1; out->vs = 0;
    out->lds_bytes_per_wave = (int32_t)lds_per_wave(h, v0, nullptr);
    out->waves_per_simd = SWB_COVER_WAVES(v0->nw);
    out->resample_waves_per_simd = 0;
    out->n_bands = 0;
    out->n_column_groups = 0;
    out->run_cap = 0;
    out->paint_in_cover = 0;
    out->arena_units = 0;
    out->large_frames = 1;
    out->many_sprites = h->many_sprites ? 1 : 0;
    out->reserved_ = 0;
    if (h->many_sprites) {            // (no cover kernel: swb_ms_state_kernel, one wave per environment)
      out->nw = 0;
      out->lds_bytes_per_wave = (int32_t)sizeof(swb_ms_lds);
      out->waves_per_simd = 0;
    }
    out->run_list_bytes = 0;
    out->frame_cache_bytes = 0;
    out->split_bands = 0;
    out->split_pad_ = 0;
    return SWB_OK;
  }
  const variant* v = pick_variant(h->p.Wc);
  if (!v) return fail(SWB_ERR_INVALID, "canvas %dx%d not supported", h->p.Wc, h->p.Hc);
  int vs = 0;
  (void)pick_resample(h->p.AA, h->vslots, &vs);
  out->nw = v->nw; out->ncol = 1; out->vs = vs;
  out->lds_bytes_per_wave = (int32_t)lds_per_wave(h, v, nullptr);
  out->waves_per_simd = SWB_COVER_WAVES(v->nw);
  out->resample_waves_per_simd = SWB_RS_WAVES_PER_SIMD;
  // (split bands: the nominal count is one; the count the lists are cut into -- once the tables exist, the one placed -- is split_bands)
  out->n_bands = h->split_bands ? 1 : (h->p.nbands ? h->p.nbands : h->nbands);
  out->split_bands = h->split_bands ? (h->p.nbands ? h->p.nbands : h->nbands) : 0;
  out->split_pad_ = 0;
  out->n_column_groups = h->p.ncg;
  out->run_cap = h->p.run_cap;
  out->paint_in_cover = paints_in_cover(h, v) ? 1 : 0;
  out->arena_units = h->d_runs ? h->p.arena_units : 0;
  out->large_frames = 0;
  out->many_sprites = 0;
  out->reserved_ = 0;
  out->run_list_bytes = h->d_runs ? ((int64_t)h->p.arena_base + h->p.arena_units + 4) * 8 : 0;
  out->frame_cache_bytes = (int64_t)h->d_frame_cache.count;
  return SWB_OK;
}

#ifndef SWB_BUILD_ID
#define SWB_BUILD_ID "unknown"
#endif
const char* swb_build_id(void) { return SWB_BUILD_ID; }

int swb_timing_enable(swb_handle h, int32_t enable) {
  if (!h) return fail(SWB_ERR_INVALID, "null handle");
  HIP_TRY(hipSetDevice(h->device));
  if (flush_timing(h)) return SWB_ERR_HIP;
  h->timing = enable != 0;
  h->timed_ms = 0.0;
  h->timed_cover_ms = 0.0;
  h->timed_launches = 0;
  return SWB_OK;
}

int swb_step_time_ms(swb_handle h, double* total_ms, int64_t* launches) {
  if (!h) return fail(SWB_ERR_INVALID, "null handle");
  HIP_TRY(hipSetDevice(h->device));
  if (flush_timing(h)) return SWB_ERR_HIP;
  if (total_ms) *total_ms = h->timed_ms;
  if (launches) *launches = h->timed_launches;
  return SWB_OK;
}

int swb_kernel_times_ms(swb_handle h, double* cover_ms, double* resample_ms, int64_t* launches) {
  if (!h) return fail(SWB_ERR_INVALID, "null handle");
  HIP_TRY(hipSetDevice(h->device));
  if (flush_timing(h)) return SWB_ERR_HIP;
  if (cover_ms) *cover_ms = h->timed_cover_ms;
  if (resample_ms) *resample_ms = h->timed_ms - h->timed_cover_ms;
  if (launches) *launches = h->timed_launches;
  return SWB_OK;
}

}  // extern "C"
